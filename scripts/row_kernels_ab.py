#!/usr/bin/env python3
"""Speed and bits of the nine stand-alone row kernels -- ik_com_task_kernel, ik_manipulability_task_kernel and
ik_rolling_tasks_kernel at 8 / 32 / 64 lanes per robot -- of this tree's library against another build of it (the parent's),
on one MI355X (profiles/row_prologue_ab.json).

    python scripts/row_kernels_ab.py --parent <parent>/pink_amd/csrc/libpinkhip.so [-o out.json] [--batch 65536] [--repeats 20]

Seven fresh processes, one at a time, parent / this tree alternated, first and last the parent; each under its own time
limit, PINKHIP_LIBRARY picks the library, and the first that fails ends the run.  Each launches every kernel on a model
of tests/*_cases.py at B = 65 536 on seeded configurations: three launches of warm-up, the median of 20 by HIP events, and
the sha256 of the e and J buffers.

  time  this tree's median over its three runs <= the parent's over its four + (max - min) of the parent's four: nothing
        smaller than the parent's own run-to-run spread can be told apart on a shared machine
  bits  the digests of every run are equal
Exit status 1 when a kernel misses either.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_SECONDS = 240


def child(B, R):
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.rollout import ModelArrays
    from tests import com_task_cases as cc
    from tests import manipulability_cases as mc
    from tests import rolling_cases as rc
    from tests.row_kernel_kit import random_configurations

    api = BatchSolver(0)
    out = {"ms": {}, "sha256": {}}

    def run(key, model, arr, rows, launch):
        """launch(dm, d_q, d_e, sE, d_J, sJ) on seeded configurations; e / J start as zeros"""
        nv = model.nv
        q = random_configurations(model, B, np.random.default_rng(11))
        e, J = np.zeros((B, rows)), np.zeros((B, rows * nv))
        dm = api.model_create(arr.desc)
        d_q, d_e, d_J = (api.alloc(8 * a.size) for a in (q, e, J))
        api.put(d_q, q), api.put(d_e, e), api.put(d_J, J)
        ms = []
        for i in range(R + 3):
            api.timer_start()
            launch(dm, d_q, d_e, rows, d_J, rows * nv)
            t = api.timer_stop()
            if i >= 3:
                ms.append(t)
        api.sync()
        api.get(e, d_e), api.get(J, d_J)
        out["ms"][key] = float(np.median(ms))
        out["sha256"][key] = {"e": hashlib.sha256(e.tobytes()).hexdigest(), "J": hashlib.sha256(J.tobytes()).hexdigest()}
        for p in (d_q, d_e, d_J):
            api.release(p)
        api.model_destroy(dm)

    try:
        for W, name in ((8, "arm6"), (32, "tree12"), (64, "tree34")):
            model, frames = cc.models()[name]
            dc, d_t = [], api.alloc(24)
            api.put(d_t, np.array([0.1, -0.2, 0.3]))

            def launch(dm, d_q, d_e, sE, d_J, sJ):
                if not dc:
                    dc.append(api.com_create(dm, *model.mass_tables()))
                api.com_task(dm, dc[0], B, d_q, d_t, False, d_e, sE, d_J, sJ, 0, None)

            run(f"com_{W}", model, ModelArrays(model, frames), 3, launch)
            api.com_destroy(dc[0])
            api.release(d_t)
        for W, name in ((8, "arm6"), (32, "tree12"), (64, "tree36")):
            mname, frame, rf, mask, _, _ = mc.CASES[name]
            model, frames = mc.models()[mname]
            f, bits = frames.index(frame), mc.mask_bits(mask)
            run(f"manipulability_{W}", model, ModelArrays(model, frames), 1,
                lambda dm, d_q, d_e, sE, d_J, sJ: api.manipulability_task(dm, B, d_q, f, int(rf), bits, 0.1, d_e, sE, d_J, sJ, 0, None))
        for W, name in ((8, "biped"), (32, "quad"), (64, "tree34")):
            model, wheels = rc.models()[name]
            assert rc.WIDTH[name] == W
            kinds, radii = [w[0] for w in wheels], [w[3] for w in wheels]
            run(f"rolling_{W}", model, rc.arrays(name), rc.rows_of(kinds),
                lambda dm, d_q, d_e, sE, d_J, sJ: api.rolling_tasks(dm, B, d_q, list(range(len(kinds))), kinds, radii, d_e, sE, d_J, sJ, 0, None))
    finally:
        api.close()
    print("ROW_KERNELS_AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build's libpinkhip.so")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "row_prologue_ab.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.batch, a.repeats)
    libs = {"parent": os.path.abspath(a.parent), "tree": os.path.join(ROOT, "pink_amd", "csrc", "libpinkhip.so")}
    runs = []
    for who in ("parent", "tree") * 3 + ("parent",):
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch),
               "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, env=dict(os.environ, PINKHIP_LIBRARY=libs[who]), capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW_KERNELS_AB ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-2000:], f"run {len(runs)} ({who}) ended with status {p.returncode}: stopping", sep="\n")
            return 2
        runs.append(dict(library=who, **json.loads(line[0].split(" ", 1)[1])))
        print(who, {k: round(v, 4) for k, v in runs[-1]["ms"].items()}, flush=True)
    report, ok = {"B": a.batch, "repeats": a.repeats, "order": [r["library"] for r in runs], "kernels": {}}, True
    for key in runs[0]["ms"]:
        ms = {who: [r["ms"][key] for r in runs if r["library"] == who] for who in libs}
        bar = float(np.median(ms["parent"]) + max(ms["parent"]) - min(ms["parent"]))
        digests = {json.dumps(r["sha256"][key], sort_keys=True) for r in runs}
        k = {"median_ms_per_run": ms, "parent_median_ms": float(np.median(ms["parent"])), "tree_median_ms": float(np.median(ms["tree"])),
             "bar_ms": bar, "time_ok": bool(np.median(ms["tree"]) <= bar), "sha256": runs[0]["sha256"][key],
             "runs_with_other_sha256": {f"{i} ({r['library']})": r["sha256"][key] for i, r in enumerate(runs) if r["sha256"][key] != runs[0]["sha256"][key]},
             "bits_equal": len(digests) == 1}
        ok = ok and k["time_ok"] and k["bits_equal"]
        report["kernels"][key] = k
        print(f"{key:18s} parent {k['parent_median_ms']:.4f} tree {k['tree_median_ms']:.4f} bar {bar:.4f} ms "
              f"{'ok' if k['time_ok'] else 'SLOWER'}, bits {'equal' if k['bits_equal'] else 'DIFFER'}")
    report["ok"] = ok
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
