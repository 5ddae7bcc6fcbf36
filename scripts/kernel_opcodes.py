#!/usr/bin/env python3
"""Where kernels of two builds of one object differ: per kernel whose name contains one of --match, the opcode histogram
of A against B (llvm-objdump -d of the gfx950 code object) and the metadata rows (scripts/kernel_meta.py).

    python scripts/kernel_opcodes.py A/build/pinkhip.o B/build/pinkhip.o --match ik_com_task_kernel ... [-o out.json]

The opcodes that decide the arithmetic and the memory traffic -- PINNED below -- must occur equally often in A and B, and
nothing may spill or use scratch: exit status 1 otherwise.  Everything else (moves, scalar control) is reported.
"""
import argparse
import collections
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_meta import LLVM, kernels  # noqa: E402

PINNED = ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_rcp", "v_rsq", "v_sqrt", "ds_", "global_", "s_load", "s_barrier")
ZERO = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def histograms(path):
    """{kernel symbol: Counter of opcodes} of the first gfx950 code object bundled in `path`"""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(path))
        shutil.copy(path, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
        co = sorted(glob.glob(local + ".*gfx950*"))[0]
        out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for ln in out.splitlines():
        if ln.endswith(">:") and "<" in ln:
            cur = res.setdefault(ln.split("<", 1)[1][:-2], collections.Counter())
        elif cur is not None and ln.strip():
            cur[ln.split()[0]] += 1
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj_a"), ap.add_argument("obj_b")
    ap.add_argument("--match", nargs="+", required=True)
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    ha, hb = histograms(a.obj_a), histograms(a.obj_b)
    ma, mb = ({k["name"]: k for k in kernels(p)} for p in (a.obj_a, a.obj_b))
    report, ok = {"object": os.path.basename(a.obj_a), "pinned_prefixes": PINNED, "kernels": {}}, True
    for name in sorted(k for k in ha if any(s in k for s in a.match) and not k.endswith(".kd")):
        x, y = ha[name], hb.get(name, collections.Counter())
        diff = {op: [x[op], y[op]] for op in sorted(set(x) | set(y)) if x[op] != y[op]}
        pinned = {op: v for op, v in diff.items() if op.startswith(PINNED)}
        meta = {f: [int(ma[name].get(f, 0)), int(mb[name].get(f, 0))] for f in ("vgpr_count", "sgpr_count") + ZERO}
        good = not pinned and all(meta[f] == [0, 0] for f in ZERO)
        ok = ok and good
        report["kernels"][name] = {"instructions": [sum(x.values()), sum(y.values())], "metadata_a_b": meta, "pinned_opcodes_differing": pinned,
                                   "other_opcodes_differing_a_b": {op: v for op, v in diff.items() if op not in pinned}, "ok": good}
        print(f"{name}: {'ok' if good else 'DIFFERS'} vgpr {meta['vgpr_count']} instructions {report['kernels'][name]['instructions']} pinned {pinned}")
    report["ok"] = ok and bool(report["kernels"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0 if report["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
