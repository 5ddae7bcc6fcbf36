#!/usr/bin/env python3
"""Cold against warm starts of the tableau solvers on one MI355X -> profiles/warm_start_ab.json.

(a) stack + solve, headline shape (draco3, nv = 30, "tight" bounds), B = 65 536: the kernel's own start (the diagonal
    guess), a warm start from the exact active set, and -- a stand-in for tracking -- a warm start from the set of the
    previous solve after every task error moved by 5 %.
(b) DeviceRollout at bench.py's two closed-loop shapes, box-only (nv = 30; nv = 50 without its barrier rows): the converged
    step and each of the four steps after a 5 cm target move, cold and with warm_start=True.

Protocol: HIP events around single launches / steps, every variant warmed up, 20 timed samples per figure (median and
min .. max), cold and warm alternated inside one process, mean exchange counts next to every time.  Reads nothing outside
the tree.

    python scripts/warm_start_ab.py [--batch 65536] [--samples 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "samples": int(ms.size)}


def stack_solve(solver, B, samples):
    import dataclasses

    from pink_amd import synthetic
    from pink_amd._lib import Warm
    from pink_amd.batch_solver import split_iters

    terms = synthetic.make_terms("draco3", B, bounds="tight")
    batch = synthetic.pack(terms)
    rng = np.random.default_rng(5)
    moved = dataclasses.replace(batch, e=batch.e * (1.0 + 0.05 * rng.normal(size=batch.e.shape)))
    nv = batch.nv
    dev, dev2 = solver.upload(batch), solver.upload(moved)
    d_exact, d_exact2, d_prev, d_out = (solver.alloc(B * nv) for _ in range(4))

    def launch(d, a_in, a_out):
        w = Warm()
        w.active_in, w.active_out = a_in, a_out
        solver.solve_warm_raw(d.args.desc, d.problem, d.result, w)

    def iters(d):
        it = np.zeros(B, np.int32)
        solver.get(it, d.d_iters)
        path = split_iters(it)
        return float(it.mean()), float((path != 0).mean())

    launch(dev, None, d_exact)    # the sets the warm variants start from
    launch(dev, None, d_prev)
    launch(dev2, None, d_exact2)
    solver.sync()
    # (None as the output: the existing cold entry point, pinkhip_solve_device -- the kernel bench.py times -- in the same rotation)
    variants = {
        "existing_cold_entry_point": (dev, None, None),
        "cold_diagonal_guess": (dev, None, d_out),
        "warm_exact_set": (dev, d_exact, d_out),
        "cold_diagonal_guess_errors_moved_5pct": (dev2, None, d_out),
        "warm_previous_set_errors_moved_5pct": (dev2, d_prev, d_out),
        "warm_exact_set_errors_moved_5pct": (dev2, d_exact2, d_out),
    }

    def run(d, a_in, a_out):
        if a_out is None:
            solver.solve_device(d)
        else:
            launch(d, a_in, a_out)

    times = {k: [] for k in variants}
    for v in variants.values():  # warm-up
        for _ in range(3):
            run(*v)
    solver.sync()
    for _ in range(samples):
        for k, v in variants.items():
            solver.timer_start()
            run(*v)
            times[k].append(solver.timer_stop())
    out = {"shape": "draco3 nv=30 tight", "B": B}
    for k, v in variants.items():
        run(*v)
        solver.sync()
        m, off = iters(v[0])
        out[k] = dict(stats(times[k]), exchanges_mean=m, off_tableau_frac=off)
    for p in (d_exact, d_exact2, d_prev, d_out):
        solver.release(p)
    dev.free(), dev2.free()
    return out


def closed_loop(solver, B, samples):
    from pink_amd import build_chain
    from pink_amd.rollout import DeviceRollout

    out = {}
    for label, model, frames in (("nv30_4frames_posture", build_chain(24, free_flyer=True, seed=2), ["tool0", "joint_8", "joint_16", "joint_20"]),
                                 ("nv50_4frames_posture_box_only", build_chain(44, free_flyer=True, seed=4), ["tool0", "joint_10", "joint_20", "joint_30"])):
        rng = np.random.default_rng(1)
        q0 = np.tile(model.neutral(), (B, 1))
        for j in model.joints:
            if j.kind != "free_flyer":
                q0[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
        specs = [(f, 1.0, 1.0 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
        ros = {"cold": DeviceRollout(solver, model, q0, specs, 5e-3, posture_cost=1e-1, fused="kernel"),
               "warm": DeviceRollout(solver, model, q0, specs, 5e-3, posture_cost=1e-1, fused="kernel", warm_start=True)}
        try:
            for ro in ros.values():
                ro.step()
            solver.sync()
            T0 = ros["cold"].frame_poses()
            state = {"away": False}

            def move():
                # every robot's targets move by a few centimetres at once (bench.py, closed_loop_figures): away from the
                # poses the loop started at by a fresh 5 cm draw, and back again
                T = T0.copy()
                state["away"] = not state["away"]
                if state["away"]:
                    T[:, :, 9:12] += 0.05 * rng.normal(size=(B, len(frames), 3))
                for ro in ros.values():
                    ro.set_targets(T)

            move()
            for ro in ros.values():
                ro.run(8, raise_on_failure=False)
            conv = {k: [] for k in ros}
            conv_it = {}
            for _ in range(max(samples, 20)):
                for k, ro in ros.items():
                    solver.timer_start()
                    ro.step()
                    conv[k].append(solver.timer_stop())
            for k, ro in ros.items():
                conv_it[k] = float(ro.last_step()[2].mean())
            after = {k: [[] for _ in range(4)] for k in ros}
            after_it = {k: [[] for _ in range(4)] for k in ros}
            for _ in range(samples):
                move()
                solver.sync()
                for s in range(4):
                    for k, ro in ros.items():
                        solver.timer_start()
                        ro.step()
                        after[k][s].append(solver.timer_stop())
                        after_it[k][s].append(float(ro.last_step()[2].mean()))
                for ro in ros.values():  # back to a converged loop before the next move
                    ro.run(8, raise_on_failure=False)
            rec = {"nv": model.nv, "B": B}
            for k in ros:
                rec[k] = {"converged_step": dict(stats(conv[k]), exchanges_mean=conv_it[k]),
                          "steps_after_a_target_move": [dict(stats(after[k][s]), exchanges_mean=float(np.mean(after_it[k][s]))) for s in range(4)],
                          "failed": int(ros[k].failures()[0].size)}
            dq_c, dq_w = ros["cold"].last_step()[0], ros["warm"].last_step()[0]
            rec["max_abs_dq_difference_last_step"] = float(np.abs(dq_c - dq_w).max())
            out[label] = rec
        finally:
            for ro in ros.values():
                ro.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_start_ab.json"))
    args = ap.parse_args()
    import __graft_entry__ as g
    from pink_amd.batch_solver import BatchSolver

    g.build_hip()
    solver = BatchSolver(0)
    try:
        rec = {"device": solver.device_info()["name"], "source_hash": g._source_hash(g.HIP_DEPS),
               "protocol": "HIP events around single launches / steps; every variant warmed up; cold and warm alternated in one process; "
                           f"{args.samples} samples per figure (median, min, max)",
               "stack_solve": stack_solve(solver, args.batch, args.samples),
               "closed_loop": closed_loop(solver, args.batch, args.samples)}
    finally:
        solver.close()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
