#!/usr/bin/env python3
"""SelfCollisionBarrier rows of sphere pairs formed on chip against the routes that served the barrier before, on one
MI355X -> profiles/self_collision_ab.json.

Stack: floating base + 24 joints (nv = 30), 4 FrameTasks + PostureTask + a SelfCollisionBarrier of 8 sphere pairs over six
spheres that keeps the 4 closest (4 dense rows), default limits.

(a) `solve_ik_batch` per call (uploads, kernel, download and all Python included), device route against the same call forced
    onto the hybrid route (`device_kinematics="frame_rows"`: FrameTask rows on the device, the barrier evaluated on the host
    -- per instance, in Python).  The hybrid route costs milliseconds per INSTANCE there, so the alternated comparison runs
    at `--hybrid-batch`; `--hybrid-full-samples N` adds N hybrid calls at the full batch (minutes each).
(b) the whole-step kernel alone (HIP events around one launch, no integration) with the barrier's 4 rows, beside the same
    stack carrying a 4-row PositionBarrier instead.

Protocol: one process, variants alternated, every variant warmed up, medians of `--samples` (min .. max next to them).
Reads nothing outside the tree.

    python scripts/self_collision_ab.py [--batch 65536] [--samples 20] [--hybrid-batch 1024] [--hybrid-full-samples 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()), "samples": int(ms.size)}


def make_stack(B, seed=1):
    """(model, q [B, nq], frame names, target poses [B, nf, 12], sphere-pair barrier, 4-row position barrier)"""
    from pink_amd import Configuration, build_chain
    from pink_amd.barriers import PositionBarrier, SelfCollisionBarrier
    from pink_amd.barriers.self_collision_barrier import SpherePairs
    from pink_amd.rollout import pose12

    m = build_chain(24, free_flyer=True, seed=2)
    frames = ["tool0", "joint_8", "joint_16", "joint_20"]
    rng = np.random.default_rng(seed)
    q = np.tile(m.neutral(), (B, 1))
    for j in m.joints:
        if j.kind != "free_flyer":
            q[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
    ref = Configuration(m, q[0])
    T = np.zeros((B, len(frames), 12))
    for k, f in enumerate(frames):
        T0 = ref.get_transform_frame_to_world(f)
        T[:, k] = pose12(T0)
        T[:, k, 9:] += 0.05 * rng.normal(size=(B, 3))
    sph = [(j, [0.02, 0.0, 0.01], 0.04) for j in (4, 8, 12, 16, 20, 24)]
    pairs = [sph[a] + sph[b] for a, b in ((0, 2), (0, 3), (1, 3), (1, 4), (2, 4), (2, 5), (0, 5), (1, 5))]
    sc = SelfCollisionBarrier(4, gain=10.0, safe_displacement_gain=1.0, d_min=0.02, distance_query=SpherePairs(pairs))
    p_tool = ref.get_transform_frame_to_world("tool0").translation
    pb = PositionBarrier("tool0", indices=[0, 1], p_min=p_tool[:2] - 2.0, p_max=p_tool[:2] + 2.0, gain=np.array([10.0] * 4), safe_displacement_gain=1.0)
    return m, q, frames, T, sc, pb


def api_calls(B, samples, hybrid_B, hybrid_full):
    import pink_amd
    from pink_amd import ConfigurationBatch, FrameTask, PostureTask, solve_ik_batch

    def problem(n):
        m, q, frames, T, sc, _ = make_stack(n)
        tasks = []
        for k, f in enumerate(frames):
            t = FrameTask(f, 1.0, 1.0 if k == 0 else 0.0, lm_damping=1e-3)
            t.set_target_poses(T[:, k, :9].reshape(n, 3, 3), T[:, k, 9:])
            tasks.append(t)
        post = PostureTask(cost=1e-1)
        post.set_target(m.neutral())
        return ConfigurationBatch(m, q), tasks + [post], sc

    def call(p, route):
        cb, tasks, sc = p
        t0 = time.perf_counter()
        v = solve_ik_batch(cb, tasks, 5e-3, barriers=[sc], device_kinematics=route)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, v, pink_amd.last_solve_stats()

    out = {}
    big = problem(B)
    _, v_dev, st = call(big, True)  # builds the device state
    assert st["route"] == "device", st
    for _ in range(3):
        call(big, True)
    out[f"device_route_B{B}"] = dict(stats([call(big, True)[0] for _ in range(samples)]), route=st["route"], solver_paths=st["paths"])
    print(f"device route, B = {B}: {out[f'device_route_B{B}']['ms_median']:.3f} ms per call", flush=True)
    small = problem(hybrid_B)
    routes = {"device": True, "hybrid": "frame_rows"}
    seen, times, v = {}, {k: [] for k in routes}, {}
    for k, r in routes.items():  # warm-up
        _, v[k], s = call(small, r)
        seen[k] = s["route"]
    assert seen == {"device": "device", "hybrid": "hybrid"}, seen
    for _ in range(samples):
        for k, r in routes.items():
            times[k].append(call(small, r)[0])
    for k in routes:
        out[f"{k}_route_B{hybrid_B}_alternated"] = dict(stats(times[k]), route=seen[k])
    out[f"max_abs_velocity_difference_device_vs_hybrid_B{hybrid_B}"] = float(np.abs(v["device"] - v["hybrid"]).max())
    print(f"B = {hybrid_B}: device {np.median(times['device']):.3f} ms, hybrid {np.median(times['hybrid']):.3f} ms per call", flush=True)
    if hybrid_full > 0:
        ts = []
        for _ in range(hybrid_full):
            ms, v_h, s = call(big, "frame_rows")
            assert s["route"] == "hybrid", s
            ts.append(ms)
        out[f"hybrid_route_B{B}"] = dict(stats(ts), route="hybrid", note="no warm-up call: the route is host-bound (the barrier is evaluated per instance)")
        out[f"max_abs_velocity_difference_device_vs_hybrid_B{B}"] = float(np.abs(v_dev - v_h).max())
    pink_amd.clear_device_cache()
    return out


def kernel_times(solver, B, samples):
    from pink_amd.batch_solver import split_iters
    from pink_amd.rollout import DeviceRollout

    m, q, frames, T, sc, pb = make_stack(B)
    specs = [(f, 1.0, 1.0 if k == 0 else 0.0, 1.0, 1e-3) for k, f in enumerate(frames)]
    ros = {name: DeviceRollout(solver, m, q, specs, 5e-3, posture_cost=1e-1, q_posture=m.neutral(), fused="kernel", position_barriers=[bar])
           for name, bar in (("self_collision_4_of_8_pairs", sc), ("position_barrier_4_rows", pb))}
    out, times = {}, {k: [] for k in ros}
    try:
        for ro in ros.values():
            assert ro.md == 4
            ro.set_targets(T)
            for _ in range(3):
                ro.step(integrate=False)
            solver.sync()
        for _ in range(samples):
            for k, ro in ros.items():
                solver.timer_start()
                ro.step(integrate=False)
                times[k].append(solver.timer_stop())
        for k, ro in ros.items():
            assert ro.fused == "kernel"
            _, st, it = ro.last_step()
            out[k] = dict(stats(times[k]), failed=int((st != 0).sum()), iters_mean=float(it.mean()),
                          share_not_solved_by_the_tableau=float((split_iters(it.copy()) != 0).mean()))
    finally:
        for ro in ros.values():
            ro.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--hybrid-batch", type=int, default=1024)
    ap.add_argument("--hybrid-full-samples", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_collision_ab.json"))
    a = ap.parse_args()
    import __graft_entry__ as g

    g.build_hip()
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.runtime import set_default_solver

    solver = BatchSolver(device_id=0)
    set_default_solver(solver)
    try:
        res = {"stack": "floating base + 24 joints (nv = 30), 4 FrameTasks + PostureTask + SelfCollisionBarrier (8 sphere pairs over 6 spheres, "
                        "n_collision_pairs = 4), default limits, dt = 5 ms",
               "protocol": f"one process, variants alternated, warm-up, medians of {a.samples}",
               "device": solver.device_info().get("name") if hasattr(solver, "device_info") else None,
               "solve_ik_batch_per_call": api_calls(a.batch, a.samples, a.hybrid_batch, a.hybrid_full_samples),
               f"whole_step_kernel_B{a.batch}_hip_events": kernel_times(solver, a.batch, a.samples)}
    finally:
        set_default_solver(None)
        solver.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
