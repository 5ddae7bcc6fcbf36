#!/usr/bin/env python3
"""What the centre-of-mass rows cost on the MI355X, measured in ONE process (profiles/com_task_ab.json):

  kernels   pinkhip_com_task_device against pinkhip_fk_frame_tasks_device at four frames -- the same pose composition,
            then strictly more arithmetic and eight times the rows -- alternated, HIP events, medians of 20
  api       the whole solve_ik_batch call on the hybrid route (device_kinematics="frame_rows") with and without a ComTask,
            alternated, host clock around the call (it ends in a device synchronise)
  step      one DeviceRollout(fused=True) step with and without a ComTask, alternated, HIP events

at B = 65 536 on the nv = 30 humanoid stand-in of bench.py (free flyer + 24 joints) with seeded masses.

    python scripts/com_task_ab.py [-o out.json] [--batch 65536] [--repeats 20]
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
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "com_task_ab.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g

    g.build_hip()
    import pink_amd
    from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, PostureTask, build_chain, solve_ik_batch
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.rollout import DeviceRollout, ModelArrays, pose12
    from pink_amd.runtime import set_default_solver

    B, R = a.batch, a.repeats
    m = build_chain(24, free_flyer=True, seed=2, mass_seed=5)
    frames = ["tool0", "joint_8", "joint_16", "joint_20"]
    nv, nq, nf = m.nv, m.nq, len(frames)
    rng = np.random.default_rng(1)
    q = np.tile(m.neutral(), (B, 1))
    for j in m.joints:
        if j.kind != "free_flyer":
            q[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
    ref = Configuration(m, q[0])
    api = BatchSolver(0)
    set_default_solver(api)
    out = {"B": B, "nv": nv, "nj": len(m.joints), "frames": nf, "repeats": R, "source_hash": g._source_hash(g.HIP_DEPS)}
    try:
        # ---- kernels ----------------------------------------------------------------------------------------------------
        arr = ModelArrays(m, frames)
        dm = api.model_create(arr.desc)
        dc = api.com_create(dm, *m.mass_tables())
        Kd = 6 * nf + 3
        Tt = np.empty((B, nf, 12))
        for k, f in enumerate(frames):
            T0 = ref.get_transform_frame_to_world(f)
            Tt[:, k] = pose12(T0)
            Tt[:, k, 9:] += 0.05 * rng.normal(size=(B, 3))
        d_q, d_Tt, d_e, d_J, d_t = (api.alloc(8 * n) for n in (B * nq, Tt.size, B * Kd, B * Kd * nv, 3))
        api.put(d_q, q), api.put(d_Tt, Tt), api.put(d_t, ref.center_of_mass())
        fk = lambda: api.fk_frame_tasks(dm, B, d_q, d_Tt, None, d_e, Kd, d_J, Kd * nv)  # noqa: E731
        com = lambda: api.com_task(dm, dc, B, d_q, d_t, False, d_e, Kd, d_J, Kd * nv, 6 * nf)  # noqa: E731
        t_fk, t_com = [], []
        for i in range(R + 3):  # (three rounds of warm-up)
            for fn, ts in ((fk, t_fk), (com, t_com)):
                api.timer_start()
                fn()
                ms = api.timer_stop()
                if i >= 3:
                    ts.append(ms)
        # the rows the timed launches wrote, against the host (a check that the timed kernel did the work)
        e = np.empty((B, Kd))
        api.sync()
        api.get(e, d_e)
        c_host = np.array([Configuration(m, q[b]).center_of_mass() for b in range(4)])
        check = float(np.abs(e[:4, 6 * nf:] - (c_host - ref.center_of_mass())).max())
        out["kernels"] = {"fk_frame_tasks_4_frames": stats(t_fk), "com_task": stats(t_com),
                          "com_over_fk_median": float(np.median(t_com) / np.median(t_fk)),
                          "com_rows_vs_host_max_abs": check,
                          "bytes_written_per_instance": {"fk_frame_tasks": 8 * 6 * nf * (nv + 1), "com_task": 8 * 3 * (nv + 1)}}
        for p in (d_q, d_Tt, d_e, d_J, d_t):
            api.release(p)
        api.com_destroy(dc)
        api.model_destroy(dm)
        # ---- the whole solve_ik_batch call on the hybrid route ------------------------------------------------------------
        tasks = []
        for k, f in enumerate(frames):
            t = FrameTask(f, 1.0, 1.0 if k == 0 else 0.0, lm_damping=1e-3)
            t.set_target_poses(Tt[:, k, :9].reshape(B, 3, 3), Tt[:, k, 9:])
            tasks.append(t)
        post = PostureTask(cost=1e-1)
        post.set_target(m.neutral())
        cm = ComTask(1.0, lm_damping=1e-3)
        cm.set_target(ref.center_of_mass() + [0.02, 0.0, 0.01])
        cb = ConfigurationBatch(m, q)
        dt = 5e-3
        t_without, t_with = [], []
        for i in range(R + 2):
            for stack, ts in ((tasks + [post], t_without), (tasks + [cm, post], t_with)):
                t0 = time.perf_counter()
                solve_ik_batch(cb, stack, dt, device_kinematics="frame_rows")
                ms = 1e3 * (time.perf_counter() - t0)
                assert pink_amd.last_solve_stats()["route"] == "hybrid"
                if i >= 2:
                    ts.append(ms)
        out["api_hybrid_call"] = {"without_com_task": stats(t_without), "with_com_task": stats(t_with),
                                  "difference_of_medians_ms": float(np.median(t_with) - np.median(t_without)),
                                  "clock": "host clock around solve_ik_batch (uploads, kernels, downloads, Python)"}
        pink_amd.clear_device_cache()
        # ---- one fused=True control step ---------------------------------------------------------------------------------------
        specs = [(f, 1.0, 1.0 if k == 0 else 0.0, 1.0, 1e-3) for k, f in enumerate(frames)]
        ros = [DeviceRollout(api, m, q, specs, dt, posture_cost=1e-1, fused=True, com_task=c) for c in (None, cm)]
        for ro in ros:
            ro.set_targets(Tt)
        t_plain, t_cm = [], []
        for i in range(R + 3):
            for ro, ts in zip(ros, (t_plain, t_cm)):
                api.timer_start()
                ro.step()
                ms = api.timer_stop()
                if i >= 3:
                    ts.append(ms)
        for ro in ros:
            _, st, _ = ro.last_step()
            assert (st == 0).all()
            ro.free()
        out["fused_true_step"] = {"without_com_task": stats(t_plain), "with_com_task": stats(t_cm),
                                  "difference_of_medians_ms": float(np.median(t_cm) - np.median(t_plain)), "clock": "HIP events around the step's launches"}
    finally:
        set_default_solver(None)
        api.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
