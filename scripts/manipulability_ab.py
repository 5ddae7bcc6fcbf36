#!/usr/bin/env python3
"""What the ManipulabilityTask row costs on the MI355X, measured in ONE process (profiles/manipulability_ab.json), by the
method of scripts/com_task_ab.py: warmed, alternated, medians of 20, HIP events around the kernels.

  kernels   pinkhip_manipulability_task_device beside pinkhip_fk_frame_tasks_device (one frame) on the same model: arm6
            (W = 8, eight robots per wavefront) and the 36-joint revolute tree of tests/manipulability_cases.py (W = 64)
  api       the whole solve_ik_batch call on the hybrid route without and with the task, alternated, host clock around the
            call (it ends in a device synchronise)
  host      the same stack with the task on the host-evaluated route (device_kinematics=False), ONE sample

at B = 65 536.

    python scripts/manipulability_ab.py [-o out.json] [--batch 65536] [--repeats 20]
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
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "manipulability_ab.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g

    g.build_hip()
    import pink_amd
    from pink_amd import Configuration, ConfigurationBatch, FrameTask, ManipulabilityTask, PostureTask, solve_ik_batch
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.rollout import ModelArrays, pose12
    from pink_amd.runtime import set_default_solver
    from tests.manipulability_cases import models

    B, R = a.batch, a.repeats
    rng = np.random.default_rng(1)
    api = BatchSolver(0)
    set_default_solver(api)
    out = {"B": B, "repeats": R, "source_hash": g._source_hash(g.HIP_DEPS), "kernels": {}}
    try:
        # ---- kernels ------------------------------------------------------------------------------------------------------
        for name, frame in (("arm6", "tool0"), ("tree36", "hand")):
            m = models()[name][0]
            nv, nq = m.nv, m.nq
            q = rng.uniform(-0.8, 0.8, size=(B, nq))
            arr = ModelArrays(m, [frame])  # (kept: the descriptor points into its arrays)
            dm = api.model_create(arr.desc)
            Kd = 6 + 1
            Tt = np.tile(pose12(Configuration(m, q[0]).get_transform_frame_to_world(frame)), (B, 1, 1))
            d_q, d_Tt, d_e, d_J, d_m = (api.alloc(8 * n) for n in (B * nq, Tt.size, B * Kd, B * Kd * nv, B))
            api.put(d_q, q), api.put(d_Tt, Tt)
            fk = lambda: api.fk_frame_tasks(dm, B, d_q, d_Tt, None, d_e, Kd, d_J, Kd * nv)  # noqa: E731
            mp = lambda: api.manipulability_task(dm, B, d_q, 0, 0, 63, 0.1, d_e, Kd, d_J, Kd * nv, 6, d_m)  # noqa: E731
            t_fk, t_mp = [], []
            for i in range(R + 3):  # (three rounds of warm-up)
                for fn, ts in ((fk, t_fk), (mp, t_mp)):
                    api.timer_start()
                    fn()
                    ms = api.timer_stop()
                    if i >= 3:
                        ts.append(ms)
            # the values the timed launches wrote, against the host class (a check that the timed kernel did the work)
            mv = np.empty(B)
            api.sync()
            api.get(mv, d_m)
            t = ManipulabilityTask(frame, m)
            m_host = np.array([t.compute_manipulability(Configuration(m, q[b])) for b in range(4)])
            out["kernels"][name] = {"nj": len(m.joints), "nv": nv, "lanes_per_robot": 8 if max(nv, len(m.joints)) <= 8 else 32 if max(nv, len(m.joints)) <= 32 else 64,
                                    "fk_frame_tasks_1_frame": stats(t_fk), "manipulability_task": stats(t_mp),
                                    "manipulability_over_fk_median": float(np.median(t_mp) / np.median(t_fk)),
                                    "m_vs_host_max_rel": float(np.abs(mv[:4] / m_host - 1.0).max())}
            for p in (d_q, d_Tt, d_e, d_J, d_m):
                api.release(p)
            api.model_destroy(dm)
        # ---- the whole solve_ik_batch call ------------------------------------------------------------------------------------
        m = models()["arm6"][0]
        q = rng.uniform(-0.8, 0.8, size=(B, m.nq))
        ft = FrameTask("tool0", 1.0, 1.0, lm_damping=1e-3)
        T0 = Configuration(m, q[0]).get_transform_frame_to_world("tool0")
        ft.set_target(T0)
        post = PostureTask(cost=1e-1)
        post.set_target(m.neutral())
        mt = ManipulabilityTask("tool0", m, cost=0.5, manipulability_rate=0.1)
        cb = ConfigurationBatch(m, q)
        dt = 5e-3
        t_without, t_with = [], []
        for i in range(R + 2):
            for stack, ts in (([ft, post], t_without), ([ft, mt, post], t_with)):
                t0 = time.perf_counter()
                solve_ik_batch(cb, stack, dt, device_kinematics="frame_rows")
                ms = 1e3 * (time.perf_counter() - t0)
                assert pink_amd.last_solve_stats()["route"] == "hybrid"
                if i >= 2:
                    ts.append(ms)
        out["api_hybrid_call"] = {"without_task": stats(t_without), "with_task": stats(t_with),
                                  "difference_of_medians_ms": float(np.median(t_with) - np.median(t_without)),
                                  "clock": "host clock around solve_ik_batch (uploads, kernels, downloads, Python)"}
        t0 = time.perf_counter()
        solve_ik_batch(cb, [ft, mt, post], dt, device_kinematics=False)
        out["api_host_evaluated_call"] = {"with_task_ms": 1e3 * (time.perf_counter() - t0), "n": 1, "route": pink_amd.last_solve_stats()["route"]}
        pink_amd.clear_device_cache()
    finally:
        set_default_solver(None)
        api.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
