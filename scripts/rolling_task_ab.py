#!/usr/bin/env python3
"""What the RollingTask / OmniwheelTask rows cost on the MI355X, measured in ONE process (profiles/rolling_task_ab.json), by
the method of scripts/com_task_ab.py: warmed, alternated, medians of 20, HIP events around the kernels and the control steps,
the host clock around whole calls (they end in a device synchronise).

  kernels   pinkhip_rolling_tasks_device at 1 / 4 / 8 wheels beside pinkhip_fk_frame_tasks_device at four frames, same model
            and configurations.  To confirm or refute: the pose phase dominates, so 8 wheels cost well under 8 x one.
  api       the whole solve_ik_batch call on the hybrid route (device_kinematics="frame_rows") with the four wheels, beside
            the same stack on the all-host route (ONE sample) and the hybrid call without the wheels
  step      one DeviceRollout(fused=True) step with and without the four wheels, alternated

at B = 65 536 on a 30-dof floating-base stand-in with four wheels: a free-flyer and four legs of six revolute joints
(nj = 25, nv = 30), the hubs on the legs' last joints, one tilted floor on the world.

    python scripts/rolling_task_ab.py [-o out.json] [--batch 65536] [--repeats 20]
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


def wheeled_stand_in(seed=4):
    """Free-flyer + 4 legs x 6 revolute joints; frames hub0..hub3 on the last joints, "base" on the root, "floor" on the world."""
    from pink_amd.configuration import Model
    from pink_amd.lie import SE3, exp3

    rng = np.random.default_rng(seed)
    m = Model()
    root = m.add_joint("root_joint", "free_flyer")
    for leg in range(4):
        parent = root
        for i in range(6):
            off = [0.2 * (1 - 2 * (leg // 2)), 0.15 * (1 - 2 * (leg % 2)), -0.05] if i == 0 else 0.3 * rng.normal(size=3) / np.sqrt(3)
            parent = m.add_joint(f"leg{leg}_{i}", "revolute", parent, SE3(exp3(0.5 * rng.normal(size=3)), off), rng.normal(size=3), -3.0, 3.0, 3.0)
        m.add_frame(f"hub{leg}", parent, SE3(exp3([0.1, -0.2, 0.15]), [0.03, 0.01, -0.02]))
    m.add_frame("base", root, SE3())
    m.add_frame("floor", -1, SE3(exp3([0.3, 0.1, 0.0]), [0.0, 0.0, -0.6]))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "rolling_task_ab.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g

    g.build_hip()
    import pink_amd
    from pink_amd import Configuration, ConfigurationBatch, FrameTask, OmniwheelTask, PostureTask, RollingTask, solve_ik_batch
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.rollout import DeviceRollout, ModelArrays, pose12
    from pink_amd.runtime import set_default_solver

    B, R = a.batch, a.repeats
    rng = np.random.default_rng(1)
    m = wheeled_stand_in()
    nv, nq = m.nv, m.nq
    hubs = [f"hub{i}" for i in range(4)]
    radii = [0.05, 0.1, 0.15, 0.2]
    wheels = [(OmniwheelTask if i % 2 else RollingTask)(hubs[i], "floor", radii[i], 1.0, gain=0.5, lm_damping=1e-3) for i in range(4)]
    q = rng.uniform(-0.8, 0.8, size=(B, nq))
    q[:, 3:7] = rng.normal(size=(B, 4))
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    api = BatchSolver(0)
    set_default_solver(api)
    out = {"B": B, "repeats": R, "source_hash": g._source_hash(g.HIP_DEPS), "model": {"nj": len(m.joints), "nv": nv, "wheels": 4}}
    try:
        # ---- kernels ----------------------------------------------------------------------------------------------------------
        farr = ModelArrays(m, hubs)  # (kept: the descriptors point into their arrays)
        rarr = ModelArrays(m, [(h, "floor") for h in hubs])
        fm, rm = api.model_create(farr.desc), api.model_create(rarr.desc)
        Kd = 24
        Tt = np.tile(np.array([pose12(Configuration(m, q[0]).get_transform_frame_to_world(h)) for h in hubs]), (B, 1, 1))
        d_q, d_Tt, d_e, d_J, d_z = (api.alloc(8 * n) for n in (B * nq, Tt.size, B * Kd, B * Kd * nv, B * 8))
        api.put(d_q, q), api.put(d_Tt, Tt)
        calls = {"fk_frame_tasks_4_frames": lambda: api.fk_frame_tasks(fm, B, d_q, d_Tt, None, d_e, Kd, d_J, Kd * nv)}
        for n in (1, 4, 8):
            slots, kinds, rad = [i % 4 for i in range(n)], [0] * n, [radii[i % 4] for i in range(n)]
            calls[f"rolling_tasks_{n}_wheels"] = (lambda s=slots, k=kinds, r=rad: api.rolling_tasks(rm, B, d_q, s, k, r, d_e, Kd, d_J, Kd * nv, 0, d_z))
        times = {k: [] for k in calls}
        for i in range(R + 3):  # (three rounds of warm-up)
            for k, fn in calls.items():
                api.timer_start()
                fn()
                ms = api.timer_stop()
                if i >= 3:
                    times[k].append(ms)
        # the rows the last timed launch (8 wheels) wrote, against the host class (a check that the timed kernel did the work)
        api.sync()
        J, z = np.empty((B, Kd * nv)), np.empty((B, 8))
        api.get(J, d_J), api.get(z, d_z)
        worst = 0.0
        for b in range(4):
            cfg = Configuration(m, q[b])
            for w in range(8):
                t = RollingTask(hubs[w % 4], "floor", radii[w % 4], 1.0)
                worst = max(worst, float(np.abs(J[b].reshape(Kd, nv)[3 * w:3 * w + 3] - t.compute_jacobian(cfg)).max()),
                            float(abs(z[b, w] - (t.compute_error(cfg)[2] + t.wheel_radius))))
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["kernels"] = {k: stats(v) for k, v in times.items()}
        out["kernels"].update({"lanes_per_robot": 32, "rows_vs_host_max_abs": worst,
                               "rolling_4_over_fk_4_frames_median": med["rolling_tasks_4_wheels"] / med["fk_frame_tasks_4_frames"],
                               "rolling_8_over_rolling_1_median": med["rolling_tasks_8_wheels"] / med["rolling_tasks_1_wheels"],
                               "rolling_4_over_rolling_1_median": med["rolling_tasks_4_wheels"] / med["rolling_tasks_1_wheels"]})
        for p in (d_q, d_Tt, d_e, d_J, d_z):
            api.release(p)
        api.model_destroy(fm), api.model_destroy(rm)
        # ---- the whole solve_ik_batch call ------------------------------------------------------------------------------------
        ft = FrameTask("base", 1.0, 1.0, lm_damping=1e-3)
        ft.set_target(Configuration(m, q[0]).get_transform_frame_to_world("base"))
        post = PostureTask(cost=1e-1)
        post.set_target(m.neutral())
        cb = ConfigurationBatch(m, q)
        dt = 5e-3
        t_without, t_with = [], []
        for i in range(R + 2):
            for stack, ts in (([ft, post], t_without), ([ft] + wheels + [post], t_with)):
                t0 = time.perf_counter()
                solve_ik_batch(cb, stack, dt, device_kinematics="frame_rows")
                ms = 1e3 * (time.perf_counter() - t0)
                assert pink_amd.last_solve_stats()["route"] == "hybrid"
                if i >= 2:
                    ts.append(ms)
        out["api_hybrid_call"] = {"without_wheels": stats(t_without), "with_4_wheels": stats(t_with),
                                  "difference_of_medians_ms": float(np.median(t_with) - np.median(t_without)),
                                  "clock": "host clock around solve_ik_batch (uploads, kernels, downloads, Python)"}
        t0 = time.perf_counter()
        solve_ik_batch(cb, [ft] + wheels + [post], dt, device_kinematics=False)
        out["api_host_evaluated_call"] = {"with_4_wheels_ms": 1e3 * (time.perf_counter() - t0), "n": 1, "route": pink_amd.last_solve_stats()["route"]}
        pink_amd.clear_device_cache()
        # ---- one fused=True control step ---------------------------------------------------------------------------------------
        specs = [("base", 1.0, 1.0, 1.0, 1e-3)]
        Tb = np.tile(pose12(Configuration(m, q[0]).get_transform_frame_to_world("base")), (B, 1, 1))
        ros = [DeviceRollout(api, m, q, specs, dt, posture_cost=1e-1, fused=True, rolling_tasks=w) for w in ((), wheels)]
        for ro in ros:
            ro.set_targets(Tb)
        t_plain, t_wheels = [], []
        for i in range(R + 3):
            for ro, ts in zip(ros, (t_plain, t_wheels)):
                api.timer_start()
                ro.step()
                ms = api.timer_stop()
                if i >= 3:
                    ts.append(ms)
        for ro in ros:
            _, st, _ = ro.last_step()
            assert (st == 0).all()
            ro.free()
        out["fused_step"] = {"without_wheels": stats(t_plain), "with_4_wheels": stats(t_wheels),
                             "difference_of_medians_ms": float(np.median(t_wheels) - np.median(t_plain)), "clock": "HIP events around DeviceRollout.step()"}
    finally:
        set_default_solver(None)
        api.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
