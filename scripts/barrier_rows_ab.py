#!/usr/bin/env python3
"""What the barrier rows cost on the MI355X, measured in ONE process (profiles/barrier_rows_ab.json), by the method of
scripts/rolling_task_ab.py: warmed, alternated, medians of 20, HIP events around the kernels and the control steps, the host
clock around whole calls (they end in a device synchronise).

  kernels   pinkhip_barrier_rows_device with 6 position rows + 1 spherical row + 8 sphere pairs / 4 rows beside
            pinkhip_rolling_tasks_device at four wheels, same model and configurations
  api       the whole solve_ik_batch call on the hybrid route (device_kinematics="frame_rows") for 4 FrameTasks + posture +
            ComTask, without barriers, with the position and spherical barriers, and with the SelfCollisionBarrier too, at
            B = 1 024 and at --batch.  To confirm or refute: where the host evaluates the barriers the call is dominated by
            that evaluation; where the device forms them the call stays within a small multiple of the stack without barriers.
  step      one DeviceRollout(fused=True) step with and without the barriers, alternated

on the 30-dof floating-base stand-in of scripts/rolling_task_ab.py (nj = 25, nv = 30) with a mass on every joint.

The script runs on any tree that has the hybrid route with a ComTask: on a tree without pinkhip_barrier_rows_device (the
parent of the commit that added it) the kernel and step sections are skipped, the api section measures the host evaluation
of the barriers, and the SelfCollisionBarrier case is run at B = 1 024 only (--host-pairs-batch).

    python scripts/barrier_rows_ab.py [-o out.json] [--batch 65536] [--repeats 20] [--label this]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    ms = np.asarray(ms, dtype=float)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "barrier_rows_ab.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3, help="samples of a call whose barriers the host evaluates")
    ap.add_argument("--host-pairs-batch", type=int, default=1024, help="largest batch at which the host evaluates a SelfCollisionBarrier")
    ap.add_argument("--label", default="this", help="key of this run's block in the output file (merged into it)")
    ap.add_argument("--no-build", action="store_true", help="use the library as it is")
    a = ap.parse_args()
    import __graft_entry__ as g

    if not a.no_build:
        g.build_hip()
    import pink_amd
    from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, PostureTask, solve_ik_batch
    from pink_amd.barriers import BodySphericalBarrier, PositionBarrier, SelfCollisionBarrier
    from pink_amd.barriers.self_collision_barrier import SpherePairs
    from pink_amd.batch_solver import BatchSolver
    from pink_amd.rollout import DeviceRollout, ModelArrays, pose12, sphere_pair_tables
    from pink_amd.runtime import set_default_solver
    from rolling_task_ab import wheeled_stand_in

    B, R = a.batch, a.repeats
    rng = np.random.default_rng(1)
    m = wheeled_stand_in()
    for j in m.joints:
        j.mass, j.com = float(rng.uniform(0.5, 3.0)), 0.05 * rng.normal(size=3)
    nv, nq = m.nv, m.nq
    hubs = [f"hub{i}" for i in range(4)]
    leg_end = [m.frames[m.getFrameId(h)].joint for h in hubs]
    q = rng.uniform(-0.8, 0.8, size=(B, nq))
    q[:, 3:7] = rng.normal(size=(B, 4))
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    # 6 position rows (a box around hub0: nothing within 50 of it), 1 spherical row, 8 sphere pairs of which 4 are kept
    box = PositionBarrier("hub0", indices=[0, 1, 2], p_min=np.full(3, -50.0), p_max=np.full(3, 50.0), gain=np.ones(6))
    sph = BodySphericalBarrier(("hub1", "hub2"), d_min=0.01, gain=1.0)
    spheres = [(leg_end[i] - k, [0.01 * (i + 1), -0.02, 0.01 * k], 0.01) for i in range(4) for k in (0, 2)]
    pairs = [(*spheres[i], *spheres[j]) for i, j in ((0, 2), (0, 4), (0, 6), (2, 4), (2, 6), (4, 6), (1, 3), (5, 7))]
    sc = SelfCollisionBarrier(4, gain=1.0, d_min=0.0, distance_query=SpherePairs(pairs))
    api = BatchSolver(0)
    set_default_solver(api)
    device = hasattr(api, "barrier_rows")
    out = {"B": B, "repeats": R, "source_hash": g._source_hash(g.HIP_DEPS), "barrier_rows_on_the_device": device,
           "model": {"nj": len(m.joints), "nv": nv, "position_rows": 6, "spherical_rows": 1, "sphere_pairs": 8, "pair_rows": 4}}
    try:
        # ---- kernels ----------------------------------------------------------------------------------------------------------
        if device:
            from pink_amd._lib import BarrierRowsArgs
            from pink_amd.rollout import barrier_row_tables, sphere_pairs_args

            frames = ["hub0", "hub1", "hub2"]
            barr, rarr = ModelArrays(m, frames), ModelArrays(m, [(h, "floor") for h in hubs])  # (kept: the descriptors point into them)
            bm, rm = api.model_create(barr.desc), api.model_create(rarr.desc)
            lists, _, _ = barrier_row_tables([box, sph], lambda f, what: frames.index(f))
            held = []

            def up(arr):
                p = api.alloc(max(arr.nbytes, 8))
                api.put(p, arr)
                held.append(p)
                return p

            br = BarrierRowsArgs()
            br.n_rows = 7
            br.frame, br.axis, br.sign, br.bound, br.gain, br.frame2 = (
                up(np.ascontiguousarray(v, dtype=t)) for v, t in zip(lists, (np.int32, np.int32, np.float64, np.float64, np.float64, np.int32)))
            host = sphere_pair_tables(m, pairs)
            sp = sphere_pairs_args([up(t) for t in host], host, sc)
            md, Kd = 11, 12
            d_q, d_G, d_h, d_d, d_e, d_J, d_z = (up(np.zeros(n)) for n in (B * nq, B * md * nv, B * md, B * 4, B * Kd, B * Kd * nv, B * 4))
            api.put(d_q, q)
            radii = [0.05, 0.1, 0.15, 0.2]
            calls = {
                "barrier_rows_7_rows_8_pairs_4_kept": lambda: api.barrier_rows(bm, B, d_q, 5e-3, br, sp, d_G, md * nv, d_h, md, 0, d_d),
                "barrier_rows_7_rows": lambda: api.barrier_rows(bm, B, d_q, 5e-3, br, None, d_G, md * nv, d_h, md, 0, None),
                "rolling_tasks_4_wheels": lambda: api.rolling_tasks(rm, B, d_q, [0, 1, 2, 3], [0] * 4, radii, d_e, Kd, d_J, Kd * nv, 0, d_z),
            }
            times = {k: [] for k in calls}
            for i in range(R + 3):  # (three rounds of warm-up)
                for k, fn in calls.items():
                    api.timer_start()
                    fn()
                    ms = api.timer_stop()
                    if i >= 3:
                        times[k].append(ms)
            # the rows of the first instances against the host classes (a check that the timed kernel did the work)
            api.sync()
            calls["barrier_rows_7_rows_8_pairs_4_kept"]()
            api.sync()
            G, h = np.empty((B, md, nv)), np.empty((B, md))
            api.get(G, d_G), api.get(h, d_h)
            worst = 0.0
            for b in range(4):
                cfg = Configuration(m, q[b])
                Gs, hs = zip(*(bar.compute_qp_inequalities(cfg, 5e-3) for bar in (box, sph, sc)))
                Gh, hh = np.vstack(Gs), np.hstack(hs)
                order = list(range(7)) + [7 + int(i) for i in np.argsort(hh[7:], kind="stable")]
                worst = max(worst, float(np.abs(G[b] - Gh[order]).max() / np.abs(Gh).max()), float(np.abs(h[b] - hh[order]).max()))
            med = {k: float(np.median(v)) for k, v in times.items()}
            out["kernels"] = {k: stats(v) for k, v in times.items()}
            out["kernels"].update({"lanes_per_robot": 32, "rows_vs_host_max_rel": worst, "clock": "HIP events around the call",
                                   "barrier_rows_over_rolling_4_wheels_median": med["barrier_rows_7_rows_8_pairs_4_kept"] / med["rolling_tasks_4_wheels"]})
            for p in held:
                api.release(p)
            api.model_destroy(bm), api.model_destroy(rm)
        # ---- the whole solve_ik_batch call ------------------------------------------------------------------------------------
        dt = 5e-3
        out["api_hybrid_call"] = {"clock": "host clock around solve_ik_batch (uploads, kernels, downloads, Python)"}
        for Bc in sorted({1024, B}):
            qc = np.ascontiguousarray(q[:Bc])
            cfg0 = Configuration(m, qc[0])
            fts = []
            for hname in hubs:
                ft = FrameTask(hname, 1.0, 0.0, lm_damping=1e-3)
                ft.set_target(cfg0.get_transform_frame_to_world(hname))
                fts.append(ft)
            post = PostureTask(cost=1e-1)
            post.set_target(m.neutral())
            com = ComTask(1.0, lm_damping=1e-3)
            com.set_target(cfg0.center_of_mass())
            cb = ConfigurationBatch(m, qc)
            stack = fts + [com, post]
            cases = {"without_barriers": None, "position_and_spherical": [box, sph]}
            if device or Bc <= a.host_pairs_batch:
                cases["with_sphere_pairs"] = [box, sph, sc]
            ts = {k: [] for k in cases}
            where = {}
            reps = R if device else a.host_repeats
            for i in range(reps + 1):  # (one round of warm-up)
                for k, bars in cases.items():
                    t0 = time.perf_counter()
                    solve_ik_batch(cb, stack, dt, barriers=bars, device_kinematics="frame_rows")
                    ms = 1e3 * (time.perf_counter() - t0)
                    s = pink_amd.last_solve_stats()
                    assert s["route"] == "hybrid" and s["failed"] == 0, s
                    where[k] = s.get("barrier_rows", "host" if bars else None)
                    if i >= 1:
                        ts[k].append(ms)
            blk = {k: dict(stats(v), barrier_rows=where[k]) for k, v in ts.items()}
            base = blk["without_barriers"]["median_ms"]
            for k in cases:
                blk[k]["over_without_barriers"] = blk[k]["median_ms"] / base
            blk["run_to_run_spread_without_barriers"] = (blk["without_barriers"]["max_ms"] - blk["without_barriers"]["min_ms"]) / base
            out["api_hybrid_call"][f"B_{Bc}"] = blk
            pink_amd.clear_device_cache()
        # ---- one fused=True control step ---------------------------------------------------------------------------------------
        if device:
            specs = [(hname, 1.0, 0.0, 1.0, 1e-3) for hname in hubs]
            Tb = np.tile(np.array([pose12(Configuration(m, q[0]).get_transform_frame_to_world(hname)) for hname in hubs]), (B, 1, 1))
            com = ComTask(1.0, lm_damping=1e-3)
            com.set_target(Configuration(m, q[0]).center_of_mass())
            ros = [DeviceRollout(api, m, q, specs, dt, posture_cost=1e-1, fused=True, com_task=com, position_barriers=bars) for bars in ((), [box, sph, sc])]
            for ro in ros:
                ro.set_targets(Tb)
            t_plain, t_bars = [], []
            for i in range(R + 3):
                for ro, ts in zip(ros, (t_plain, t_bars)):
                    api.timer_start()
                    ro.step(integrate=False)
                    ms = api.timer_stop()
                    if i >= 3:
                        ts.append(ms)
            for ro in ros:
                _, st, _ = ro.last_step()
                assert (st == 0).all()
                ro.free()
            out["fused_step"] = {"without_barriers": stats(t_plain), "with_barriers": stats(t_bars),
                                 "difference_of_medians_ms": float(np.median(t_bars) - np.median(t_plain)), "clock": "HIP events around DeviceRollout.step()"}
    finally:
        set_default_solver(None)
        api.close()
    have = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            have = json.load(f)
    have[a.label] = out
    with open(a.out, "w") as f:
        json.dump(have, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
