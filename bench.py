#!/usr/bin/env python3
"""Headline benchmark: batched IK-QP solves/s on MI355X (BASELINE.json metric).  No PyTorch.

One "step" = one pass of the hot path (stack H, c + solve the QP) over one synthetic batch that is
already resident in HBM.  N = 1: BASELINE.json config 3 (Draco3-shaped, nv = 30, 4 FrameTasks +
PostureTask + joint/velocity box limits, B = 65 536).  N > 1 (config 5): `--scaling weak` (default)
keeps 65 536 instances per GPU, `--scaling strong --global-batch 524288` splits BASELINE's batch
over the ranks; instances are independent, so ranks never exchange data inside the timed region.

    python bench.py --gpus 1 --steps 20 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

The launcher only provides RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*: the process bootstrap is a
TCP rendezvous (pink_amd.comm), the work is libpinkhip.so through ctypes, the gather of dq is
ncclGather through the library's own RCCL binding.

A plain run does only what the headline figure needs: set up, spin up + W warm-up steps, the K timed
steps, the one JSON line (`ms_per_step` = wall milliseconds of one timed step).  `--dump-outputs DIR`
then writes what the last timed step computed -- rank 0's dq, status, iters, path as DIR/<name>.npy
(float64; a fixed seeded sample of the rows if they would exceed 64 MB) -- for output-for-output
comparisons of two builds (the inputs are seeded: identical from run to run).  `--full` adds everything
below (`--headline-only` / `--no-cpu-baseline` then drop parts of it again, as before).

Rank 0 prints ONE JSON line.  Besides the contract fields it carries (from the timed steps themselves)
  roofline        HBM view of the fused kernel (algorithmic bytes / HIP-event time vs 8 TB/s)
  roofline_fp64   fp64-vector view of the same launches (flop model of SURVEY.md 8d from the measured
                  iteration counts vs 78.6 TFLOP/s): the fused kernel is VALU bound, not HBM bound
and a `--full` run adds
  stack_only      the HBM-streaming kernel (build_ik's P, q)
  configs         BASELINE configs 2 (UR5, B = 4096) and 4 (JVRC + 2 barriers, B = 65 536)
  end_to_end      C-ABI call from host buffers (H2D + kernel + D2H), never `value`
  latency_B1_us   config 1 (UR5, batch of one): one solve_ik-sized call
  cpu_baseline    the oracle on the host cores: B0 per-call NumPy, B0' the reference's own build_ik
                  (when PINK_REFERENCE names a checkout of it), B1 C single thread, B2 C all cores
  parity          every instance of rank 0's batch against the C oracle
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X_MICROARCH.md: fp64 vector (= fp64 MFMA) dense peak


def flops_per_qp(batch, iters_mean: float) -> float:
    """Useful-flop model of SURVEY.md 8(d) for the active-set path: stacking of the symmetric half
    Kd nv (nv+1) (+ 2 Kd nv for c), Cholesky nv^3/3, two triangular solves 2 nv^2, then per active-set
    iteration ~4 nv^2 (z = J2 d2 and the update of J) + 2 md nv for the slacks of the dense rows."""
    nv, Kd, md = batch.nv, batch.Kd, batch.md
    return Kd * nv * (nv + 1) + 2 * Kd * nv + nv ** 3 / 3.0 + 2 * nv * nv + iters_mean * (4 * nv * nv + 2 * md * nv)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores() -> int:
    """Threads this process may really use: the affinity mask, capped by a cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    try:  # cgroup v2
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = max(1, min(n, int(q / p + 0.5)))
        except (OSError, ValueError):
            pass
    return n


def _timed(fn, repeats: int, warmup: int = 1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def cpu_baseline(terms, budget_s: float = 20.0):
    """The CPU legs of BASELINE.md section 3 on a bounded sample of the same workload (Pink + quadprog
    cannot run offline: every leg is the restated path of oracle/, labelled so).  Medians over >= 10 repeats."""
    from oracle import c_oracle
    from oracle import pink_oracle as po
    from pink_amd import synthetic

    cores = usable_cores()
    out = {"unit": "solves/s", "kind": "port", "cpu_model": cpu_model(), "logical_cpus": os.cpu_count(),
           "usable_cores": cores,
           "label": "restated CPU baseline (Pink + quadprog unavailable offline): oracle/ stacking as pink/tasks/task.py:145-167 "
                    "+ Goldfarb-Idnani"}
    n_all = terms.B

    def pf_of(n):
        return synthetic.pink_form(terms.slice(0, n))

    def legs(pf, nthreads):
        return lambda: c_oracle.solve_ik_batch(**pf, nthreads=nthreads)

    # B1: C, one thread
    n1 = min(n_all, 512)
    pf1 = pf_of(n1)
    t1 = _timed(legs(pf1, 1), 10)
    b1 = n1 / statistics.median(t1)
    out["B1_c_single_thread"] = {"median": b1, "best": n1 / min(t1), "repeats": len(t1), "sample": n1, "threads": 1}
    # B2: C, OpenMP over the batch; the thread count is swept (a container may expose more logical CPUs than it
    # may use) and the best median is the baseline
    n2 = min(n_all, max(2048, min(32768, int(b1 * cores * 0.1))))
    pf2 = pf_of(n2)
    sweep = {}
    cand = sorted({c for c in (min(cores, 8), min(cores, 32), min(cores, 64), cores // 2, cores) if c >= 1})
    for th in cand:
        ts = _timed(legs(pf2, th), 10 if th == cores else 4)
        sweep[th] = {"median": n2 / statistics.median(ts), "best": n2 / min(ts), "repeats": len(ts)}
    best_th = max(sweep, key=lambda k: sweep[k]["median"])
    b2 = sweep[best_th]["median"]
    out["B2_c_all_cores"] = {"median": b2, "best": sweep[best_th]["best"], "threads": best_th, "sample": n2,
                             "repeats": sweep[best_th]["repeats"],
                             "parallel_efficiency": b2 / (b1 * best_th),
                             "thread_sweep": {str(k): v["median"] for k, v in sweep.items()}}
    # B0: the solve_ik calling pattern -- one QP per call, NumPy stacking + NumPy Goldfarb-Idnani, one core
    n0 = min(n_all, 24)
    pf0 = pf_of(n0)
    rows = pf0["rows"]

    def per_call():
        for b in range(n0):
            tasks = [(pf0["J"][b, rows[t]:rows[t + 1]], pf0["e"][b, rows[t]:rows[t + 1]], pf0["cost"][rows[t]:rows[t + 1]],
                      float(pf0["gain"][t]), float(pf0["lm"][t])) for t in range(len(rows) - 1)]
            P, q = po.qp_objective(terms.nv, tasks, terms.damping)
            if pf0.get("diag_extra") is not None:
                P = P + pf0["diag_extra"][b] * np.eye(terms.nv)
            po.goldfarb_idnani(P, q, pf0["G"][b], pf0["h"][b])

    t0 = _timed(per_call, 10)
    out["B0_numpy_per_call"] = {"median": n0 / statistics.median(t0), "best": n0 / min(t0), "repeats": len(t0), "sample": n0,
                                "threads": 1, "note": "Pinocchio time excluded (J, e given)"}
    # B0': the reference's own build_ik (stacking half only; its QP solve needs quadprog) where the checkout exists
    out["B0prime_reference_build_ik"] = reference_build_ik_rate(terms)
    out.update(value=b2, cores=best_th,
               sample=f"B2: {n2} instances of the same workload, C oracle (stack + Goldfarb-Idnani), OpenMP static over "
                      f"{best_th} threads, median of {sweep[best_th]['repeats']}")
    ref = c_oracle.solve_ik_batch(**pf2, nthreads=best_th)
    return out, ref, n2


def reference_build_ik_rate(terms):
    """pink.build_ik verbatim (pink/solve_ik.py:152-203) on stub pinocchio/qpsolvers, per call -- only where the
    environment variable PINK_REFERENCE names a checkout of the reference (nothing outside the repository is read
    otherwise); the GPU box has none."""
    ref_dir = os.environ.get("PINK_REFERENCE")
    if not ref_dir or not os.path.isdir(os.path.join(ref_dir, "pink")):
        return {"available": False, "reason": "PINK_REFERENCE names no reference checkout on this host (measured where one was: "
                                              "profiles/cpu_baseline_container_r02.json)"}
    try:
        import importlib.util

        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        return mg.time_reference_build_ik(terms, repeats=10)
    except Exception as exc:  # noqa: BLE001  the baseline must never cost the bench line
        return {"available": False, "reason": f"failed: {exc!r}"}


def kernel_ms_of(solver, dev, steps: int, stack: bool = False, repeats: int = 3) -> float:
    """Median over `repeats` of the HIP-event time of `steps` back-to-back launches (auxiliary figures only: the
    headline is timed once, over exactly K steps, in main())."""
    run = solver.stack_device if stack else solver.solve_device
    emulated = bool(getattr(solver, "device_info", None)) and solver.device_info().get("gcn_arch") == "cpu-emulator"
    if stack:
        steps = max(steps, 20)  # (round-5 review: identical stack-only launches read +-25 % from five launches behind a cold clock)
    if emulated:
        steps, repeats = 1, 1  # (the CPU dry runs of tests/test_bench_dryrun.py: control flow, not timing)
    run(dev)
    solver.sync()
    # (these figures follow seconds of oracle work on the host cores: ~25 ms of launches bring the clocks back up first --
    # one 0.3 ms launch does not, and the sub-millisecond kernels read 5-10 % slow without it)
    t0, n = time.perf_counter(), 0
    while not emulated and (n < 3 or (time.perf_counter() - t0 < 0.025 and n < 200)):
        run(dev)
        solver.sync()
        n += 1
    out = []
    for _ in range(repeats):
        solver.timer_start()  # HIP events on the stream the kernel runs on
        for _ in range(steps):
            run(dev)
        out.append(solver.timer_stop() / max(steps, 1))
    return statistics.median(out)


def full_parity(terms, batch, res, n_exact: int = 4) -> dict:
    """SURVEY.md 8(d) parity procedure over EVERY instance of the batch (oracle/parity_report.py: the C oracle on the
    host cores, the checker -- never the thing measured)."""
    from oracle.parity_report import parity_report
    from pink_amd import synthetic

    t0 = time.perf_counter()
    dq_ref = np.full_like(res.dq, np.nan)
    rep = parity_report(lambda lo, hi: synthetic.pink_form(terms.slice(lo, hi)), batch, res.dq, res.status,
                        nthreads=min(usable_cores(), 64), dq_ref_out=dq_ref)
    rep["max_abs_dq_err_vs_oracle"] = rep["max_abs_err"]
    # ... and both against the EXACT minimiser (50-digit KKT solve, oracle/exact_qp.py) where they differ most: what anchors
    # the QP half in the absence of quadprog, and says which fp64 answer is nearer where dq is weakly determined
    try:
        from oracle.exact_qp import anchor_report

        okk = (res.status == 0) & np.isfinite(dq_ref).all(axis=1)
        t1 = time.perf_counter()
        rep["exact_anchor"] = anchor_report(lambda lo, hi: synthetic.pink_form(terms.slice(lo, hi)), terms.damping, res.dq,
                                            np.nan_to_num(dq_ref), n_exact, n_exact, ok=okk)
        rep["exact_anchor"]["seconds"] = time.perf_counter() - t1
    except Exception as exc:  # noqa: BLE001  (mpmath missing on a box: the report says so)
        rep["exact_anchor"] = {"failed": repr(exc)}
    del dq_ref
    # what the tasks see: the weighted rows of the dense tasks, W J (dq - dq_ref), on a sample -- the quantity that stays
    # within the tolerance where dq itself is only weakly determined (flat directions of a weakly regularised H)
    from oracle import c_oracle

    n = min(batch.B, 4096)
    ref = c_oracle.solve_ik_batch(**synthetic.pink_form(terms.slice(0, n)), nthreads=min(usable_cores(), 64))
    okk = (ref["status"] == 0) & (res.status[:n] == 0)
    cost = batch.cost[:n, :batch.Kd] if batch.cost.ndim == 2 else batch.cost[None, :batch.Kd]
    rep["max_abs_weighted_task_row_err_on_sample"] = float(np.abs(np.einsum("bkj,bj->bk", batch.J[:n] * cost[:, :, None], res.dq[:n] - ref["dq"]))[okk].max(initial=0.0))
    rep["task_row_sample"] = n
    rep["tolerance"] = 1e-8
    rep["checker_seconds"] = time.perf_counter() - t0
    rep["note"] = "oracle = restated Goldfarb-Idnani; QP half parity-unpinned against quadprog (DESIGN.md 4)"
    return rep


def solver_paths(res) -> dict:
    """Which code solved the instances of a batch (include/pinkhip.h, PINKHIP_PATH_*): shares per path, and
    `handover_frac` = the share that paid for BOTH solvers (tableau result failed its KKT certificate)."""
    fr = res.path_fractions()
    return {"paths": fr, "handover_frac": fr.get("handover", 0.0), "routed_frac": fr.get("routed", 0.0)}


def measure_config(solver, name: str, B: int, steps: int, seed=None, ab_gi_alone: bool = False, **kw) -> dict:
    """One BASELINE configuration on the resident-batch path: kernel time, both rooflines, stack-only kernel,
    parity of the whole batch against the oracle.  `ab_gi_alone`: also time the Goldfarb-Idnani kernel alone on the same
    resident batch (PINKHIP_SOLVER=packed, read by the library per call) -- what an instance that skips the tableau costs."""
    from pink_amd import synthetic

    terms = synthetic.make_terms(name, B, seed=seed, **kw)
    batch = synthetic.pack(terms)
    dev = solver.upload(batch)
    ms = kernel_ms_of(solver, dev, steps)
    res = solver.download(dev)
    gi_alone = None
    if ab_gi_alone:
        old = os.environ.get("PINKHIP_SOLVER")
        os.environ["PINKHIP_SOLVER"] = "packed"
        try:
            ms_gi = kernel_ms_of(solver, dev, steps)
            r_gi = solver.download(dev)
            gi_alone = {"kernel_ms": ms_gi, "ratio_default_over_gi_alone": ms / ms_gi, "failed": int((r_gi.status != 0).sum()),
                        "max_abs_dq_difference_to_default": float(np.abs(r_gi.dq - res.dq)[(r_gi.status == 0) & (res.status == 0)].max(initial=0.0))}
        finally:
            if old is None:
                del os.environ["PINKHIP_SOLVER"]
            else:
                os.environ["PINKHIP_SOLVER"] = old
        solver.solve_device(dev)  # (leave the default kernel's result in the buffers)
        solver.sync()
    stack_ms = kernel_ms_of(solver, dev, steps, stack=True)
    dev.free()
    parity = full_parity(terms, batch, res)
    it = float(res.iters.mean())
    fl = flops_per_qp(batch, it)
    rate = B / (ms * 1e-3)
    return {
        "workload": f"{name}: nv={batch.nv}, Kd={batch.Kd}, K={batch.K}, md={batch.md}, B={B}, " + ", ".join(f"{k}={v}" for k, v in kw.items()),
        "kernel_ms": ms, "solves_per_s": rate, "bytes_per_qp": batch.bytes_per_qp(),
        "hbm_GBs": batch.bytes_per_qp() * rate / 1e9, "hbm_frac": batch.bytes_per_qp() * rate / 1e9 / HBM_PEAK_GBS,
        "flops_per_qp": fl, "fp64_TFLOPs": fl * rate / 1e12, "fp64_frac": fl * rate / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
        "iters_mean": it, "iters_max": int(res.iters.max()), "failed": int((res.status != 0).sum()),
        "solver_stats": solver_paths(res), "goldfarb_idnani_kernel_alone": gi_alone,
        "stack_only": {"kernel_ms": stack_ms, "bytes_per_qp": batch.bytes_per_stack(),
                       "achieved_GBs": batch.bytes_per_stack() * B / (stack_ms * 1e-3) / 1e9,
                       "frac": batch.bytes_per_stack() * B / (stack_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
        "parity": parity,
    }


def api_level(solver, B: int = 4096, Bh: int = 65536) -> dict:
    """`pink_amd.solve_ik_batch(configurations, tasks, dt)` -- the Python API of the drop-in -- on B configurations
    of a 6-dof arm: with the kinematics evaluated by the device kernels from q (default for B >= 64) and with
    tasks / limits evaluated per configuration on the host as Pink does (on a 256-configuration sample)."""
    import pink_amd
    from pink_amd import Configuration, FrameTask, PostureTask, build_chain, solve_ik_batch
    from pink_amd.lie import SE3
    from pink_amd.runtime import set_default_solver

    set_default_solver(solver)
    try:
        m = build_chain(6)
        rng = np.random.default_rng(2)
        cfgs, tasks = [], []
        for _ in range(B):
            q = m.neutral()
            for j in m.joints:
                q[j.idx_q] = rng.uniform(-0.9, 0.9)
            cfg = Configuration(m, q)
            t = FrameTask("tool0", 1.0, 1.0, lm_damping=1.0)
            t.set_target(cfg.get_transform_frame_to_world("tool0") * SE3(np.eye(3), 0.05 * rng.normal(size=3)))
            p = PostureTask(cost=1e-3)
            p.set_target(m.neutral())
            cfgs.append(cfg)
            tasks.append([t, p])
        dt = 1.0 / 200.0
        v_dev = solve_ik_batch(cfgs, tasks, dt)
        t_dev = statistics.median(_timed(lambda: solve_ik_batch(cfgs, tasks, dt), 3))
        v_host = solve_ik_batch(cfgs, tasks, dt, device_kinematics=False)
        t_host = statistics.median(_timed(lambda: solve_ik_batch(cfgs, tasks, dt, device_kinematics=False), 3, warmup=0))
        out = {"workload": f"6-dof arm, FrameTask + PostureTask, {B} configurations, pink_amd {pink_amd.__version__}",
               "device_kinematics": {"ms": t_dev * 1e3, "solves_per_s": B / t_dev},
               "host_evaluated_tasks_list_of_configurations": {
                   "what": "the same list of Configuration objects and per-instance task objects with device_kinematics=False: tasks, "
                           "limits evaluated on the host for the whole batch at once (pink_amd/batch_eval.py over one vectorised "
                           "forward kinematics), QP on the device; what is left per instance is reading q and the target out of the "
                           "Python objects",
                   "ms": t_host * 1e3, "instances": B, "solves_per_s": B / t_host},
               "max_abs_velocity_difference": float(np.abs(v_dev - v_host).max())}
        out["host_evaluated_tasks"] = api_level_host_evaluated(m, B)
        out["headline_shape_arrays"] = api_level_arrays(Bh)
        if hasattr(solver, "pinned_empty"):
            out["headline_shape_arrays_page_locked"] = api_level_arrays(Bh, pinned=True)
            out["headline_shape_arrays_page_locked_frozen_targets"] = api_level_arrays(Bh, pinned=True, freeze=True)
            out["headline_shape_arrays_page_locked_quaternion_targets"] = api_level_arrays(Bh, pinned=True, quat=True)
        # the task stack of the reference's own humanoid example (examples/humanoid_draco3.py:34-71: FrameTasks, a
        # PostureTask, two JointCouplingTasks) and one with a DampingTask: formed on chip by the whole-step kernel from
        # constant tables; beside them the same calls with only the FrameTask rows formed on the device
        # (pink_amd/hybrid.py: the route of stacks the kernel does not form) and with everything evaluated on the host
        out["reference_example_stack"] = api_level_arrays(Bh, extra_task="couplings")
        out["headline_shape_plus_damping_task"] = api_level_arrays(Bh, extra_task="damping")
        # round 5: build_ik's remaining arguments on the whole-step kernel -- constraints=[FrameTask] (its leading equality
        # rows) and a BodySphericalBarrier next to a PositionBarrier (rows formed on chip); round 4: hybrid / host routes
        out["headline_shape_plus_equality_constraint"] = api_level_arrays(Bh, extra_task="constraint")
        out["headline_shape_plus_spherical_and_position_barrier"] = api_level_arrays(Bh, extra_task="barriers")
        out["headline_shape_plus_damping_task_frame_rows_only"] = api_level_arrays(Bh, extra_task="damping", route="frame_rows")
        out["headline_shape_plus_damping_task_all_host"] = api_level_arrays(Bh, extra_task="damping", route=False)
        return out
    finally:
        pink_amd.clear_device_cache()
        set_default_solver(None)


def api_level_host_evaluated(m, B: int) -> dict:
    """`solve_ik_batch(ConfigurationBatch, tasks, dt)` for the stack round 3's verdict measured at 17.5 k solves/s --
    FrameTask + PostureTask + DampingTask + a JointCouplingTask, under ConfigurationLimit + VelocityLimit +
    AccelerationLimit passed explicitly.  Since the end of round 4 the whole-step kernel forms all of it (route `device`);
    `all_evaluated_on_the_host` is the same call on the host-evaluated route: every task / limit evaluated for the whole
    batch by pink_amd/batch_eval.py (vectorised NumPy over one batched forward kinematics), the QP by the stack + solve
    kernel."""
    import pink_amd
    from pink_amd import Configuration, ConfigurationBatch, DampingTask, FrameTask, PostureTask, solve_ik, solve_ik_batch
    from pink_amd.lie import SE3
    from pink_amd.limits import AccelerationLimit, ConfigurationLimit, VelocityLimit
    from pink_amd.tasks import JointCouplingTask

    rng = np.random.default_rng(5)
    q = np.tile(m.neutral(), (B, 1))
    for j in m.joints:
        q[:, j.idx_q] = rng.uniform(-0.9, 0.9, size=B)
    cfgs = ConfigurationBatch(m, q)
    ref = Configuration(m, q[0])
    ft = FrameTask("tool0", 1.0, 1.0, lm_damping=1.0)
    T0 = ref.get_transform_frame_to_world("tool0")
    ft.set_target_poses(np.broadcast_to(T0.rotation, (B, 3, 3)), T0.translation + 0.05 * rng.normal(size=(B, 3)))
    po = PostureTask(cost=1e-3)
    po.set_target(m.neutral())
    tasks = [ft, po, DampingTask(cost=1e-2), JointCouplingTask(["joint_2", "joint_3"], [1.0, -1.0], 0.5, ref)]
    acc = AccelerationLimit(m, np.full(m.nv, 50.0))
    limits = [ConfigurationLimit(m), VelocityLimit(m), acc]
    dt = 1.0 / 200.0
    v = solve_ik_batch(cfgs, tasks, dt, limits=limits)
    stats = pink_amd.last_solve_stats()
    ts = _timed(lambda: solve_ik_batch(cfgs, tasks, dt, limits=limits), 5)
    t_call = statistics.median(ts)
    # (since the whole-step kernel forms couplings, identity tasks and the acceleration limit, this stack takes the device
    # route by itself; the same call with every task / limit evaluated on the host for the whole batch beside it)
    v_h = solve_ik_batch(cfgs, tasks, dt, limits=limits, device_kinematics=False, gpu_frame_tasks=False)
    ts_h = _timed(lambda: solve_ik_batch(cfgs, tasks, dt, limits=limits, device_kinematics=False, gpu_frame_tasks=False), 5)
    n = 8  # cross-check: Pink's own calling pattern, one solve_ik per configuration
    v_ref = []
    for b in range(n):
        fb = FrameTask("tool0", 1.0, 1.0, lm_damping=1.0)
        fb.set_target(SE3(ft.target_poses[b, :9].reshape(3, 3), ft.target_poses[b, 9:]))
        v_ref.append(solve_ik(Configuration(m, q[b]), [fb, po, tasks[2], tasks[3]], dt, limits=limits))
    return {"workload": f"6-dof arm, FrameTask + PostureTask + DampingTask + JointCouplingTask, ConfigurationLimit + VelocityLimit + "
                        f"AccelerationLimit, B = {B} as ConfigurationBatch, targets as arrays",
            "route": stats.get("route"), "ms_per_call": t_call * 1e3, "ms_per_call_best": min(ts) * 1e3, "solves_per_s": B / t_call,
            "max_abs_velocity_difference_vs_per_configuration_solve_ik_on_sample": float(np.abs(v[:n] - np.array(v_ref)).max()), "sample": n,
            "all_evaluated_on_the_host": {"route": "host-evaluated", "ms_per_call": statistics.median(ts_h) * 1e3, "ms_per_call_best": min(ts_h) * 1e3,
                                          "solves_per_s": B / statistics.median(ts_h),
                                          "max_abs_velocity_difference_vs_the_device_route": float(np.abs(v - v_h).max())}}


def api_level_arrays(B: int, extra_task: str = "", pinned: bool = False, route=None, freeze: bool = False, quat: bool = False) -> dict:
    """`pink_amd.solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)` at the HEADLINE shape: a floating-base robot
    with nv = 30 (free flyer + 24 joints), 4 FrameTasks + PostureTask under the model's limits, B configurations as one
    array and per-instance targets as arrays -- q and targets go in, velocities come out, per call (H2D, the
    whole-step kernel, D2H and all Python included)."""
    from pink_amd import Configuration, ConfigurationBatch, FrameTask, PostureTask, build_chain, solve_ik_batch
    from pink_amd.lie import SE3

    import pink_amd

    m = build_chain(24, free_flyer=True, seed=2)
    frames = ["tool0", "joint_8", "joint_16", "joint_20"]
    rng = np.random.default_rng(1)
    # pinned: q, the per-frame target arrays and the output live in page-locked memory (pink_amd.pinned_empty), the way a
    # control loop that refills them in place would hold them
    alloc = pink_amd.pinned_empty if pinned else (lambda shape: np.empty(shape))
    q = alloc((B, m.nq))
    q[:] = m.neutral()
    for j in m.joints:
        if j.kind != "free_flyer":
            q[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
    tasks = []
    ref = Configuration(m, q[0])
    for k, f in enumerate(frames):
        t = FrameTask(f, 1.0, 1.0 if k == 0 else 0.0, lm_damping=1e-3)
        T0 = ref.get_transform_frame_to_world(f)
        # every robot's target: the reference robot's frame pose displaced by a few centimetres
        if quat:  # FrameTask.set_target_poses_quat: translation + quaternion, 7 numbers per target instead of 12
            from scipy.spatial.transform import Rotation

            t.set_target_poses_quat(T0.translation + 0.05 * rng.normal(size=(B, 3)), np.broadcast_to(Rotation.from_matrix(T0.rotation).as_quat(), (B, 4)),
                                    out=alloc((B, 7)))
        else:
            t.set_target_poses(np.broadcast_to(T0.rotation, (B, 3, 3)), T0.translation + 0.05 * rng.normal(size=(B, 3)), out=alloc((B, 12)))
        if freeze:  # FrameTask.freeze_targets: the target arrays go up once per device state, not with every call
            t.freeze_targets()
        tasks.append(t)
    post = PostureTask(cost=1e-1)
    post.set_target(m.neutral())
    tasks.append(post)
    if extra_task == "damping":
        from pink_amd import DampingTask

        tasks.append(DampingTask(cost=1e-2))
    elif extra_task == "couplings":  # (humanoid_draco3.py:57-70: two knee couplings, cost 100, lm_damping 5e-7)
        from pink_amd.tasks import JointCouplingTask

        tasks.append(JointCouplingTask(["joint_3", "joint_4"], [1.0, -1.0], 100.0, ref, lm_damping=5e-7))
        tasks.append(JointCouplingTask(["joint_9", "joint_10"], [1.0, -1.0], 100.0, ref, lm_damping=5e-7))
    cfgs = ConfigurationBatch(m, q)
    dt = 5e-3
    v_out = alloc((B, m.nv)) if pinned else None
    all_host = route is False
    route_kw = {} if route is None else dict(device_kinematics=route)  # (False: every task evaluated on the host, for comparison)
    if extra_task == "constraint":  # pink/solve_ik.py:125-149: one frame held strictly where it is (six equality rows)
        hold = FrameTask("joint_12", 1.0, 1.0, gain=0.5)
        Th = ref.get_transform_frame_to_world("joint_12")
        hold.set_target(Th)
        q[:] = q[0]  # (every robot at the reference configuration: the constraint is within reach of one step everywhere)
        route_kw["constraints"] = [hold]
    elif extra_task == "barriers":
        from pink_amd.barriers import BodySphericalBarrier, PositionBarrier

        p_tool = ref.get_transform_frame_to_world("tool0").translation
        d = float(np.linalg.norm(p_tool - ref.get_transform_frame_to_world("joint_4").translation))
        q[:] = q[0]
        route_kw["barriers"] = [BodySphericalBarrier(("tool0", "joint_4"), d_min=0.98 * d, gain=10.0),
                                PositionBarrier("tool0", indices=[2], p_max=np.array([p_tool[2] + 0.01]), gain=np.array([50.0]), safe_displacement_gain=1.0)]
    v = solve_ik_batch(cfgs, tasks, dt, out=v_out, **route_kw)  # builds the device state
    stats = pink_amd.last_solve_stats()
    ts = _timed(lambda: solve_ik_batch(cfgs, tasks, dt, out=v_out, **route_kw), 5 if not all_host else 2)
    t_call = statistics.median(ts)
    n = min(B, 16)
    host_kw = {k: v_ for k, v_ in route_kw.items() if k != "device_kinematics"}
    v_host = solve_ik_batch(cfgs[:n], [_slice_task(t, n) for t in tasks], dt, device_kinematics=False, gpu_frame_tasks=False, **host_kw)
    return {"workload": f"floating base + 24 joints (nv = {m.nv}), {len(frames)} FrameTasks + PostureTask" +
                        {"": "", "damping": " + DampingTask", "couplings": " + 2 JointCouplingTasks", "constraint": " + constraints=[FrameTask]",
                         "barriers": " + BodySphericalBarrier + PositionBarrier"}[extra_task] +
                        f", default limits, B = {B} as ConfigurationBatch, targets as arrays",
            "route": stats.get("route"), "solver_paths": stats.get("paths"),
            "ms_per_call": t_call * 1e3, "ms_per_call_best": min(ts) * 1e3, "solves_per_s": B / t_call,
            "bytes_in_per_call": int(q.nbytes + (0 if freeze else B * len(frames) * (7 if quat else 12) * 8)), "bytes_out_per_call": int(B * m.nv * 8 + 8 * B),
            "targets": "frozen (FrameTask.freeze_targets: resident on the device)" if freeze else
                       ("translation + quaternion (FrameTask.set_target_poses_quat), uploaded with every call" if quat else "uploaded with every call"),
            "max_abs_velocity_difference_vs_host_evaluated_tasks_on_sample": float(np.abs(v[:n] - v_host).max()), "sample": n}


def _slice_task(task, n):
    """The first n per-instance targets of a task carrying batched targets (for the host-evaluated cross-check)."""
    import copy

    t = copy.copy(task)
    if getattr(t, "target_poses", None) is not None:
        t.target_poses = t.target_poses[:n]
    if getattr(t, "target_pq", None) is not None:
        t.target_pq = t.target_pq[:n]
    if getattr(t, "target_q_batch", None) is not None:
        t.target_q_batch = t.target_q_batch[:n]
    return t


def closed_loop_figures(solver, B: int, only=None) -> dict:
    """Device-resident closed loop (pink_amd.rollout.DeviceRollout, the whole control step in one kernel): B robots,
    HIP-event time per step.  Headline shape (nv = 30, 4 FrameTasks + posture) and BASELINE config 4's shape (nv = 50,
    4 FrameTasks + posture + 2 PositionBarriers = 6 barrier rows formed on chip)."""
    from pink_amd import Configuration, build_chain
    from pink_amd.barriers import PositionBarrier
    from pink_amd.rollout import DeviceRollout

    out = {}
    for label, model, frames, nbar in (("nv30_4frames_posture", build_chain(24, free_flyer=True, seed=2), ["tool0", "joint_8", "joint_16", "joint_20"], 0),
                                       ("nv30_4frames_posture_2barriers", build_chain(24, free_flyer=True, seed=2), ["tool0", "joint_8", "joint_16", "joint_20"], 2),
                                       ("jvrc_shape_nv50_4frames_posture_2barriers", build_chain(44, free_flyer=True, seed=4), ["tool0", "joint_10", "joint_20", "joint_30"], 2)):
        if only and only not in label:
            continue
        rng = np.random.default_rng(1)
        q0 = np.tile(model.neutral(), (B, 1))
        for j in model.joints:
            if j.kind != "free_flyer":
                q0[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
        specs = [(f, 1.0, 1.0 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
        bars = []
        for f in frames[:nbar]:
            p = np.array([Configuration(model, q0[b]).get_transform_frame_to_world(f).translation for b in range(min(B, 64))])
            bars.append(PositionBarrier(f, p_min=p.min(axis=0) - 0.02, gain=np.array([100.0] * 3), safe_displacement_gain=1.0))
        ro = DeviceRollout(solver, model, q0, specs, 5e-3, posture_cost=1e-1, fused="kernel", position_barriers=bars)
        try:
            ro.step()
            solver.sync()
            T = ro.frame_poses()
            T[:, :, 9:12] += 0.05 * rng.normal(size=(B, len(frames), 3))
            ro.set_targets(T)
            ro.run(5)
            steps = 30
            solver.timer_start()
            for _ in range(steps):
                ro.step()
            ms = solver.timer_stop() / steps
            _, st, it = ro.last_step()
            n_path = np.bincount(ro.last_path.astype(np.int64), minlength=4)
            out[label] = {"nv": model.nv, "B": B, "ms_per_step": ms, "robot_steps_per_s": B / (ms * 1e-3), "launches_per_step": 1 if ro.fused == "kernel" else 2,
                          "barrier_rows": ro.md, "qp_iters_mean": float(it.mean()), "failed": int((st != 0).sum()),
                          "handover_frac": float(n_path[1]) / B, "routed_frac": float(n_path[2]) / B}
            # what a target change costs: every robot's targets move by a few centimetres at once (the steady state above
            # is a converged loop: < 1 active-set step per QP); the first steps afterwards, one HIP-event bracket each
            T[:, :, 9:12] += 0.05 * rng.normal(size=(B, len(frames), 3))
            ro.set_targets(T)
            solver.sync()
            after = []
            for _ in range(4):
                solver.timer_start()
                ro.step()
                t_ms = solver.timer_stop()
                after.append({"ms": t_ms, "qp_iters_mean": float(ro.last_step()[2].mean())})
            out[label]["steps_after_a_target_move"] = after
        finally:
            ro.free()
    return out


def _matching_traffic_file():
    """(`profiles/traffic_rNN.json` record, its name) of the newest committed PMC pass that was collected on exactly these
    kernel sources (content hash), or (None, reason)."""
    import glob

    import __graft_entry__ as g

    want = g._source_hash(g.HIP_DEPS)
    newest = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "traffic_r*.json")), reverse=True):
        try:
            t = json.load(open(path))
        except (OSError, ValueError):
            continue
        newest = newest or os.path.basename(path)
        if t.get("source_hash") == want:
            return t, os.path.basename(path)
    return None, (f"profiles/{newest} is from other kernel sources: not reported" if newest else "no PMC pass committed for these sources")


def traffic_from_profiles():
    """HBM bytes per launch of the fused kernel from the committed rocprofv3 PMC pass -- reported only when that
    pass was collected on exactly these kernel sources (content hash), else null."""
    t, name = _matching_traffic_file()
    if t is None:
        return None, name
    return t.get("solve_kernel_hbm_bytes_per_launch"), f"profiles/{name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, same kernel sources {t['source_hash'][:12]})"


def _valu_issue(kernel_ms: float, n_cu: int):
    """VALU-issue roofline of the solve kernel: wavefront-level VALU instructions per launch (SQ_INSTS_VALU of the
    committed counter pass, same kernel sources) over the live launch duration, against the issue rate of the SIMDs --
    n_cu x 4 SIMDs, one wave64 VALU instruction per 4 cycles (16 lanes per SIMD; fp64 FMA has the full rate on
    MI355X), at the 2.4 GHz peak engine clock (MI355X_MICROARCH.md)."""
    t, name = _matching_traffic_file()
    if t is None or "solve_kernel_valu_instructions_per_launch" not in t:
        return None
    insts = t["solve_kernel_valu_instructions_per_launch"]
    peak = n_cu * 4 * 2.4e9 / 4 / 1e9
    achieved = insts / (kernel_ms * 1e-3) / 1e9
    return {"bound": "valu issue", "achieved": achieved, "peak": peak, "unit": "G wave64 VALU instructions/s", "frac": achieved / peak,
            "valu_instructions_per_launch": insts, "fma_f64_share": t.get("solve_kernel_fma_f64_instructions_per_launch", 0.0) / insts,
            "source": f"SQ_INSTS_VALU of profiles/{name.replace('traffic', 'sq_counters').replace('.json', '.txt')} (rocprofv3 --pmc, same kernel sources) / kernel_ms measured here"}


def _with_timeout(fn, seconds: float, what: str):
    """`fn()` on a daemon thread; TimeoutError if it is not back after `seconds` (collectives that never return must
    not cost the bench line; the caller then leaves the process through os._exit)."""
    import threading

    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as exc:  # noqa: BLE001
            box["error"] = exc

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(seconds)
    if t.is_alive():
        raise TimeoutError(f"{what} did not return within {seconds:.0f} s")
    if "error" in box:
        raise box["error"]
    return box.get("value")


def _device_count() -> int:
    import ctypes

    from pink_amd import _lib

    n = ctypes.c_int(0)
    _lib.load_library().pinkhip_device_count(ctypes.byref(n))
    return n.value


def self_launch(n: int) -> int:
    """``python bench.py --gpus N`` with no launcher around it (WORLD_SIZE unset): start the N ranks from here, one
    process per GPU, rendezvous on a free port of 127.0.0.1; rank 0 prints the one JSON line to the inherited stdout.
    Returns the exit code of the job (non-zero as soon as a rank fails; the other ranks are then stopped)."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = list(sys.orig_argv) if getattr(sys, "orig_argv", None) else [sys.executable] + sys.argv
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, env=env, stdout=_RESULT_FD))  # (the ranks inherit the original stdout)
    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is not None:
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr)
                    deadline = time.time() + 10.0
                    while time.time() < deadline and any(procs[q].poll() is None for q in pending):
                        time.sleep(0.2)
                    for q in pending:
                        if procs[q].poll() is None:
                            procs[q].kill()  # exactly the processes started above
        time.sleep(0.05)
    return rc


# keys of the ONE stdout line (the driver keeps a bounded tail of stdout and parses the last line: round 4's line had
# grown to 22.6 KB and did not parse).  Everything else goes to the detail file + stderr.
_HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data")
_HEADLINE_LIMIT = 4096


def _finite(x):
    """NaN / inf have no JSON spelling: None in the emitted objects (json.dumps(allow_nan=False) then holds)."""
    if isinstance(x, float):
        return x if math.isfinite(x) else None
    if isinstance(x, dict):
        return {str(k): _finite(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite(v) for v in x]
    if isinstance(x, np.generic):
        return _finite(x.item())
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def headline_of(line: dict, detail_path) -> dict:
    """The bounded stdout line: BASELINE.json's metric, the workload, the roofline of the dominant kernel, the CPU
    baseline and the whole-batch parity figures -- and a pointer to the detail file."""
    cfg = dict(_pick(line["config"], ("workload", "batch_per_gpu", "global_batch", "nv", "Kd", "K", "md", "parallelism")),
               solver="principal pivoting from a guessed active set on a register-resident sweep tableau, fp64, KKT-certified; GI fallback")
    out = _pick(line, _HEADLINE_KEYS)
    out["config"] = cfg
    out["roofline"] = _pick(line["roofline"], ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "bytes_per_qp",
                                               "bound_actual", "bound_actual_frac"))
    if "cpu_baseline" in line:
        out["cpu_baseline"] = _pick(line["cpu_baseline"], ("value", "unit", "cores", "kind", "cpu_model", "sample"))
        out["cpu_baseline"]["label"] = line["cpu_baseline"].get("label", "")[:100]
    if "parity" in line:
        out["parity"] = _pick(line["parity"], ("instances_compared", "max_abs_err", "status_mismatch", "active_set_equal_frac", "tolerance"))
        out["parity"]["note"] = line["parity"].get("note", "")[:110]
        ex = line["parity"].get("exact_anchor") or {}
        if "max_abs_err_vs_exact" in ex:  # 50-digit minimiser on a sample (oracle/exact_qp.py)
            out["parity"]["exact"] = _pick(ex, ("instances", "max_abs_err_vs_exact", "oracle_max_abs_err_vs_exact"))
    if line.get("n_gpus", 1) > 1:
        out["per_rank_kernel_ms"] = line.get("per_rank_kernel_ms")
        g = line.get("gather") or {}
        out["gather"] = _pick(g, ("ms", "bytes_per_rank", "rank0_shard_intact", "failed"))
        out["gather"]["transport"] = str(g.get("transport", ""))[:48]
        out["comm_note"] = None if line.get("comm_note") is None else str(line["comm_note"])[:220]
    # the other bounds of the same launches and the regime a control loop runs in (kernel time only), one number each
    also = {"fp64_frac": (line.get("roofline_fp64") or {}).get("frac"), "valu_issue_frac": (line.get("roofline_valu_issue") or {}).get("frac"),
            "stack_only_hbm_frac": (line.get("stack_only") or {}).get("frac"),
            "tracking_regime_kernel_ms": ((line.get("other_regimes") or {}).get("tracking_small_errors") or {}).get("kernel_ms"),
            "failed": (line.get("solver_stats") or {}).get("failed")}
    out["also"] = {k: v for k, v in also.items() if v is not None}
    out["detail"] = detail_path
    return out


def _headline_and_detail(line: dict) -> str:
    """Writes the full record to the detail file (+ stderr) and returns the bounded stdout line."""
    line = _finite(line)
    path = os.environ.get("PINK_BENCH_DETAIL", os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    full = json.dumps(line, allow_nan=False)
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(full + "\n")
        shown = os.path.relpath(path, ROOT) if path.startswith(ROOT + os.sep) else path
    except OSError as exc:  # a read-only checkout: the detail still goes to stderr
        shown = f"stderr only ({exc.__class__.__name__})"
    print("bench detail: " + full, file=sys.stderr, flush=True)
    head = headline_of(line, shown)
    text = json.dumps(head, allow_nan=False)
    if len(text) > _HEADLINE_LIMIT:  # never again an unparseable line: drop the free-text fields first
        head["config"]["solver"] = head["config"]["solver"][:40]
        head["config"]["workload"] = head["config"]["workload"][:120]
        for k in ("cpu_baseline", "parity"):
            if k in head:
                head[k].pop("label", None), head[k].pop("note", None), head[k].pop("sample", None)
        text = json.dumps(head, allow_nan=False)
    assert len(text) <= _HEADLINE_LIMIT, len(text)
    return text



_RESULT_FD = None


def _keep_stdout_for_the_result() -> None:
    """The contract is ONE JSON line on stdout.  Libraries loaded into the process print there too (RCCL's version
    banner when the first communicator is created, flushed when the process exits): file descriptor 1 is pointed at
    stderr for everything else and the result goes to a duplicate of the original."""
    global _RESULT_FD
    if _RESULT_FD is None:
        sys.stdout.flush()
        _RESULT_FD = os.dup(1)
        os.dup2(2, 1)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, res) -> None:
    """What the timed path hands its caller (BatchResult: dq, status, iters, path) as out_dir/<name>.npy, float64.
    Above DUMP_LIMIT_BYTES in all, a fixed seeded sample of the instances is written instead (`rows`: their indices)."""
    arrays = {"dq": res.dq, "status": res.status, "iters": res.iters}
    if res.path is not None:
        arrays["path"] = res.path
    B = res.dq.shape[0]
    per_row = sum(8 * (a.size // max(B, 1)) for a in arrays.values())
    if per_row * B > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(B, DUMP_LIMIT_BYTES // (per_row + 8), replace=False))
        arrays = dict({k: a[rows] for k, a in arrays.items()}, rows=rows)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def _emit(text: str) -> None:
    data = (text + "\n").encode()
    if _RESULT_FD is None:
        sys.stdout.write(text + "\n")
        sys.stdout.flush()
        return
    while data:
        data = data[os.write(_RESULT_FD, data):]


def main() -> None:
    _keep_stdout_for_the_result()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="draco3", choices=["ur5", "draco3", "draco3_freeflyer", "draco3b", "jvrc", "jvrc_noposture"])
    ap.add_argument("--batch", type=int, default=65536, help="instances per GPU (weak scaling)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--global-batch", type=int, default=524288, help="total instances, split over the ranks (strong scaling)")
    ap.add_argument("--bounds", default="tight", choices=["tight", "kinematic"])
    ap.add_argument("--jacobians", default="dense", choices=["dense", "kinematic"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="with --full: only the timed headline (profiling runs)")
    ap.add_argument("--full", action="store_true", help="every figure besides the headline (configs, regimes, end-to-end, latency, "
                                                        "closed loop, API level, CPU baseline, whole-batch parity)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy")
    args = ap.parse_args()
    if not args.full:  # a plain run: the headline figure and nothing else
        args.headline_only = args.no_cpu_baseline = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: this process becomes the launcher of N ranks (one per GPU) instead of silently running one
        have = _device_count()
        if have < args.gpus and os.environ.get("PINKHIP_ALLOW_SHARED_DEVICE") != "1":
            raise SystemExit(f"--gpus {args.gpus} but {have} device(s) visible (PINKHIP_ALLOW_SHARED_DEVICE=1 lets ranks share one)")
        raise SystemExit(self_launch(args.gpus))

    from pink_amd.comm import HostComm, HostRendezvous, RcclComm

    rdzv = HostRendezvous.from_env()
    rank, world = rdzv.rank, rdzv.world
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: one rank per GPU")

    import __graft_entry__ as g
    from pink_amd import batch_solver, synthetic
    from pink_amd.sharding import shard_bounds

    # the library travels prebuilt; if it is stale only rank 0 rebuilds it (hipcc), the others wait
    if rank == 0 and "PINKHIP_LIBRARY" not in os.environ:  # (a development library is used as it is)
        g.build_hip()
    rdzv.barrier()
    if args.scaling == "strong":
        lo, hi = shard_bounds(args.global_batch, rank, world)
        B = hi - lo
        global_batch = args.global_batch
    else:
        B = args.batch
        global_batch = world * B
    # every rank draws its own shard of the global batch (seeded by rank)
    seed = synthetic.SEED0 + synthetic.CONFIGS[args.config]["config_id"] + 1000 * rank
    terms = synthetic.make_terms(args.config, B, bounds=args.bounds, jacobians=args.jacobians, seed=seed)
    batch = synthetic.pack(terms)
    nv = batch.nv

    solver = batch_solver.BatchSolver(device_id=local_rank % max(int(os.environ.get("PINKHIP_VISIBLE_DEVICES", "0")) or _device_count(), 1))
    info = solver.device_info()
    comm, comm_note = None, None
    dev = solver.upload(batch)

    def barrier():
        rdzv.barrier()
        solver.sync()

    # device spin-up (untimed, before the W warm-up steps): a GPU that idled through the host-side setup starts at
    # its idle clocks; ~0.2 s of the same kernel brings it to the sustained state a production loop runs in
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.2:
        for _ in range(8):
            solver.solve_device(dev)
        solver.sync()
    for _ in range(args.warmup):
        solver.solve_device(dev)
    barrier()
    t0 = time.perf_counter()
    solver.timer_start()  # HIP events on the stream the kernel runs on
    for _ in range(args.steps):
        solver.solve_device(dev)
    kernel_ms = solver.timer_stop() / max(args.steps, 1)
    barrier()
    elapsed = rdzv.allreduce_max(time.perf_counter() - t0)

    res = solver.download(dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res)
    # what a host-fed job sees per rank: H2D + kernel + D2H through pinkhip_solve_host from pageable buffers, all ranks
    # at once (they share the host's PCIe / memory bandwidth: SURVEY.md 8(e) "report kernel-only and end-to-end")
    e2e_ranks = None
    if not args.headline_only:
        barrier()
        e2e_ms = statistics.median(_timed(lambda: solver.solve(batch), 3)) * 1e3
        e2e_ranks = [float(np.frombuffer(b, dtype=np.float64)[0]) for b in rdzv.allgather_bytes(np.float64(e2e_ms).tobytes())]
    n_bad = int(rdzv.allreduce_sum(float((res.status != 0).sum())))
    kernel_ms_ranks = [float(np.frombuffer(b, dtype=np.float64)[0]) for b in rdzv.allgather_bytes(np.float64(kernel_ms).tobytes())]

    # the only inter-GPU traffic of the workload: gather of dq to rank 0 (untimed leg of the job, after the timed
    # region: nothing that happens here can cost the throughput figure).  The communicator is created collectively;
    # if RCCL refuses it (e.g. two ranks placed on one device) every rank gets the error, if it does not come back
    # within a minute every rank's watchdog fires, and the job gathers over the rendezvous sockets instead.
    gather = None
    abandoned = False  # a watchdog fired: a thread may still sit in a collective -> leave through os._exit
    if world > 1:
        comm = HostComm(rdzv)
        shared = world > max(_device_count(), 1)  # (PINKHIP_ALLOW_SHARED_DEVICE=1: several ranks on one device)
        if shared:
            comm_note = ("ranks share a device (RCCL refuses duplicate devices in one communicator): dq gathered over the TCP "
                         "rendezvous; no N > 1 RCCL run exists on this pool (1-GPU boxes)")
        if hasattr(solver, "comm_unique_id") and not shared:
            try:
                barrier()
                comm = _with_timeout(lambda: RcclComm(solver, rdzv), 60.0, "RCCL communicator")
            except TimeoutError as exc:
                abandoned = True
                comm_note = f"{exc}; dq gathered over the TCP rendezvous instead"
            except Exception as exc:  # noqa: BLE001
                comm_note = f"RCCL communicator unavailable ({exc}); dq gathered over the TCP rendezvous instead"
        try:
            if not abandoned:
                barrier()
            tg = time.perf_counter()
            if isinstance(comm, RcclComm):
                def rccl_gather():
                    d = comm.gather_device(dev.d_dq, 8 * B * nv, 0)
                    solver.sync()
                    return d

                d_recv = _with_timeout(rccl_gather, 60.0, "ncclGather")
                gather_ms = (time.perf_counter() - tg) * 1e3
                ok = None
                if rank == 0:  # rank 0's own shard must come back unchanged
                    back = np.zeros((B, nv))
                    solver.get(back, d_recv)
                    ok = bool(np.array_equal(back, res.dq))
                    solver.release(d_recv)
                gather = {"ms": gather_ms, "bytes_per_rank": 8 * B * nv, "transport": "ncclGather (RCCL over xGMI) via pinkhip_comm_gather_bytes",
                          "rank0_shard_intact": ok}
            elif abandoned:
                gather = {"failed": comm_note}
            else:
                parts = comm.gather_arrays([res.dq], 0)
                gather = {"ms": (time.perf_counter() - tg) * 1e3, "bytes_per_rank": 8 * B * nv, "transport": "host TCP (no device)",
                          "rank0_shard_intact": None if parts is None else bool(np.array_equal(parts[0][0].reshape(B, nv), res.dq))}
        except TimeoutError as exc:
            abandoned = True
            gather = {"failed": repr(exc)}
        except Exception as exc:  # noqa: BLE001  report, never lose the bench line
            gather = {"failed": repr(exc)}

    if rank == 0:
        extra = {}
        if not args.headline_only:
            # stack-only kernel: the HBM-streaming half (build_ik equivalent), same batch
            stack_ms = kernel_ms_of(solver, dev, max(args.steps, 1), stack=True)
            extra["stack_only"] = {
                "kernel": "ik_stack_mfma_kernel", "kernel_ms": stack_ms, "bytes_per_qp": batch.bytes_per_stack(),
                "achieved": batch.bytes_per_stack() * B / (stack_ms * 1e-3) / 1e9, "unit": "GB/s",
                "frac": batch.bytes_per_stack() * B / (stack_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            }
            # other input regimes of the same config, kernel time only (HIP events)
            regimes = {}
            for label, kw in (("kinematic_bounds", dict(bounds="kinematic", jacobians="kinematic")),
                              ("tracking_small_errors", dict(bounds="kinematic", jacobians="kinematic", error_scale=0.02))):
                t2 = synthetic.make_terms(args.config, B, seed=seed + 7, **kw)
                d2 = solver.upload(synthetic.pack(t2))
                ms2 = kernel_ms_of(solver, d2, 5)
                r2 = solver.download(d2)
                b2 = synthetic.pack(t2)
                regimes[label] = {"kernel_ms": ms2, "solves_per_s": B / (ms2 * 1e-3), "iters_mean": float(r2.iters.mean()),
                                  "failed": int((r2.status != 0).sum()), "solver_stats": solver_paths(r2),
                                  "parity": None if args.no_cpu_baseline else full_parity(t2, b2, r2)}
                d2.free()
                del b2
            extra["other_regimes"] = regimes
            # BASELINE configs 2 and 4 in the same line
            extra["configs"] = {
                "ur5_B4096": measure_config(solver, "ur5", 4096 if B >= 4096 else B, 20, bounds="tight", jacobians="dense"),
                "jvrc_B65536": measure_config(solver, "jvrc", 65536 if B >= 4096 else B, 5, bounds="tight", jacobians="dense"),
                # the headline stack at the size Draco3's own model has (examples/humanoid_draco3.py:55-56: free-flyer root,
                # nv = 33): one coordinate more than a 32-lane group holds -- ik_solve_sweep_kernel<34, 0, 64>, one QP per wavefront
                "draco3_freeflyer_nv33_B65536": measure_config(solver, "draco3_freeflyer", 65536 if B >= 4096 else B, 5, bounds="tight", jacobians="dense"),
                # the headline stack with two position barriers: 30 coordinates + 6 dense rows = 36 tableau rows on a
                # 32-lane group (ik_sweepx.h); the Goldfarb-Idnani kernel alone beside it
                "draco3_2barriers_B65536": measure_config(solver, "draco3b", 65536 if B >= 4096 else B, 5, ab_gi_alone=True, bounds="tight",
                                                          jacobians="dense"),
                # the weakly regularised regime: examples/humanoid_jvrc.py:69-81,112-114 as it is -- nv = 50, four
                # FrameTasks, NO posture task, damping = 1e-12: cond(H) ~ 1e13-1e14.  dq is only determined to
                # cond(H) eps there (two correct solvers differ by far more than 1e-8 along the flat directions): the
                # parity entry certifies the point by its KKT residuals and its objective against the oracle's
                "jvrc_noposture_weakly_regularised_B65536": measure_config(
                    solver, "jvrc_noposture", 65536 if B >= 4096 else B, 5, ab_gi_alone=True, bounds="tight", jacobians="dense"),
                "jvrc_noposture_weakly_regularised_tracking_B65536": measure_config(
                    solver, "jvrc_noposture", 65536 if B >= 4096 else B, 5, ab_gi_alone=True, bounds="kinematic", jacobians="kinematic",
                    error_scale=0.05),
            }
            # C-ABI call from host buffers: H2D + kernel + D2H (pinkhip_solve_host), and a batch of one (config 1)
            bytes_in = int(sum(a.nbytes for _, a in dev.args.streams()))
            e2e = statistics.median(_timed(lambda: solver.solve(batch), 5))
            extra["end_to_end"] = {"call": "pinkhip_solve_host: H2D in ~32 MB chunks overlapped with the kernels, D2H of dq / status / iters",
                                   "host_bytes_in": bytes_in, "host_bytes_out": 8 * B * nv + 8 * B,
                                   "pageable": {"ms": e2e * 1e3, "solves_per_s": B / e2e, "h2d_GBs": bytes_in / e2e / 1e9}}
            if hasattr(solver, "pin"):  # page-locked buffers (pinkhip_host_alloc): DMA at the PCIe rate
                pb, pr = solver.pin(batch), solver.pinned_result(B, nv)
                e2p = statistics.median(_timed(lambda: solver.solve(pb, out=pr), 5))
                extra["end_to_end"]["pinned"] = {"ms": e2p * 1e3, "solves_per_s": B / e2p, "h2d_GBs": bytes_in / e2p / 1e9,
                                                 "same_result": bool(np.array_equal(pr.dq, res.dq))}
                del pb, pr
            one = synthetic.pack(synthetic.make_terms("ur5", 1, bounds="kinematic", jacobians="kinematic"))
            tl = _timed(lambda: solver.solve(one), 200, warmup=20)
            d1 = solver.upload(one)
            extra["latency_B1_us"] = {"config": "UR5 nv=6, 1 FrameTask + PostureTask, batch of one (BASELINE config 1 shape)",
                                      "host_call_median": statistics.median(tl) * 1e6, "host_call_p90": sorted(tl)[int(0.9 * len(tl))] * 1e6,
                                      "kernel_only": kernel_ms_of(solver, d1, 50) * 1e3}
            d1.free()

            try:
                extra["closed_loop_on_device"] = closed_loop_figures(solver, 65536 if B >= 4096 else B)
            except Exception as exc:  # noqa: BLE001  never lose the bench line
                extra["closed_loop_on_device"] = {"failed": repr(exc)}
            # Pink's own calling pattern, batched: solve_ik_batch on Configuration objects (BASELINE config 2's shape:
            # 6-dof arm, 1 FrameTask + PostureTask, one target per instance)
            try:
                extra["api_solve_ik_batch"] = api_level(solver, B=4096 if B >= 4096 else 64, Bh=65536 if B >= 4096 else B)  # (small: the CPU dry runs of tests/)
            except Exception as exc:  # noqa: BLE001  never lose the bench line
                extra["api_solve_ik_batch"] = {"failed": repr(exc)}

        total = global_batch * args.steps
        value = total / elapsed
        bytes_qp = batch.bytes_per_qp()
        achieved = bytes_qp * B / (kernel_ms * 1e-3) / 1e9
        it_mean = float(res.iters.mean())
        fl = flops_per_qp(batch, it_mean)
        tflops = fl * B / (kernel_ms * 1e-3) / 1e12
        traffic, traffic_source = traffic_from_profiles() if (args.config, B, args.bounds) == ("draco3", 65536, "tight") else (None, "not the profiled workload")
        line = {
            "metric": "ik_qp_solves_per_s",
            "value": value,
            "unit": "solves/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / max(args.steps, 1) * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"{args.config}-shaped stand-in: nv={nv}, {len(terms.dense_tasks)} FrameTask(6 rows)+PostureTask, "
                            f"box limits, md={batch.md} barrier rows, B={B} per GPU, bounds={args.bounds}, jacobians={args.jacobians}",
                "batch_per_gpu": B, "global_batch": global_batch, "nv": nv, "Kd": batch.Kd, "K": batch.K, "md": batch.md,
                "parallelism": f"batch-sharded x{world}",
                "solver": "active set by single principal pivoting (largest objective change, started from the active set "
                          "x_i = -c_i / H_ii guesses; Goldfarb-Idnani's dual method behind it where dense rows make a pivot irregular) on a "
                          "register-resident sweep tableau, HIP fp64, 64/W QPs per wavefront (W = 32 lanes per QP at nv = 30), closing trips that "
                          "refine the point and certify it against the KKT conditions (an instance that fails is solved again by the "
                          "Goldfarb-Idnani kernel of round 2 in the same launch)",
            },
            "roofline": {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                "kernel": "ik_solve_sweep_kernel", "kernel_ms": kernel_ms, "bytes_per_qp": bytes_qp,
                "note": "fused stack+solve is VALU-issue bound, not HBM bound (see roofline_fp64; DESIGN.md 3.1); "
                        "stack_only is the HBM-streaming kernel",
            },
            "roofline_fp64": {
                "bound": "fp64 vector ALU", "flops_per_qp": fl, "iters_mean": it_mean, "achieved": tflops,
                "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tflops / FP64_VECTOR_PEAK_TFLOPS,
                "model": "Kd nv (nv+1) + 2 Kd nv + nv^3/3 + 2 nv^2 + iters (4 nv^2 + 2 md nv), SURVEY.md 8(d); useful flops, not issued lanes",
            },
            # (the counter pass is of the default workload: its instruction count says nothing about another batch or regime)
            "roofline_valu_issue": _valu_issue(kernel_ms, int(info.get("compute_units") or 256)) if traffic is not None else None,
            "solver_stats": dict({"failed": n_bad, "iters_mean": it_mean, "iters_max": int(res.iters.max())}, **solver_paths(res)),
            "per_rank_kernel_ms": kernel_ms_ranks,
            "per_rank_end_to_end_ms": e2e_ranks,
            "end_to_end_solves_per_s_all_ranks": None if not e2e_ranks else global_batch / (max(e2e_ranks) * 1e-3),
            "gather": gather,
            "comm_note": comm_note,
            "device": info.get("gcn_arch"),
        }
        # what actually bounds the fused kernel, inside the roofline object (round-5 review): the VALU issue rate
        vi = line.get("roofline_valu_issue")
        line["roofline"]["bound_actual"] = "valu_issue"
        line["roofline"]["bound_actual_frac"] = None if not vi else vi["frac"]
        line.update(extra)
        if not args.no_cpu_baseline:
            base, _, _ = cpu_baseline(terms)
            line["cpu_baseline"] = base
            line["parity"] = full_parity(terms, batch, res, n_exact=8)  # every instance of rank 0's batch
        _emit(_headline_and_detail(line))
    if abandoned:  # a thread of this process may still sit inside an RCCL call: no orderly teardown
        sys.stdout.flush()
        os._exit(0)
    try:
        rdzv.barrier()
    except (OSError, ConnectionError):  # a rank that abandoned a collective has left already
        os._exit(0)
    dev.free()
    if comm is not None:
        comm.close()
    solver.close()
    rdzv.close()


if __name__ == "__main__":
    main()
