"""One call per launching plan kind through the C ABI, at the smallest entry of its table (dispatch.h PINKHIP_FAMILIES):
every family is launched by the one launcher unit (tu_kernel.hip) through the one lookup (launchers.h find_launcher), so
a wrong grid, LDS size or argument fix-up there shows here, in seconds.

Batch: B = 2 (64 / W) + 1 instances -- two full wavefronts of groups plus a tail group.  Each call is held to the C
oracle at the tolerance the parity tests already use for that path (tests/parity_suite.py TOL_DQ for stack + solve,
1e-8 on the velocity for the whole-step kernels: tests/test_rollout.py), and ``PINKHIP_ITERS_PATH`` must name the code
of the family that was meant to run: TABLEAU for the tableau families, GI for the Goldfarb-Idnani kernel."""
import ctypes

import numpy as np
import pytest

import pink_amd
from oracle import c_oracle
from pink_amd import Configuration, FrameTask, PostureTask, build_chain
from pink_amd._lib import PackedArgs
from pink_amd.barriers import PositionBarrier, SelfCollisionBarrier
from pink_amd.barriers.self_collision_barrier import SpherePairs
from pink_amd.rollout import DeviceRollout, pose12
from pink_amd.runtime import set_default_solver

from tests import parity_suite as ps
from tests.cases import random_case

pytestmark = pytest.mark.gpu

PATH_TABLEAU, PATH_GI = 0, 3  # include/pinkhip.h
PLAN_SWEEP, PLAN_SWEEPX, PLAN_PACKED = 3, 4, 5  # dispatch.h, PlanKind


def _batch(W):
    return 2 * (64 // W) + 1


# (name, nv, md, PINKHIP_SOLVER, the plan {kind, NV, MD, W, dense}, path)
SOLVE_KINDS = [
    ("packed", 6, 0, "packed", (PLAN_PACKED, 6, 0, 8, 0), PATH_GI),
    ("packed_dense", 6, 1, "packed", (PLAN_PACKED, 6, 0, 8, 1), PATH_GI),
    ("sweep", 8, 0, None, (PLAN_SWEEP, 8, 0, 16, 0), PATH_TABLEAU),
    ("sweep_rows", 12, 4, None, (PLAN_SWEEP, 12, 4, 16, 0), PATH_TABLEAU),
    ("sweepx", 16, 8, None, (PLAN_SWEEPX, 16, 8, 16, 0), PATH_TABLEAU),
]


@pytest.mark.parametrize("name,nv,md,solver,plan,path", SOLVE_KINDS, ids=[k[0] for k in SOLVE_KINDS])
def test_stack_and_solve_families(gpu_solver, emu, monkeypatch, name, nv, md, solver, plan, path):
    if solver:
        monkeypatch.setenv("PINKHIP_SOLVER", solver)
    else:
        monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
    B = _batch(plan[3])
    batch, pf = random_case(nv, B, 40 + nv + md, md=md)
    planned = (ctypes.c_int * 6)()
    assert emu.lib.pinkhip_emu_plan_solve(ctypes.byref(PackedArgs(batch).desc), ctypes.byref(planned)) == 0
    assert tuple(planned)[:5] == plan and planned[5] == 3  # (the shared host plan: two full wavefronts and the tail)
    out, _ = ps.check_against_oracle(gpu_solver, batch, pf)
    assert (out.path == path).all(), out.path


def test_warm_sweep_family(gpu_solver, monkeypatch):
    monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
    batch, pf = random_case(16, _batch(16), 61)
    ref = c_oracle.solve_ik_batch(**pf)
    assert (ref["status"] == 0).all()
    out = gpu_solver.solve(batch, return_active=True)  # pinkhip_solve_warm_device: <16, 0, 16> of PINKHIP_WSWEEP_TABLE
    err = np.abs(out.dq - ref["dq"]).max()
    print(f"warm sweep: max|dq - dq_oracle| = {err:.3e}")
    assert (out.status == 0).all() and err <= ps.TOL_DQ
    assert (out.path == PATH_TABLEAU).all() and out.active is not None and out.active.shape == (batch.B, 16)


def _arm12(B):
    """The 12-joint arm of tests/test_rollout.py (nv = nj = 12: the 16-lane entries), B configurations, frame targets"""
    model, frames = build_chain(12, seed=5), ["tool0", "joint_6"]
    rng = np.random.default_rng(7)
    q0 = np.tile(model.neutral(), (B, 1))
    for j in model.joints:
        q0[:, j.idx_q] = rng.uniform(-0.6, 0.6, size=B)
    specs = [(f, 1.0, 0.5 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    targets, host_tasks = np.zeros((B, len(frames), 12)), []
    for b in range(B):
        cfg, tl = Configuration(model, q0[b]), []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            tgt = cfg.get_transform_frame_to_world(f).copy()
            tgt.translation = tgt.translation + (np.array([0.0, 0.0, 0.08]) if i == 0 else 0.02 * rng.normal(size=3))
            t.set_target(tgt)
            targets[b, i] = pose12(tgt)
            tl.append(t)
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        tl.append(p)
        host_tasks.append(tl)
    return model, frames, q0, specs, targets, host_tasks


def _barriers(kind, model, q0):
    if kind == "rdense":  # one row: a ceiling 1 cm above the highest tool, every target 8 cm above its tool
        z = [Configuration(model, q).get_transform_frame_to_world("tool0").translation[2] for q in q0]
        return [PositionBarrier("tool0", indices=[2], p_max=np.array([max(z) + 0.01]), gain=np.array([50.0]))]
    if kind == "rpairs":  # two rows: the two closest of four sphere pairs
        sph = [(1, [0.02, 0.0, 0.01], 0.04), (3, [0.0, 0.03, 0.0], 0.05), (8, [0.05, 0.0, 0.0], 0.03), (11, [0.1, 0.0, 0.0], 0.05)]
        query = SpherePairs([sph[a] + sph[b] for a, b in ((0, 2), (0, 3), (1, 2), (1, 3))])
        return [SelfCollisionBarrier(2, gain=1.0, safe_displacement_gain=1.0, d_min=0.05, distance_query=query)]
    return []


@pytest.mark.parametrize("kind", ["rollout", "rdense", "wrollout", "rpairs"])
def test_whole_step_families(gpu_solver, kind):
    """<12, 0, 16> of PINKHIP_ROLLOUT_TABLE, <12, 4, 16> of PINKHIP_ROLLOUT_DENSE_TABLE, <16, 0, 16> of PINKHIP_WROLLOUT_TABLE
    and <12, 4, 16> of PINKHIP_RPAIRS_TABLE: one control step, not integrated, against the oracle's minimiser of the QP
    that build_ik states for every robot."""
    B, dt = _batch(16), 5e-3
    model, frames, q0, specs, targets, host_tasks = _arm12(B)
    bars = _barriers(kind, model, q0)
    set_default_solver(gpu_solver)
    try:
        ro = DeviceRollout(gpu_solver, model, q0, specs, dt, posture_cost=1e-2, fused="kernel", position_barriers=bars, warm_start=kind == "wrollout")
        try:
            ro.set_targets(targets)
            ro.step(integrate=False)
            gpu_solver.sync()
            assert ro.fused == "kernel" and ro.md == {"rollout": 0, "rdense": 1, "wrollout": 0, "rpairs": 2}[kind]
            dq, st, _ = ro.last_step()
            assert (st == 0).all() and (ro.last_path == PATH_TABLEAU).all(), (st, ro.last_path)
            if kind == "wrollout":
                assert ro.last_active().shape == (B, 12)
        finally:
            ro.free()
        worst = 0.0
        for b in range(B):
            qp = pink_amd.build_ik(Configuration(model, q0[b]), host_tasks[b], dt, barriers=bars or None)
            x, status, _, _ = c_oracle.gi_solve(qp.P, qp.q, qp.G, qp.h)
            assert status == 0
            worst = max(worst, float(np.abs(dq[b] - x).max()) / dt)
        print(f"{kind}: max|v - v_oracle| = {worst:.3e}")
        assert worst < 1e-8
    finally:
        pink_amd.clear_device_cache()
        set_default_solver(None)
