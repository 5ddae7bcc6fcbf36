"""The sweep-tableau kernels keep a lane's own diagonal entry in a register from the first stacked row on, address the
streams with a scalar base and one 32-bit offset per lane, and form the LDS addresses of the closing product where they
are used (pink_amd/csrc/ik_sweep.h, ik_stack_rows.h: add_in_lane, WaveSplit).  None of that may change a result: every
instantiation family that shares the code solves a small batch, is held to the C oracle (pink/solve_ik.py:206-275 through
Goldfarb-Idnani) at the suite's 1e-10, and is run twice with bit-equal results.  Emulator here, MI355X under -m gpu.

B = 7 throughout: odd, so the last wave holds a surplus group that redoes the last instance and writes nothing.  In the
stack + solve cases instance 1 has an infinite bound on every coordinate (nothing to guess, nothing to exchange) and
instance 2 a box that the diagonal guess x_i = -c_i / H_ii violates in every bounded coordinate (the start fixes them all:
no initial sweep runs, the diagonal register is all the start has).  The whole-step kernel takes its bounds from the model
and starts with every coordinate free, so its case has the odd batch only.

Shapes: nv = 30 and the padded nv = 29 (the identity row of the pad lane goes through the diagonal register) on
<30, 0, 32>; nv = 32 on <32, 0, 32>; nv = 16 and 13 on <16, 0, 16> (four groups per wave; an odd nv is an odd row pitch);
nv = 33 / 34 with free leading coordinates on <34, 0, 32> (the front elimination updates the register); nv = 50 on
<50, 0, 64>; nv = 30 with two dense rows on <30, 2, 32>; one DeviceRollout step at nv = 30 (rows of six formed on chip)."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import pink_oracle as po
from pink_amd import Configuration, FrameTask, PostureTask, build_chain, build_ik
from pink_amd._lib import PackedArgs
from pink_amd.lie import SE3, exp3
from pink_amd.rollout import DeviceRollout, pose12

from tests.cases import random_case

B = 7
TOL = 1e-10


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def solver(request):
    return request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver")


_CASES = {}


def _case(nv, md, lead):
    """(batch, oracle result) of one shape, built and solved by the oracle once."""
    key = (nv, md, lead)
    if key in _CASES:
        return _CASES[key]
    batch, pf = random_case(nv, B, 100 + nv + md, md=md, root=lead)
    lb, ub = batch.lb, batch.ub
    # instance 1: no bound at all
    lb[1], ub[1] = -np.inf, np.inf
    # instance 2: every bounded coordinate starts fixed -- the box lies strictly below (even coordinates) resp. above (odd
    # ones) the point the diagonal guess looks at
    Hc = c_oracle.solve_ik_batch(**dict(pf, G=None, h=None), want_Hc=True, solve=False)
    xd = -Hc["c"][2] / np.diagonal(Hc["H"][2])
    idx = np.arange(lead, nv)
    below = idx % 2 == 0
    ub[2, idx] = np.where(below, xd[idx] - 0.01, xd[idx] + 0.06)
    lb[2, idx] = np.where(below, xd[idx] - 0.06, xd[idx] + 0.01)
    # (the oracle's rows: +e_i x <= ub, -e_i x <= -lb, then the dense rows -- tests/cases.py)
    hb = np.concatenate([ub, -lb], axis=1)
    pf["h"][:, :2 * nv] = np.where(np.isfinite(hb), hb, 1e30)
    ref = c_oracle.solve_ik_batch(**pf)
    assert (ref["status"] == 0).all(), "an infeasible draw would hide a failure"
    _CASES[key] = (batch, ref)
    return _CASES[key]


@pytest.mark.parametrize("nv,md,lead", [(30, 0, 0), (29, 0, 0), (32, 0, 0), (16, 0, 0), (13, 0, 0), (33, 0, 6), (34, 0, 6),
                                        (50, 0, 0), (30, 2, 0)])
def test_stack_and_solve_families(solver, nv, md, lead):
    batch, ref = _case(nv, md, lead)
    if lead:
        assert PackedArgs(batch).desc.n_free_lead == lead  # (what selects the instantiation with the front elimination)
    one = solver.solve(batch)
    two = solver.solve(batch)
    err = float(np.abs(one.dq - ref["dq"]).max())
    print(f"nv={nv} md={md} lead={lead}: max|dq - dq_ref| = {err:.3e}, iters {one.iters.tolist()}, path {one.path.tolist()}")
    assert np.array_equal(one.status, ref["status"])
    assert (one.path == 0).all()  # the tableau code itself, no hand-over
    assert err < TOL
    # instance 1 is its unconstrained minimiser (no exchange); instance 2 sits on at least one of its bounds
    if md == 0:
        assert one.iters[1] == 0
    assert (np.isclose(one.dq[2], batch.lb[2], atol=1e-12) | np.isclose(one.dq[2], batch.ub[2], atol=1e-12)).any()
    assert np.array_equal(one.dq, two.dq) and np.array_equal(one.status, two.status) and np.array_equal(one.iters, two.iters)


def _rollout_step(solver, model, q0, specs, targets, dt):
    ro = DeviceRollout(solver, model, q0, specs, dt, posture_cost=5e-2, fused="kernel")
    ro.set_targets(targets)
    ro.step()
    solver.sync()
    dq, st, it = ro.last_step()
    out = dq.copy(), st.copy(), it.copy(), ro.last_path.copy(), ro.configurations().copy()
    assert ro.fused == "kernel"
    ro.free()
    return out


def test_whole_step_kernel_at_nv30(solver):
    from tests.test_rollout import _random_q

    model, frames = build_chain(24, free_flyer=True, seed=2), ["tool0", "joint_12"]
    assert model.nv == 30
    rng = np.random.default_rng(77)
    dt = 5e-3
    q0 = _random_q(model, B, rng) * 0.6 + 0.4 * np.tile(model.neutral(), (B, 1))
    q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    specs = [(f, 1.0, 0.5, 0.9, 1e-3) for f in frames]
    targets = np.zeros((B, len(frames), 12))
    ref = np.zeros((B, model.nv))
    for b in range(B):
        cfg = Configuration(model, q0[b])
        tasks = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            d = rng.normal(size=3)
            tgt = cfg.get_transform_frame_to_world(f) * SE3(exp3(0.3 * rng.normal(size=3)), 0.3 * d / np.linalg.norm(d))
            targets[b, i] = pose12(tgt)
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            t.set_target(tgt)
            tasks.append(t)
        post = PostureTask(cost=5e-2)
        post.set_target(q0[b])
        tasks.append(post)
        prob = build_ik(cfg, tasks, dt)
        P, q = po.qp_objective(model.nv, [(t.compute_jacobian(cfg), t.compute_error(cfg), t.cost, t.gain, getattr(t, "lm_damping", 0.0))
                                          for t in tasks], 1e-12)
        x, st, _, _ = c_oracle.gi_solve(P, q, prob.G, prob.h)
        assert st == 0
        ref[b] = x
    dq, st, it, path, q1 = _rollout_step(solver, model, q0, specs, targets, dt)
    err = float(np.abs(dq - ref).max())
    print(f"whole-step kernel nv=30: max|dq - dq_ref| = {err:.3e}, iters {it.tolist()}, path {path.tolist()}")
    assert (st == 0).all() and (path == 0).all()
    assert np.abs(ref).max() > 1e-4 and err < TOL
    dq2, st2, it2, _, q2 = _rollout_step(solver, model, q0, specs, targets, dt)
    assert np.array_equal(dq, dq2) and np.array_equal(st, st2) and np.array_equal(it, it2) and np.array_equal(q1, q2)
