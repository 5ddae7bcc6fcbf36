"""SelfCollisionBarrier rows of sphere pairs selected and formed by the whole-step kernel (``ik_rollout.h`` PAIRS,
``pinkhip_rollout_step_pairs_device``): per robot the world centres of the spheres, the distance of every pair, the
``n_collision_pairs`` closest pairs and one dense row each -- the device route of ``solve_ik_batch`` and the closed loop
of ``DeviceRollout``.  Expected values come from the reference's own rows (tests/golden/pink_round4.npz, ``sc_*``) or
from the host-evaluated route; emulator here, MI355X under ``-m gpu``.

Robots are ``build_chain`` arms: the 9-joint chain behind a free-flyer ("humanoid", nv = 15) of the golden cases, its
7-joint fixed-base sibling, and a 36-joint chain (nv = 36 -- 36 fits the LDS check of ``select_rollout_pairs``: one robot per
wavefront on ``<50, 14, 64>``)."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import pink_amd
from oracle import c_oracle
from pink_amd import Configuration, ConfigurationBatch, FrameTask, PostureTask, build_chain, solve_ik, solve_ik_batch
from pink_amd._lib import ABI_SYMBOLS, Desc, PinkHipError, RolloutStep, SpherePairsArgs
from pink_amd.barriers import PositionBarrier, SelfCollisionBarrier
from pink_amd.barriers.self_collision_barrier import SpherePairs
from pink_amd.exceptions import PinkError
from pink_amd.rollout import DeviceRollout, ModelDesc, pose12
from pink_amd.runtime import set_default_solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_ROLLOUT_PAIRS = 10  # host_plan.h, PlanKind


class PairsSpy:
    """A solver object plus ``rollout_step_pairs`` -- the emulator's (``emu`` has none, so that every other test keeps its
    route) or the library's own -- that remembers the model description and the arguments of the last such call, so that a
    test can ask the host plan (``host_plan.h`` through the emulator's harness) which instantiation ran it."""

    def __init__(self, inner, emu, on_gpu):
        self._inner, self._emu, self.on_gpu = inner, emu, on_gpu
        lib = emu.lib
        args = [ctypes.POINTER(Desc), ctypes.c_void_p, ctypes.POINTER(RolloutStep), ctypes.POINTER(SpherePairsArgs)]
        lib.pinkhip_emu_rollout_step_pairs.argtypes = args
        lib.pinkhip_emu_plan_rollout_pairs.argtypes = args + [ctypes.POINTER(ctypes.c_int * 6)]
        lib.pinkhip_emu_pairs_last_error.restype = ctypes.c_char_p
        self.last_call = self.last_model = None

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def model_create(self, desc):
        self.last_model = desc
        return self._inner.model_create(desc)

    def rollout_step_pairs(self, desc, model, args, pairs):
        self.last_call = (desc, args, pairs)
        if self.on_gpu:
            return self._inner.rollout_step_pairs(desc, model, args, pairs)
        rc = self._emu.lib.pinkhip_emu_rollout_step_pairs(ctypes.byref(desc), model, ctypes.byref(args), ctypes.byref(pairs))
        if rc == -5:
            return False
        if rc != 0:
            raise PinkHipError(rc, self._emu.lib.pinkhip_emu_pairs_last_error().decode())
        return True

    def planned(self):
        """``(NV, MD, W)`` of the instantiation the last ``rollout_step_pairs`` call ran on (the plan looks at no array)."""
        desc, args, pairs = self.last_call
        model = self._emu.model_create(self.last_model)
        out = (ctypes.c_int * 6)()
        try:
            rc = self._emu.lib.pinkhip_emu_plan_rollout_pairs(ctypes.byref(desc), model, ctypes.byref(args), ctypes.byref(pairs), ctypes.byref(out))
        finally:
            self._emu.model_destroy(model)
        assert rc == 0 and out[0] == PLAN_ROLLOUT_PAIRS, (rc, list(out))
        return out[1], out[2], out[3]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    emu = request.getfixturevalue("emu")
    spy = PairsSpy(emu if request.param == "emu" else request.getfixturevalue("gpu_solver"), emu, request.param == "gpu")
    set_default_solver(spy)
    yield spy
    pink_amd.clear_device_cache()
    set_default_solver(None)


@pytest.fixture(scope="module")
def golden4():
    return np.load(os.path.join(ROOT, "tests", "golden", "pink_round4.npz"))


def _declined_reason():
    return sys.modules["pink_amd.solve_ik"]._DECLINED["reason"]


def _route():
    return pink_amd.last_solve_stats()["route"]


def _golden_query(g, case):
    return SpherePairs([(int(r[0]), r[1:4], float(r[4]), int(r[5]), r[6:9], float(r[9])) for r in g[f"{case}/pairs"]])


def _humanoid():
    return build_chain(9, free_flyer=True, seed=6)  # (the robot of the golden case sc_humanoid)


_HUM = {}


def _humanoid_batch(B=70, seed=11):
    """``B`` random configurations of the humanoid and six pairs over five distinct spheres (built once)."""
    if (B, seed) not in _HUM:
        m = _humanoid()
        rng = np.random.default_rng(seed)
        q = np.tile(m.neutral(), (B, 1))
        for j in m.joints:
            if j.kind != "free_flyer":
                q[:, j.idx_q] = rng.uniform(-1.2, 1.2, size=B)
        quat = rng.normal(size=(B, 4))
        q[:, 0:3], q[:, 3:7] = 0.3 * rng.normal(size=(B, 3)), quat / np.linalg.norm(quat, axis=1, keepdims=True)
        nj = len(m.joints)
        sph = [(1, [0.02, 0.0, 0.01], 0.04), (3, [0.0, 0.03, 0.0], 0.05), (5, [0.05, 0.0, 0.0], 0.03), (nj - 3, [0.0, 0.0, 0.04], 0.04),
               (nj - 1, [0.1, 0.0, 0.0], 0.05)]
        pairs = [sph[a] + sph[b] for a, b in ((0, 3), (0, 4), (1, 3), (1, 4), (2, 4), (0, 2))]
        _HUM[(B, seed)] = (m, q, SpherePairs(pairs))
    m, q, query = _HUM[(B, seed)]
    return m, q.copy(), query


def _pair_distances(m, q, query):
    """[B, n_pairs] distances of the host's distance query."""
    return np.array([[p.min_distance for p in query(Configuration(m, qb))] for qb in q])


def _tasks(m, q0, lift=(0.03, -0.02, 0.04), posture_cost=1e-2):
    cfg = Configuration(m, q0)
    ft = FrameTask("tool0", 1.0, 0.5, lm_damping=1e-3)
    T = cfg.get_transform_frame_to_world("tool0").copy()
    T.translation = T.translation + np.array(lift)
    ft.set_target(T)
    po = PostureTask(cost=posture_cost)
    po.set_target(m.neutral())
    return ft, po


def _close(V_dev, V_host):
    assert np.isfinite(V_dev).all()
    assert np.abs(V_dev - V_host).max() < 1e-8 * max(1.0, np.abs(V_host).max())


# ------------------------------------------------------------------------------------------ 1. the reference's rows
@pytest.mark.parametrize("case,name,inst", [("sc_arm", "all", (30, 6, 32)), ("sc_arm", "closest2", (12, 4, 16)),
                                            ("sc_humanoid", "all", (30, 6, 32)), ("sc_humanoid", "closest2", (30, 6, 32))])
def test_device_route_pair_rows_are_the_references(api, golden4, case, name, inst):
    """The velocity of the device route is the minimiser of the QP whose barrier rows and regulariser the REFERENCE's class
    made of the same sphere pairs (``sc_*/{all, closest2}/{G, h, H, c}``), solved by the oracle from those arrays: pink_amd's
    barrier class does not enter the expected value."""
    g = golden4
    m = build_chain(int(g[f"{case}/n"]), free_flyer=bool(g[f"{case}/ff"]), seed=6)
    cfg, dt = Configuration(m, g[f"{case}/q"].copy()), float(g[f"{case}/dt"])
    ft, po = _tasks(m, cfg.q, lift=(0.02, -0.01, 0.05))
    base = pink_amd.build_ik(cfg, [ft, po], dt)  # the stack without barriers: P, q, limit rows (pinned to the reference elsewhere)
    cb = ConfigurationBatch(m, np.tile(cfg.q, (66, 1)))
    sb = SelfCollisionBarrier(int(g[f"{case}/{name}/n_collision_pairs"]), gain=float(g[f"{case}/{name}/gain"]),
                              safe_displacement_gain=float(g[f"{case}/{name}/safe_displacement_gain"]), d_min=float(g[f"{case}/{name}/d_min"]),
                              distance_query=_golden_query(g, case))
    V = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device"
    assert api.planned() == inst
    P, q = base.P + g[f"{case}/{name}/H"], base.q + g[f"{case}/{name}/c"]
    G, h = np.vstack([base.G, g[f"{case}/{name}/G"]]), np.concatenate([base.h, g[f"{case}/{name}/h"]])
    x_ref, status, _, _ = c_oracle.gi_solve(P, q, G, h)
    assert status == 0
    err = np.abs(V * dt - x_ref[None, :]).max()
    print(f"{case}/{name}: max|dq - x_ref| = {err:.3e}")
    assert err < 1e-9 * max(1.0, np.abs(x_ref).max())
    assert np.array_equal(V, np.tile(V[0], (V.shape[0], 1)))  # (the same robot 66 times)


# ---------------------------------------------------------------- 2. rows that bind, a selection that differs per robot
def test_binding_rows_and_per_robot_selection(api):
    m, q, query = _humanoid_batch()
    B, dt = q.shape[0], 5e-3
    dist = _pair_distances(m, q, query)
    srt = np.sort(dist, axis=1)
    d_min = float(np.median(srt[:, 0]))  # the closest pair of about half the robots is inside it
    sb = SelfCollisionBarrier(3, gain=1.0, safe_displacement_gain=1.0, d_min=d_min, distance_query=query)
    ft, po = _tasks(m, q[0])
    cb = ConfigurationBatch(m, q)
    V_host = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=False)
    assert pink_amd.last_solve_stats()["failed"] == 0
    # conditions on the inputs, from the host class's rows
    assert (srt[:, 3] - srt[:, 2]).min() > 1e-6
    selections = {tuple(sorted(np.argsort(d)[:3])) for d in dist}
    assert len(selections) >= 3, selections
    active = 0
    for b in range(B):
        G, h = sb.compute_qp_inequalities(Configuration(m, q[b]), dt)
        active += bool((np.abs(G @ (V_host[b] * dt) - h) <= 1e-9 * (1.0 + np.abs(h))).any())
    assert active >= B / 4, active
    assert 0.3 * B <= (srt[:, 0] < d_min).sum() <= 0.7 * B
    V = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device" and pink_amd.last_solve_stats()["failed"] == 0
    assert api.planned() == (30, 6, 32)
    print(f"binding rows: {active} of {B} robots, {len(selections)} selections, max|V - V_host| = {np.abs(V - V_host).max():.3e}")
    _close(V, V_host)


# ------------------------------------------------------------------------------------------ 3. mixed stack on <50, 14, 64>
def test_mixed_stack_with_constraint_and_position_barrier(api):
    """One equality constraint (a FrameTask), one PositionBarrier and the self-collision barrier: md = 6 + 1 + 2 dense rows,
    the pair rows last."""
    m, q, query = _humanoid_batch()
    q, dt = q[:6], 5e-3  # (one robot per wavefront: six blocks)
    ft, po = _tasks(m, q[0])
    hold = FrameTask("joint_2", 1.0, 1.0)
    hold.set_target(Configuration(m, q[0]).get_transform_frame_to_world("joint_2"))
    z = np.array([Configuration(m, qb).get_transform_frame_to_world("tool0").translation[2] for qb in q])
    pb = PositionBarrier("tool0", indices=[2], p_max=np.array([z.max() + 0.01]), gain=np.array([20.0]))
    sb = SelfCollisionBarrier(2, gain=2.0, safe_displacement_gain=1.0, d_min=float(np.median(_pair_distances(m, q, query).min(axis=1))), distance_query=query)
    cb = ConfigurationBatch(m, np.tile(q[0], (6, 1)))  # (the constraint holds joint_2 where robot 0 has it)
    kw = dict(barriers=[sb, pb], constraints=[hold])
    V_host = solve_ik_batch(cb, [ft, po], dt, device_kinematics=False, **kw)
    V = solve_ik_batch(cb, [ft, po], dt, device_kinematics=True, **kw)
    assert _route() == "device" and api.planned() == (50, 14, 64)
    assert api.last_call[0].md == 9 and api.last_call[2].n_rows == 2
    _close(V, V_host)


def test_chain_of_36_joints_with_eight_pair_rows(api):
    m = build_chain(36, seed=3, link_length=0.1)
    rng = np.random.default_rng(5)
    B, dt = 6, 5e-3  # (one robot per wavefront: six blocks)
    q = rng.uniform(-0.6, 0.6, size=(B, m.nq))
    sph = [(j, [0.01 * (j % 3), 0.0, 0.01], 0.02 + 0.001 * (j % 5)) for j in range(0, 36, 3)]  # 12 spheres
    pairs = [sph[a] + sph[b] for a in range(12) for b in range(a + 2, 12)][:40]
    query = SpherePairs(pairs)
    dist = _pair_distances(m, q, query)
    sb = SelfCollisionBarrier(8, gain=1.0, safe_displacement_gain=1.0, d_min=float(np.median(dist.min(axis=1))), distance_query=query)
    srt = np.sort(dist, axis=1)
    assert (srt[:, 8] - srt[:, 7]).min() > 1e-6
    ft, po = _tasks(m, q[0], posture_cost=1e-1)
    cb = ConfigurationBatch(m, q)
    V_host = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=False)
    V = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device" and api.planned() == (50, 14, 64)
    _close(V, V_host)


# ------------------------------------------------------------------------------- 4. the Goldfarb-Idnani code forms the rows
def test_rank_deficient_stack_goes_through_the_goldfarb_idnani_code(api):
    """A FrameTask alone on 15 coordinates -- no Levenberg-Marquardt term, no barrier regulariser -- is rank deficient by
    construction: the kernel goes straight to the Goldfarb-Idnani code, whose kinematics pass runs the sphere-pair stage."""
    m, q, query = _humanoid_batch()
    dt = 5e-3
    dist = _pair_distances(m, q, query)
    sb = SelfCollisionBarrier(3, gain=1.0, safe_displacement_gain=0.0, d_min=float(np.median(dist.min(axis=1))), distance_query=query)
    ft, _ = _tasks(m, q[0])
    ft.lm_damping = 0.0
    cb = ConfigurationBatch(m, q)
    V_host = solve_ik_batch(cb, [ft], dt, barriers=[sb], device_kinematics=False)
    V = solve_ik_batch(cb, [ft], dt, barriers=[sb], device_kinematics=True)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "device" and stats["paths"]["goldfarb_idnani"] == 1.0, stats
    # H = J^T W J + 1e-12 I has a null space but for the damping: that component of the velocity is fixed to ~1e-4 only, in
    # either route (the project's bound for this kind of stack, tests/test_round4.py; 1.5e-4 measured on the emulator) ...
    assert np.isfinite(V).all()
    err = np.abs(V - V_host).max() / max(1.0, np.abs(V_host).max())
    print(f"rank deficient: max|V - V_host| / max(1, |V_host|) = {err:.3e}")
    assert err < 1e-3
    # ... while what the QP does determine is the same to rounding: the rows hold and the objective has the host's value
    for b in range(0, q.shape[0], 7):
        qp = pink_amd.build_ik(Configuration(m, q[b]), [ft], dt, barriers=[sb])
        x, x_host = V[b] * dt, V_host[b] * dt
        assert (qp.G @ x <= qp.h + 1e-9 * (1.0 + np.abs(qp.h))).all()
        f, f_host = (0.5 * y @ qp.P @ y + qp.q @ y for y in (x, x_host))
        assert abs(f - f_host) < 1e-8 * max(1.0, abs(f_host)), (b, f, f_host)


# ---------------------------------------------------------------------------------------------------------- 5. edges
def _copies(m, q0, B=66):
    return ConfigurationBatch(m, np.tile(q0, (B, 1)))


def test_touching_pair_gives_a_zero_row_on_both_routes(api):
    m, q, _ = _humanoid_batch()
    q0, dt = q[0], 5e-3
    cfg = Configuration(m, q0)
    nj = len(m.joints)
    c1, c2 = np.array([0.02, 0.0, 0.01]), np.array([0.1, 0.0, 0.0])
    rho = float(np.linalg.norm(cfg.oMi[nj - 1].act(c2) - cfg.oMi[1].act(c1)))
    r1 = 0.4 * rho
    query = SpherePairs([(1, c1, r1, nj - 1, c2, rho - r1 - 1e-7),  # 1e-7 from touching: the closest pair
                         (3, [0.0, 0.03, 0.0], 0.05, nj - 1, c2, 0.02), (1, c1, 0.01, 5, [0.05, 0.0, 0.0], 0.03)])
    sb = SelfCollisionBarrier(2, gain=3.0, safe_displacement_gain=0.0, d_min=0.0, distance_query=query)
    d = np.array([p.min_distance for p in query(cfg)])
    assert abs(d[0] - 1e-7) < 1e-12 and d[0] == d.min()
    J = sb.compute_jacobian(cfg)
    assert (np.abs(J).max(axis=1) == 0.0).sum() == 1  # the host's row of that pair is zero
    ft, po = _tasks(m, q0)
    V_host = solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=[sb], device_kinematics=False)
    V = solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device"
    _close(V, V_host)


def test_every_pair_selected(api):
    m, q, query = _humanoid_batch()
    dt = 5e-3
    dist = _pair_distances(m, q[:66], query)
    sb = SelfCollisionBarrier(len(query.pairs), gain=1.0, safe_displacement_gain=1.0, d_min=float(np.median(dist.min(axis=1))), distance_query=query)
    ft, po = _tasks(m, q[0])
    cb = ConfigurationBatch(m, q[:66])
    V_host = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=False)
    V = solve_ik_batch(cb, [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device" and api.planned() == (30, 6, 32)
    _close(V, V_host)


def _many_spheres(m, n_spheres, n_pairs):
    nj = len(m.joints)
    sph = [(1 + s % (nj - 1), [0.01 * (s % 4), 0.005 * (s % 3), 0.002 * s], 0.01 + 0.0005 * s) for s in range(n_spheres)]
    # (a ring over all spheres, then the pairs two, three, ... apart: neighbours within eight sit on different joints)
    pairs = [sph[a] + sph[(a + k) % n_spheres] for k in range(1, 8) for a in range(n_spheres)]
    pairs = [p for p in pairs if p[0] != p[3]][:n_pairs]
    assert len(pairs) == n_pairs and len({s for p in pairs for s in ((p[0], tuple(p[1]), p[2]), (p[3], tuple(p[4]), p[5]))}) == n_spheres
    return SpherePairs(pairs)


def test_sixty_four_pairs_over_thirty_two_spheres(api):
    m, q, _ = _humanoid_batch()
    q0, dt = q[1], 5e-3
    query = _many_spheres(m, 32, 64)
    d = np.sort([p.min_distance for p in query(Configuration(m, q0))])
    assert d[4] - d[3] > 1e-6
    sb = SelfCollisionBarrier(4, gain=1.0, safe_displacement_gain=1.0, d_min=float(d[1]), distance_query=query)
    ft, po = _tasks(m, q0)
    V_host = solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=[sb], device_kinematics=False)
    V = solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=[sb], device_kinematics=True)
    assert _route() == "device" and api.planned() == (30, 6, 32)
    assert (api.last_call[2].n_spheres, api.last_call[2].n_pairs) == (32, 64)
    _close(V, V_host)


@pytest.mark.parametrize("what", ["33 spheres", "65 pairs", "vector gain", "two barriers", "other query"])
def test_declined_stacks_name_the_term(api, what):
    m, q, query = _humanoid_batch()
    q0, dt = q[2], 5e-3
    kw = dict(gain=1.0, safe_displacement_gain=1.0, d_min=0.01)
    if what == "33 spheres":
        bars = [SelfCollisionBarrier(2, distance_query=_many_spheres(m, 33, 40), **kw)]
    elif what == "65 pairs":
        bars = [SelfCollisionBarrier(2, distance_query=_many_spheres(m, 20, 65), **kw)]
    elif what == "vector gain":
        bars = [SelfCollisionBarrier(2, distance_query=query, **dict(kw, gain=np.array([1.0, 2.0])))]
    elif what == "two barriers":
        bars = [SelfCollisionBarrier(2, distance_query=query, **kw), SelfCollisionBarrier(1, distance_query=query, **kw)]
    else:
        bars = [SelfCollisionBarrier(2, distance_query=lambda cfg: query(cfg), **kw)]
    ft, po = _tasks(m, q0)
    V = solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=bars)
    assert _route() != "device"
    assert "SelfCollisionBarrier" in _declined_reason(), _declined_reason()
    assert np.isfinite(V).all()
    with pytest.raises(PinkError, match="SelfCollisionBarrier"):
        solve_ik_batch(_copies(m, q0), [ft, po], dt, barriers=bars, strict_route="device")


# ----------------------------------------------------------------------------------------------------- 6. closed loop
@pytest.mark.parametrize("n_rows", [3, 2])
def test_closed_loop_keeps_the_links_apart(api, n_rows):
    """``DeviceRollout`` with the barrier against the host loop (per-robot ``solve_ik`` + ``integrate_inplace``): the tool is
    sent toward the sphere on joint_2, the barrier stops it at ``d_min``.  ``n_rows = 3`` keeps every pair, 2 selects."""
    m = build_chain(7, seed=6)
    rng = np.random.default_rng(21)
    B, dt, steps = 5, 5e-3, 12
    q0 = np.tile(np.array([0.2, -0.9, 1.6, 0.9, 0.3, 0.4, 0.1]), (B, 1)) + 0.08 * rng.normal(size=(B, m.nq))
    nj = len(m.joints)
    query = SpherePairs([(1, [0.0, 0.0, 0.02], 0.05, nj - 1, [0.15, 0.0, 0.0], 0.04), (2, [0.1, 0.0, 0.0], 0.04, nj - 1, [0.15, 0.0, 0.0], 0.04),
                         (1, [0.0, 0.0, 0.02], 0.05, nj - 2, [0.05, 0.0, 0.0], 0.03)])
    cfgs = [Configuration(m, q0[b]) for b in range(B)]
    d0 = _pair_distances(m, q0, query)
    d_min = float(d0.min()) - 0.01  # (without the barrier the closest pair of every robot ends 3 to 12 cm closer than that)
    sb = SelfCollisionBarrier(n_rows, gain=100.0, safe_displacement_gain=1.0, d_min=d_min, distance_query=query)
    specs = [("tool0", 1.0, 0.0, 1.0, 1e-3)]
    targets, host_tasks = np.zeros((B, 1, 12)), []
    for b, cfg in enumerate(cfgs):
        t = FrameTask("tool0", 1.0, 0.0, lm_damping=1e-3)
        tgt = cfg.get_transform_frame_to_world("tool0").copy()
        tgt.translation = cfg.oMi[1].act(np.array([0.0, 0.0, 0.02]))  # the centre of the sphere on joint_2
        t.set_target(tgt)
        targets[b, 0] = pose12(tgt)
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        host_tasks.append([t, p])
    ro = DeviceRollout(api, m, q0, specs, dt, posture_cost=1e-2, fused="kernel", position_barriers=[sb])
    try:
        ro.set_targets(targets)
        ro.run(steps)
        assert ro.fused == "kernel" and ro.md == n_rows
        qd = ro.configurations()
        _, st, _ = ro.last_step()
        assert (st == 0).all()
    finally:
        ro.free()
    near = False
    for b, cfg in enumerate(cfgs):
        for _ in range(steps):
            d = np.sort([p.min_distance for p in query(cfg)])
            if n_rows < len(d):  # (the selection is defined only while the pairs it separates differ)
                assert d[n_rows] - d[n_rows - 1] > 1e-6
            cfg.integrate_inplace(solve_ik(cfg, host_tasks[b], dt, barriers=[sb]), dt)
        cd = Configuration(m, qd[b])
        Ta, Tb = cd.get_transform_frame_to_world("tool0"), cfg.get_transform_frame_to_world("tool0")
        assert np.abs(Ta.translation - Tb.translation).max() < 1e-8 and np.abs(Ta.rotation - Tb.rotation).max() < 1e-8
        d_dev, d_host = (np.array([p.min_distance for p in query(c)]) for c in (cd, cfg))
        assert (d_dev >= np.minimum(d_min - 1e-6, d_host - 1e-8)).all(), (d_dev, d_host, d_min)
        near |= bool(d_dev.min() < d_min + 5e-3)
    assert near  # ... and the barrier was needed: at least one robot ends up against it


# -------------------------------------------------------------------------------------------- 7. ABI and code objects
def test_new_symbols_are_exported(built, emu):
    from pink_amd import _lib

    assert "pinkhip_rollout_step_pairs_device" in ABI_SYMBOLS
    assert hasattr(_lib.load_library(), "pinkhip_rollout_step_pairs_device")
    assert "#define PINKHIP_HAS_SPHERE_PAIRS 1" in open(os.path.join(ROOT, "include", "pinkhip.h")).read()
    for name in ("pinkhip_emu_rollout_step_pairs", "pinkhip_emu_plan_rollout_pairs", "pinkhip_emu_pairs_last_error"):
        assert hasattr(emu.lib, name), name


def test_c_call_refuses_what_the_stage_cannot_hold(api):
    m, q, query = _humanoid_batch()
    sb = SelfCollisionBarrier(3, gain=1.0, safe_displacement_gain=1.0, d_min=0.01, distance_query=query)
    ro = DeviceRollout(api, m, q[:4], [("tool0", 1.0, 0.5, 1.0, 1e-3)], 5e-3, posture_cost=1e-2, fused="kernel", position_barriers=[sb])
    try:
        ro.set_targets(np.tile(pose12(Configuration(m, q[0]).get_transform_frame_to_world("tool0")), (4, 1, 1)))
        ro.step(integrate=False)
        api.sync()
        dq0, st0, _ = ro.last_step()
        assert (st0 == 0).all()
        desc, args, pairs = api.last_call

        def call(**change):
            sp = SpherePairsArgs()
            ctypes.memmove(ctypes.byref(sp), ctypes.byref(pairs), ctypes.sizeof(sp))
            for k, v in change.items():
                setattr(sp, k, v)
            return api.rollout_step_pairs(desc, ro.dmodel, args, sp)

        for change in (dict(n_rows=0), dict(n_rows=2), dict(n_pairs=2)):  # (n_rows = 2: the rows are no longer the last group)
            with pytest.raises(PinkHipError) as ei:
                call(**change)
            assert ei.value.code == -1, change
        assert call(n_spheres=33) is False and call(n_pairs=65) is False  # PINKHIP_E_UNSUPPORTED
        api.sync()
        dq1, st1, _ = ro.last_step()
        assert np.array_equal(dq0, dq1) and np.array_equal(st0, st1)  # nothing was touched
    finally:
        ro.free()


def test_pairs_objects_keep_the_tableau_in_registers(built):
    """The rule of tests/test_abi.py::test_tableau_rows_stay_in_registers over the sphere-pair objects: a private segment
    beyond four bytes per spilled register stays under 128 bytes."""
    build = os.path.join(ROOT, "pink_amd", "csrc", "build")
    objs = sorted(glob.glob(os.path.join(build, "rpairs_*.o")))
    assert len(objs) == 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_meta.py")] + objs, capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-objdump / llvm-readelf not available: " + out.stderr[-200:])
    print(out.stdout)
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ik_rollout_pairs_kernel")]
    assert len(rows) == 3, out.stdout[-2000:]
    excess = lambda f: int(f[-2]) - 4 * int(f[-4])  # noqa: E731  (columns: ... vspill sspill scratch lds)
    worst = max(rows, key=excess)
    assert excess(worst) < 128, " ".join(worst)
