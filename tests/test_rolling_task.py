"""RollingTask / OmniwheelTask on the host: the classes and the batched evaluator against 60-digit rows
(tests/rolling_cases.py builds them), the exact structure of the rows, that every term of the geometry is worth far more
than the bar on the cases, the reference's own unit tests restated, and the tasks inside solve_ik."""
import numpy as np
import pytest

import pink_amd
from pink_amd import Configuration, FrameTask, OmniwheelTask, PostureTask, RollingTask, solve_ik
from pink_amd import batch_eval as be
from pink_amd.exceptions import FrameNotFound
from pink_amd.kinematics_batch import BatchKinematics
from pink_amd.runtime import set_default_solver
from tests.rolling_cases import (arrays, configurations, models, note_ratios, reference, reference_bar, tasks_of,
                                 term_moves, worst, write_ratios)

NAMES = ["cart", "biped", "quad", "tree34", "chain8", "chain32"]


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_ROLLING_TASK_RATIOS=<file>: the worst ratios of this run as JSON (profiles/rolling_task_exact.json)


def host_rows(name, q):
    """(e [B, nr], J [B, nr, nv], z [B, n]) of the host classes, one Configuration per instance."""
    model, wheels = models()[name]
    ts = tasks_of(name)
    e, J, z = [], [], []
    for qb in q:
        cfg = Configuration(model, qb)
        e.append(np.concatenate([t.compute_error(cfg) for t in ts]))
        J.append(np.vstack([t.compute_jacobian(cfg) for t in ts]))
        z.append([t.compute_error(cfg)[-1] + t.wheel_radius for t in ts])
    return np.array(e), np.array(J), np.array(z)


@pytest.mark.parametrize("name", NAMES)
def test_host_rows_against_60_digits(name):
    """e and J of the classes, and of the batched evaluator, within the bar of u = S + eps max|exact|."""
    model, wheels = models()[name]
    q, _ = reference(name)
    bar_e, bar_j = reference_bar(name)
    e, J, z = host_rows(name, q)
    re, rj, rz = worst(name, e, J)
    print(f"host {name:7s} e {re:.3g} J {rj:.3g} (bars {bar_e:.3g} {bar_j:.3g})")
    note_ratios("host", name, re, rj)
    assert re <= bar_e and rj <= bar_j, (re, rj)
    kin = BatchKinematics(model, q)
    terms = [be.task_term(kin, [t] * q.shape[0]) for t in tasks_of(name)]
    eb, Jb = np.concatenate([t.e for t in terms], axis=1), np.concatenate([t.J for t in terms], axis=1)
    re, rj, _ = worst(name, eb, Jb)
    note_ratios("host_batched", name, re, rj)
    assert re <= bar_e and rj <= bar_j, (re, rj)


@pytest.mark.parametrize("name", NAMES)
def test_exact_structure_of_the_host_rows(name):
    """Off-path columns are exactly zero, the first error entry is zero for both kinds and the second for Rolling, and the
    Omniwheel rows are bit-equal to rows 0 and 2 of a Rolling wheel with the same frames and radius."""
    model, wheels = models()[name]
    arr = arrays(name)
    q = configurations(name)
    for w, (kind, hub, floor, r) in enumerate(wheels):
        path = set()
        k = int(arr.frame_joint[w])
        while k >= 0:
            path.add(k)
            k = model.joints[k].parent
        off = [c for k, j in enumerate(model.joints) if k not in path for c in range(j.idx_v, j.idx_v + j.nv)]
        on = [c for k, j in enumerate(model.joints) if k in path for c in range(j.idx_v, j.idx_v + j.nv)]
        roll, omni = RollingTask(hub, floor, r, 1.0), OmniwheelTask(hub, floor, r, 1.0)
        for qb in q:
            cfg = Configuration(model, qb)
            J3, e3 = roll.compute_jacobian(cfg), roll.compute_error(cfg)
            assert J3.shape == (3, model.nv) and (J3[:, off] == 0.0).all() and (np.abs(J3[:, on]).max(axis=0) > 0.0).all()
            assert e3[0] == 0.0 and e3[1] == 0.0 and e3[2] != 0.0
            J2, e2 = omni.compute_jacobian(cfg), omni.compute_error(cfg)
            assert J2.tobytes() == J3[[0, 2]].tobytes() and e2.tobytes() == e3[[0, 2]].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_every_term_is_worth_100_bars(name):
    """The magnitudes of the cases are a condition: dropping any one term of the rows -- rho in the contact point, R_F^T, the
    path mask, the Omniwheel's row choice, the sign of rho, the zero columns of the floor's ancestors -- moves the 60-digit
    rows by at least 100 bars on every instance of every model the term applies to.  No kernel takes part."""
    moves = term_moves(name)
    print(name, {k: "%.3g" % v for k, v in moves.items()})
    assert {"pc_is_ph", "no_RF", "rho_sign"} <= set(moves)
    assert ("no_mask" in moves) == (name != "cart") and ("omni_01" in moves) == (name != "cart")
    assert ("floor_ancestors" in moves) == (name == "tree34")
    assert all(v >= 100.0 for v in moves.values()), moves


def test_every_term_is_covered_by_some_model():
    assert set().union(*(set(term_moves(n)) for n in NAMES)) == {"pc_is_ph", "no_RF", "no_mask", "omni_01", "rho_sign", "floor_ancestors"}


# ---- the surface of the classes ---------------------------------------------------------------------------------------------
def test_exports_attributes_and_repr():
    assert pink_amd.RollingTask is RollingTask and pink_amd.tasks.OmniwheelTask is OmniwheelTask
    assert issubclass(OmniwheelTask, RollingTask)
    t = RollingTask("hub", "floor", 0.12, cost=[1.0, 2.0, 3.0], gain=0.7, lm_damping=1e-3)
    assert (t.hub_frame, t.floor_frame, t.wheel_radius, t.gain, t.lm_damping) == ("hub", "floor", 0.12, 0.7, 1e-3)
    assert repr(t) == "RollingTask(hub_frame=hub, floor_frame=floor, wheel_radius=0.12, cost=[1.0, 2.0, 3.0], gain=0.7, lm_damping=0.001)"
    o = OmniwheelTask("hub", "floor", 0.12, cost=1.0)
    assert repr(o) == "OmniwheelTask(hub_frame=hub, floor_frame=floor, wheel_radius=0.12, cost=1.0, gain=1.0, lm_damping=0.0)"


def test_unknown_frames_raise_what_a_frame_task_raises():
    model, _ = models()["cart"]
    cfg = Configuration(model, model.neutral())
    ft = FrameTask("nope", 1.0, 1.0)
    ft.set_target(pink_amd.lie.SE3())
    with pytest.raises(FrameNotFound):
        ft.compute_error(cfg)
    for t in (RollingTask("nope", "floor", 0.1, 1.0), RollingTask("hub", "nope", 0.1, 1.0), OmniwheelTask("nope", "floor", 0.1, 1.0)):
        with pytest.raises(FrameNotFound):
            t.compute_error(cfg)
        with pytest.raises(FrameNotFound):
            t.compute_jacobian(cfg)


def test_the_reference_unit_tests_restated():
    """tests/test_rolling_task.py and tests/test_omniwheel_task.py of the reference, on the biped: the in-plane error entries
    are zero, the Jacobians have three and two rows."""
    model, _ = models()["biped"]
    cfg = Configuration(model, configurations("biped")[0])
    roll = RollingTask("left_hub", floor_frame="world", wheel_radius=0.1, cost=1.0)
    assert np.linalg.norm(roll.compute_error(cfg)[:2]) == 0.0
    assert roll.compute_jacobian(cfg).shape == (3, model.nv)
    omni = OmniwheelTask("left_hub", floor_frame="world", wheel_radius=0.1, cost=1.0)
    assert omni.compute_error(cfg)[0] == 0.0
    assert omni.compute_jacobian(cfg).shape == (2, model.nv)


def test_the_jacobian_is_the_derivative_of_the_contact_point():
    """Central differences of the contact point (held in the hub's body, floor inertial) along q (+) h e_j."""
    model, wheels = models()["biped"]
    q = configurations("biped")[1]
    cfg = Configuration(model, q)
    for kind, hub, floor, r in wheels:
        T_F, T_H = cfg.get_transform_frame_to_world(floor), cfg.get_transform_frame_to_world(hub)
        c_in_hub = T_H.inverse().act(T_H.translation - r * T_F.rotation[:, 2])
        J = RollingTask(hub, floor, r, 1.0).compute_jacobian(cfg)
        h = 1e-6
        for j in range(model.nv):
            v = np.zeros(model.nv)
            v[j] = h
            p = [Configuration(model, model.integrate(q, s * v)).get_transform_frame_to_world(hub).act(c_in_hub) for s in (1, -1)]
            assert np.abs(T_F.rotation.T @ (p[0] - p[1]) / (2 * h) - J[:, j]).max() < 1e-8


def test_uniform_slot_rule():
    a, b = RollingTask("hub", "floor", 0.1, 1.0), RollingTask("hub", "floor", 0.1, 1.0)
    assert be.rolling_slot_is_uniform([a, a]) and be.rolling_slot_is_uniform([a, b], with_weights=True)
    assert not be.rolling_slot_is_uniform([a, RollingTask("hub", "floor", 0.2, 1.0)])
    assert not be.rolling_slot_is_uniform([a, RollingTask("hub", "other", 0.1, 1.0)])
    assert not be.rolling_slot_is_uniform([a, OmniwheelTask("hub", "floor", 0.1, 1.0)])
    assert be.rolling_slot_is_uniform([a, RollingTask("hub", "floor", 0.1, 2.0)])
    assert not be.rolling_slot_is_uniform([a, RollingTask("hub", "floor", 0.1, 2.0)], with_weights=True)
    assert not be.rolling_slot_is_uniform([a, RollingTask("hub", "floor", 0.1, 1.0, gain=0.5)], with_weights=True)


def test_per_instance_radii_on_the_batched_evaluator():
    model, wheels = models()["biped"]
    q = configurations("biped")
    col = [OmniwheelTask("right_hub", "ramp", 0.07 if b % 2 else 0.11, 1.0) for b in range(q.shape[0])]
    term = be.task_term(BatchKinematics(model, q), col)
    for b, t in enumerate(col):
        cfg = Configuration(model, q[b])
        assert np.allclose(term.e[b], t.compute_error(cfg), rtol=0, atol=1e-14) and np.allclose(term.J[b], t.compute_jacobian(cfg), rtol=0, atol=1e-14)


# ---- inside the solver ------------------------------------------------------------------------------------------------------
def _biped_stack(cost=1.0):
    model, wheels = models()["biped"]
    base = FrameTask("base", position_cost=1.0, orientation_cost=1.0, lm_damping=1e-3)
    posture = PostureTask(cost=1e-2)
    return model, base, tasks_of("biped", cost=cost), posture


def test_solve_ik_returns_the_oracle_minimiser(emu):
    """solve_ik on one Configuration with a RollingTask and an OmniwheelTask in the stack: the minimiser of the QP the oracle
    builds from the same rows."""
    from oracle import pink_oracle

    model, base, wheels, posture = _biped_stack(cost=[1.0, 0.5, 2.0])
    wheels[1].cost = [0.8, 1.5]
    q = configurations("biped")[2]
    cfg = Configuration(model, q)
    base.set_target(cfg.get_transform_frame_to_world("base") * pink_amd.lie.exp6(0.05 * np.arange(1.0, 7.0) / 6.0))
    posture.set_target(model.neutral())
    tasks = [base] + wheels + [posture]
    set_default_solver(emu)
    try:
        v = solve_ik(cfg, tasks, dt=1e-2, damping=1e-8, limits=[])
        problem = pink_amd.build_ik(cfg, tasks, 1e-2, damping=1e-8, limits=[])
        P, c = np.array(problem.P), np.array(problem.q)
    finally:
        set_default_solver(None)
    rows = [(t.compute_jacobian(cfg), t.compute_error(cfg), t.cost, t.gain, t.lm_damping) for t in tasks]
    res, (H, g, _, _) = pink_oracle.solve_ik_instance(model.nv, rows, 1e-2, damping=1e-8)
    assert np.abs(P - H).max() <= 1e-12 * np.abs(H).max() and np.abs(c - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(v * 1e-2 - res.x).max() <= 1e-8 * max(1.0, np.abs(res.x).max())


def test_ten_steps_bring_the_wheels_to_the_floor(emu):
    """Host loop on the biped: both hubs start 2 cm above their floors' planes at height rho, and |z - rho| shrinks
    monotonically over ten steps."""
    model, base, wheels, posture = _biped_stack()
    for t in wheels:
        t.gain = 0.5
    q = configurations("biped")[3].copy()
    cfg = Configuration(model, q)
    # radii chosen so that each hub is 2 cm too high at the start
    for t in wheels:
        t.wheel_radius = float(t.compute_error(cfg)[-1] + t.wheel_radius) - 0.02
    base.set_target(cfg.get_transform_frame_to_world("base"))
    base.cost = np.r_[1e-2 * np.ones(3), 1e-2 * np.ones(3)]
    posture.set_target(q)
    tasks = [base] + wheels + [posture]
    set_default_solver(emu)
    try:
        gaps = [[abs(t.compute_error(cfg)[-1]) for t in wheels]]
        for _ in range(10):
            v = solve_ik(cfg, tasks, dt=1e-2, damping=1e-10, limits=[])
            cfg.integrate_inplace(v, 1e-2)
            gaps.append([abs(t.compute_error(cfg)[-1]) for t in wheels])
    finally:
        set_default_solver(None)
    gaps = np.array(gaps)
    assert np.allclose(gaps[0], 0.02, atol=1e-12)
    assert (np.diff(gaps, axis=0) < 0.0).all(), gaps
    assert (gaps[-1] < 0.02 * 0.5 ** 9).all()
