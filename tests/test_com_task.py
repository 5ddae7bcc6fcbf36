"""ComTask on the host: the model's masses (``Joint.mass`` / ``Joint.com``, ``load_urdf``'s ``<inertial>``), the centre of mass
and its Jacobian of ``Configuration`` and ``BatchKinematics`` against 60-digit values, and the task class's behaviour
(``pink/tasks/com_task.py``; the reference's ``tests/test_com_task.py`` restated).  Models and reference:
tests/com_task_cases.py."""
import os

import mpmath as mp
import numpy as np
import pytest

from oracle import exact_kinematics as ek
from pink_amd import ComTask, Configuration, build_chain, build_ik, load_urdf
from pink_amd.configuration import Model
from pink_amd.exceptions import TargetNotSet, TaskDefinitionError
from pink_amd.kinematics_batch import BatchKinematics
from pink_amd.lie import SE3
from pink_amd.rollout import ModelArrays
from tests.com_task_cases import H_FD, K_COM, ROOT, configurations, models, moved, note_ratios, reference, worst, write_ratios


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_COM_TASK_RATIOS=<file>: the host path's worst ratios (profiles/com_task_exact.json)


# ---- 0. the model ---------------------------------------------------------------------------------------------------------
def test_models_are_what_the_device_tests_need():
    m = models()
    assert len(m["arm6"][0].joints) == 6 and len(m["tree12"][0].joints) == 12 and len(m["tree34"][0].joints) == 34
    t = m["tree12"][0]
    assert [j.name for j in t.joints if j.mass == 0.0] == ["joint_3", "joint_10"]
    assert abs(t.joints[8].mass / t.total_mass - 0.8) < 1e-12 and not any(j.parent == 8 for j in t.joints)
    assert sum(j.kind == "prismatic" for j in t.joints) == 1
    assert m["tree34"][0].nv == 39 and m["tree34"][0].joints[0].kind == "free_flyer"
    for n in (8, 32):  # the chains: serial (depth = nj = the group width), all revolute, every joint with a mass
        c = m[f"chain{n}"][0]
        assert [j.parent for j in c.joints] == list(range(-1, n - 1)) and all(j.kind == "revolute" and j.mass > 0.0 for j in c.joints)


def test_default_models_stay_massless():
    a, b = build_chain(6), build_chain(6, mass_seed=3)
    assert a.total_mass == 0.0 and all(j.mass == 0.0 and not j.com.any() for j in a.joints)
    assert b.total_mass > 0.0
    for ja, jb in zip(a.joints, b.joints):  # the mass draw has a generator of its own: the kinematics are bit-identical
        assert np.array_equal(ja.axis, jb.axis) and np.array_equal(ja.placement.translation, jb.placement.translation)
    with pytest.raises(ValueError):
        Configuration(a, a.neutral()).center_of_mass()
    with pytest.raises(ValueError):
        Model().add_joint("j", "revolute", -1, SE3(), [0, 0, 1], mass=-1.0)


def test_load_urdf_reads_inertial_blocks():
    m = models()["pend"][0]
    assert [j.mass for j in m.joints] == [0.2, 0.3]  # the base link's 0.1 is fixed to the world: it does not count
    assert np.allclose(m.joints[0].com, [0, 0, 0.05]) and np.allclose(m.joints[1].com, [0, 0, 0.1])
    assert m.total_mass == 0.5
    mf = load_urdf(os.path.join(ROOT, "tests", "golden", "double_pendulum.urdf"), free_flyer=True)
    assert abs(mf.total_mass - 0.6) < 1e-15 and mf.joints[0].mass == 0.1


_FIXED_URDF = """<robot name="r">
 <link name="base"><inertial><mass value="7"/><origin xyz="1 1 1"/></inertial></link>
 <link name="arm"><inertial><mass value="1"/><origin xyz="0.1 0 0" rpy="0.3 0 0"/></inertial></link>
 <link name="tool"><inertial><mass value="3"/><origin xyz="0 0.2 0"/></inertial></link>
 <link name="tip"><inertial><mass value="2"/><origin xyz="0 0 0.5"/></inertial></link>
 <joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 1"/><axis xyz="0 0 1"/>
  <limit lower="-1" upper="1" velocity="1"/></joint>
 <joint name="f1" type="fixed"><parent link="arm"/><child link="tool"/><origin xyz="1 0 0" rpy="0 0 1.5707963267948966"/></joint>
 <joint name="f2" type="fixed"><parent link="tool"/><child link="tip"/><origin xyz="0 0 1"/></joint>
</robot>"""


def test_load_urdf_folds_links_behind_fixed_joints_into_their_moving_parent(tmp_path):
    path = tmp_path / "fixed.urdf"
    path.write_text(_FIXED_URDF)
    m = load_urdf(str(path))
    assert len(m.joints) == 1 and m.total_mass == 6.0
    # arm at (0.1, 0, 0); tool frame at (1, 0, 0) turned a quarter about z: its (0, 0.2, 0) is (-0.2, 0, 0) + (1, 0, 0);
    # tip one up from the tool: (1, 0, 1) + (0, 0, 0.5)
    want = (1 * np.array([0.1, 0, 0]) + 3 * np.array([0.8, 0, 0]) + 2 * np.array([1.0, 0, 1.5])) / 6.0
    assert np.allclose(m.joints[0].com, want, atol=1e-15)
    c = Configuration(m, np.array([0.0])).center_of_mass()
    assert np.allclose(c, want + [0, 0, 1], atol=1e-15)


# ---- 1. exact anchor, host ------------------------------------------------------------------------------------------------
def test_the_moved_joint_follows_exact_kinematics_integrate():
    model, frames = models()["tree34"]
    arr = ModelArrays(model, frames)
    q = configurations("tree34")[0]
    with mp.workdps(ek.DPS):
        for k, sub in ((0, 4), (5, 0)):
            v = np.zeros(model.nv)
            v[model.joints[k].idx_v + sub] = H_FD
            want = ek.integrate(arr, q, v)[k]
            jt, iq = int(arr.jtype[k]), int(arr.idx_q[k])
            base = ek.joint_matrix(jt, arr.axis[k], q[iq:iq + (7 if jt == ek.FREE_FLYER else 1)])
            got = moved(arr, base, k, sub, mp.mpf(H_FD))
            assert max(abs(a - b) for a, b in zip(ek.flat(want), ek.flat(got))) < mp.mpf(10) ** -55


@pytest.mark.parametrize("name", ["arm6", "tree12", "tree34", "pend", "chain8", "chain32"])
def test_host_centre_of_mass_and_jacobian_against_60_digits(name):
    model, _ = models()[name]
    q, _ = reference(name)
    kin = BatchKinematics(model, q)
    cb, Jb = kin.center_of_mass(), kin.jacobian_center_of_mass()
    cs = np.array([Configuration(model, q[b]).center_of_mass() for b in range(q.shape[0])])
    Js = np.array([Configuration(model, q[b]).jacobian_center_of_mass() for b in range(q.shape[0])])
    for who, (c, J) in {"configuration": (cs, Js), "batch": (cb, Jb)}.items():
        rc, rj = worst(name, c, J)
        print(f"host {who:13s} {name:7s} com {rc:.3g} J {rj:.3g}")
        note_ratios("host", name, rc, rj)
        assert rc <= K_COM and rj <= K_COM, (who, rc, rj)
    assert np.abs(Js - Jb).max() <= 1e-13 and np.abs(cs - cb).max() <= 1e-13
    task = ComTask(1.0)
    task.set_target(np.zeros(3))
    assert np.abs(task.compute_jacobian(Configuration(model, q[0])) - Jb[0]).max() <= 1e-13
    # structure: a joint in front of massless leaves only ... and a column of the prismatic joint is its axis, scaled
    if name == "tree12":
        j = model.joints[3]
        sub, _ = model.subtree_tables()
        assert np.allclose(Jb[:, :, j.idx_v], kin._axes_world()[:, 3] * sub[3] / model.total_mass, atol=1e-15)


# ---- 4. class behaviour ---------------------------------------------------------------------------------------------------
def _cfg(name="tree12"):
    return Configuration(models()[name][0], configurations(name)[0])


def test_target_not_set_is_raised_before_a_target():
    task, cfg = ComTask(1.0), _cfg()
    with pytest.raises(TargetNotSet):
        task.compute_error(cfg)
    with pytest.raises(TargetNotSet):
        task.compute_jacobian(cfg)


def test_set_target_copies():
    task = ComTask(1.0)
    t = np.array([0.1, 0.2, 0.3])
    task.set_target(t)
    t[0] = 9.0
    assert task.target_com[0] == 0.1
    with pytest.raises(TaskDefinitionError):
        task.set_target(np.zeros(4))


def test_error_is_zero_at_the_own_configuration_and_actual_minus_target_elsewhere():
    task, cfg = ComTask(1.0), _cfg()
    task.set_target_from_configuration(cfg)
    assert np.array_equal(task.compute_error(cfg), np.zeros(3))
    task.set_target(cfg.center_of_mass() - [0.0, 0.0, 0.25])
    assert np.allclose(task.compute_error(cfg), [0.0, 0.0, 0.25], atol=1e-15)
    assert task.compute_jacobian(cfg).shape == (3, cfg.model.nv)


def test_costs():
    task = ComTask(2.0)
    assert np.array_equal(task.cost, [2.0, 2.0, 2.0])
    task.set_cost([1.0, 0.0, 3.0])
    assert np.array_equal(task.cost, [1.0, 0.0, 3.0])
    for bad in (-1.0, [1.0, -2.0, 1.0], [1.0, 2.0]):
        with pytest.raises(TaskDefinitionError):
            task.set_cost(bad)
    with pytest.raises(TaskDefinitionError):
        ComTask([1.0, 1.0, -1.0])
    r = repr(ComTask([1.0, 2.0, 3.0], lm_damping=0.5, gain=0.7))
    assert r.startswith("ComTask(") and "gain=0.7" in r and "lm_damping=0.5" in r and "target_com=None" in r


def test_the_jacobian_is_the_derivative_of_the_centre():
    for name in ("tree12", "tree34"):
        cfg = _cfg(name)
        J = cfg.jacobian_center_of_mass()
        h = 1e-6
        for j in range(cfg.model.nv):
            v = np.zeros(cfg.model.nv)
            v[j] = h
            cp = Configuration(cfg.model, cfg.model.integrate(cfg.q, v)).center_of_mass()
            cm = Configuration(cfg.model, cfg.model.integrate(cfg.q, -v)).center_of_mass()
            assert np.abs((cp - cm) / (2 * h) - J[:, j]).max() < 1e-8, (name, j)


def test_objective_through_build_ik(emu):
    """H = J^T W^2 J and c = -(W (-gain e))^T W J = gain J^T W^2 e of the one task, e = actual - target
    (pink/tasks/task.py:145-167): the minimiser of the objective, -H^+ c, moves the centre TOWARDS its target."""
    from pink_amd.runtime import set_default_solver

    set_default_solver(emu)
    try:
        cfg = _cfg()
        task = ComTask([1.0, 2.0, 0.5], gain=0.7)
        task.set_target(cfg.center_of_mass() + [0.02, -0.01, 0.03])
        problem = build_ik(cfg, [task], dt=0.01, damping=0.0, limits=[])
        H, c = problem.P, problem.q
        J, e, W = task.compute_jacobian(cfg), task.compute_error(cfg), np.diag(task.cost)
        assert np.abs(c - 0.7 * J.T @ W @ W @ e).max() < 1e-14
        assert np.abs(H - J.T @ W @ W @ J).max() < 1e-14
        dq = -np.linalg.pinv(H) @ c
        assert np.allclose(J @ dq, -0.7 * e, atol=1e-12)  # J dq = -gain e: first order, the error shrinks by the gain
    finally:
        set_default_solver(None)
