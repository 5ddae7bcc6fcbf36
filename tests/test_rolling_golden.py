"""The host RollingTask / OmniwheelTask and pink_amd.build_ik against the reference's own classes and pink.build_ik
(tests/golden/rolling_task.npz, written by tests/golden/make_golden_rolling.py): e, J and the P, q of [two FrameTasks + the
wheels + PostureTask] with cost vectors, gain 0.7 and lm_damping 1e-3, on the biped and on tree34 -- whose second floor
hangs on a moving joint -- to 1e-13 max|value| (the bar of tests/test_com_task_golden.py)."""
import os

import numpy as np
import pytest

from pink_amd import Configuration, FrameTask, OmniwheelTask, PostureTask, RollingTask, build_ik
from pink_amd.lie import SE3
from pink_amd.limits import ConfigurationLimit, VelocityLimit
from pink_amd.runtime import set_default_solver
from tests.rolling_cases import OMNI, ROOT, arrays, models

FRAME_TASKS = {"biped": ("base", "right_hub"), "tree34": ("hand", "foot")}
COSTS = {0: [1.0, 0.5, 2.0], 1: [0.8, 1.5]}
TOL = 1e-13


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rolling_task.npz"))


def _wheels(name):
    return [(OmniwheelTask if k == OMNI else RollingTask)(hub, floor, r, cost=np.array(COSTS[k]), gain=0.7, lm_damping=1e-3)
            for k, hub, floor, r in models()[name][1]]


def test_the_fixture_has_a_floor_on_a_moving_joint(golden):
    arr = arrays("tree34")
    assert int(arr.frame_root_joint[1]) > 0 and int(arr.frame_root_joint[0]) == -1
    # ... and that floor's ancestors own no column in the reference's rows
    model = models()["tree34"][0]
    anc, k = set(), int(arr.frame_joint[1])
    while k >= 0:
        anc.add(k)
        k = model.joints[k].parent
    deck = model.joints[int(arr.frame_root_joint[1])]
    assert int(arr.frame_root_joint[1]) not in anc and (golden["tree34/J"][2:, deck.idx_v] == 0.0).all()
    assert all(np.isfinite(golden[k]).all() and golden[k].dtype.kind in "fiu" for k in golden.files)  # numeric arrays only


@pytest.mark.parametrize("name", ["biped", "tree34"])
def test_classes_match_the_reference_on_the_anchor_configurations(golden, name):
    model = models()[name][0]
    ts = _wheels(name)
    for q, e_ref, J_ref in zip(golden[f"{name}/anchor_q"], golden[f"{name}/anchor_e"], golden[f"{name}/anchor_J"]):
        cfg = Configuration(model, q)
        e = np.concatenate([t.compute_error(cfg) for t in ts])
        J = np.vstack([t.compute_jacobian(cfg) for t in ts])
        assert e.shape == e_ref.shape and J.shape == J_ref.shape
        assert np.abs(e - e_ref).max() <= TOL * np.abs(e_ref).max() and np.abs(J - J_ref).max() <= TOL * np.abs(J_ref).max()
        assert np.array_equal(J == 0.0, J_ref == 0.0)  # the same exact zeros


@pytest.mark.parametrize("name", ["biped", "tree34"])
def test_class_and_build_ik_match_the_reference(emu, golden, name):
    g = golden
    model = models()[name][0]
    cfg = Configuration(model, g[f"{name}/q"])
    ts = _wheels(name)
    e = np.concatenate([t.compute_error(cfg) for t in ts])
    J = np.vstack([t.compute_jacobian(cfg) for t in ts])
    assert np.abs(e - g[f"{name}/e"]).max() <= TOL * np.abs(g[f"{name}/e"]).max()
    assert np.abs(J - g[f"{name}/J"]).max() <= TOL * np.abs(g[f"{name}/J"]).max()
    fts = []
    for i, (frame, p) in enumerate(zip(FRAME_TASKS[name], g[f"{name}/targets"])):
        ft = FrameTask(frame, 1.0 + i, 0.5, lm_damping=1e-3, gain=0.9)
        ft.set_target(SE3(p[:9].reshape(3, 3), p[9:]))
        fts.append(ft)
    po = PostureTask(cost=5e-2, gain=0.8)
    po.set_target(g[f"{name}/q_star"])
    set_default_solver(emu)
    try:
        limits = [ConfigurationLimit(model), VelocityLimit(model)]
        problem = build_ik(cfg, fts + ts + [po], float(g[f"{name}/dt"]), damping=1e-12, limits=limits)
        problem0 = build_ik(cfg, fts + [po], float(g[f"{name}/dt"]), damping=1e-12, limits=limits)
        P, c, c0 = problem.P, problem.q, problem0.q  # (stacked by the solver on first access)
    finally:
        set_default_solver(None)
    assert np.abs(P - g[f"{name}/P"]).max() <= TOL * np.abs(g[f"{name}/P"]).max()
    assert np.abs(c - g[f"{name}/c"]).max() <= TOL * np.abs(g[f"{name}/c"]).max()
    assert np.abs(c0 - g[f"{name}/c"]).max() > 1e-6  # the wheels' share is in there
