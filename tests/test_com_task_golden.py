"""pink_amd.build_ik with a ComTask against the reference's own pink.build_ik (tests/golden/com_task.npz, written by
tests/golden/make_golden_com.py): [2 FrameTasks + ComTask (vector cost, gain 0.7, lm_damping 1e-3) + PostureTask] on the
arm and on the tree, P and q to the 1e-13 of the other fixtures."""
import os

import numpy as np
import pytest

from pink_amd import ComTask, Configuration, FrameTask, PostureTask, build_ik
from pink_amd.lie import SE3
from pink_amd.limits import ConfigurationLimit, VelocityLimit
from pink_amd.runtime import set_default_solver
from tests.com_task_cases import ROOT, models


@pytest.fixture(scope="module")
def com_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "com_task.npz"))


@pytest.mark.parametrize("case, frames", [("arm6", ["tool0", "joint_3"]), ("tree12", ["hand", "foot"])])
def test_build_ik_matches_the_reference(emu, com_golden, case, frames):
    g = com_golden
    m = models()[case][0]
    mass, com_tab = m.mass_tables()
    assert np.array_equal(mass, g[f"{case}/mass"]) and np.array_equal(com_tab, g[f"{case}/com"])  # the fixture's model
    cfg = Configuration(m, g[f"{case}/q"])
    tasks = []
    for k, (pc, oc, lm, gain) in enumerate(((1.0, 0.5, 1e-3, 0.9), ([1.0, 2.0, 0.5], 0.0, 0.0, 0.85))):
        t = FrameTask(frames[k], pc, oc, lm_damping=lm, gain=gain)
        p = g[f"{case}/target{k}"]
        t.set_target(SE3(p[:9].reshape(3, 3), p[9:]))
        tasks.append(t)
    com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
    com.set_target(g[f"{case}/com_target"])
    po = PostureTask(cost=5e-2, gain=0.8)
    po.set_target(g[f"{case}/q_star"])
    assert np.abs(com.compute_error(cfg) - g[f"{case}/com_e"]).max() <= 1e-15
    assert np.abs(com.compute_jacobian(cfg) - g[f"{case}/com_J"]).max() <= 1e-15
    set_default_solver(emu)
    try:
        problem = build_ik(cfg, tasks + [com, po], float(g[f"{case}/dt"]), damping=1e-12, limits=[ConfigurationLimit(m), VelocityLimit(m)])
        P, c = problem.P, problem.q
    finally:
        set_default_solver(None)
    assert np.abs(P - g[f"{case}/P"]).max() <= 1e-13 * max(1.0, np.abs(g[f"{case}/P"]).max())
    assert np.abs(c - g[f"{case}/c"]).max() <= 1e-13 * max(1.0, np.abs(g[f"{case}/c"]).max())
    # the ComTask's share is in there: without it the objective differs
    problem0 = build_ik(cfg, tasks + [po], float(g[f"{case}/dt"]), damping=1e-12, limits=[ConfigurationLimit(m), VelocityLimit(m)])
    set_default_solver(emu)
    try:
        assert np.abs(problem0.q - g[f"{case}/c"]).max() > 1e-6
    finally:
        set_default_solver(None)
