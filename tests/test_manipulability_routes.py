"""ManipulabilityTask through solve_ik_batch: up to four slots beside FrameTasks take the hybrid route -- their rows are
formed on the device by pinkhip_manipulability_task_device behind the FrameTask and ComTask rows -- and agree with the
all-host evaluation to the 1e-10 tests/test_com_task_routes.py holds the ComTask to; what declines to the host route; and
that a positive rate raises the manipulability (the one behavioural check of the sign of e)."""
import numpy as np
import pytest

import pink_amd
from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, ManipulabilityTask, PostureTask, ReferenceFrame, solve_ik_batch
from pink_amd.exceptions import PinkError
from pink_amd.lie import exp6
from pink_amd.runtime import set_default_solver
from tests.manipulability_cases import cond_A, models
from tests.row_kernel_kit import with_row_kernels


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    s = with_row_kernels(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))
    set_default_solver(s)
    yield s
    pink_amd.clear_device_cache()
    set_default_solver(None)


def _stack(B, seed=3, with_com_task=False, n_manip=1):
    model, _ = models()["arm6"]  # (carries mass: a ComTask fits beside it)
    rng = np.random.default_rng(seed)
    specs = [dict(cost=0.8, gain=0.6, lm_damping=1e-3, manipulability_rate=0.2),
             dict(cost=0.3, mask="position", reference_frame=ReferenceFrame.WORLD, manipulability_rate=-0.1),
             dict(cost=0.5, mask="planar_xy"), dict(cost=0.2, mask=np.array([1.0, 0, 1, 0, 1, 1]), gain=0.4)]
    frames = ["tool0", "joint_5", "tool0", "joint_6"]
    # the regular band of tests/manipulability_cases.py: cond(A) <= 1e4 for every task of the stack, filtered before anything
    # is compared (the two routes form A in different orders: they differ by eps cond(A))
    q = rng.uniform(-1.0, 1.0, size=(16 * B, model.nq))
    ok = np.ones(len(q), bool)
    for i in range(n_manip):
        ok &= cond_A(model, frames[i], specs[i].get("reference_frame", ReferenceFrame.LOCAL), specs[i].get("mask"), q) <= 1e4
    q = q[ok][:B]
    assert q.shape[0] == B
    ft = FrameTask("tool0", 1.0, 0.5, lm_damping=1e-3, gain=0.9)
    R, t = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b in range(B):
        T = Configuration(model, q[b]).get_transform_frame_to_world("tool0") * exp6(0.05 * rng.normal(size=6))
        R[b], t[b] = T.rotation, T.translation
    ft.set_target_poses(R, t)
    tasks = [ft]
    if with_com_task:
        com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
        com.set_target(Configuration(model, q[0]).center_of_mass() + [0.01, -0.02, 0.03])
        tasks.append(com)
    tasks += [ManipulabilityTask(frames[i], model, **specs[i]) for i in range(n_manip)]
    po = PostureTask(cost=5e-2)
    po.set_target(model.neutral())
    return model, q, tasks + [po]


@pytest.mark.parametrize("B", [64, 200])
@pytest.mark.parametrize("with_com_task, n_manip", [(False, 1), (True, 1), (True, 4)])
def test_manipulability_tasks_take_the_hybrid_route(backend, B, with_com_task, n_manip):
    dt = 5e-3
    model, q, tasks = _stack(B, with_com_task=with_com_task, n_manip=n_manip)
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "hybrid" and stats["failed"] == 0 and stats["instances"] == B
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, device_kinematics=False)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated" and pink_amd.last_solve_stats()["failed"] == 0
    err = np.abs(V - V_host).max() * dt
    print(f"hybrid vs host-evaluated max|dq| difference {err:.3e}")
    assert err < 1e-10 and np.abs(V).max() * dt > 1e-4
    # the task's share is in there
    V0 = solve_ik_batch(ConfigurationBatch(model, q), [t for t in tasks if not isinstance(t, ManipulabilityTask)], dt)
    assert np.abs(V - V0).max() * dt > 1e-6


def test_what_declines_to_the_host_route(backend):
    B, dt = 64, 5e-3
    model, q, tasks = _stack(B)
    with pytest.raises(PinkError, match="ManipulabilityTask"):
        solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, strict_route="device")
    # five slots
    extra = [ManipulabilityTask("tool0", model, cost=0.1, manipulability_rate=0.01 * i) for i in range(4)]
    solve_ik_batch(ConfigurationBatch(model, q), tasks[:-1] + extra + tasks[-1:], dt)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated"
    # a solver without the call: the host route, the same velocities
    V1 = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    assert pink_amd.last_solve_stats()["route"] == "hybrid"
    pink_amd.clear_device_cache()
    set_default_solver(_Without(backend))
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated" and np.abs(V - V1).max() * dt < 1e-10


class _Without:
    """A solver whose library lacks pinkhip_manipulability_task_device."""

    def __init__(self, api):
        self._api = api

    def __getattr__(self, name):
        if name == "manipulability_task":
            raise AttributeError(name)
        return getattr(self._api, name)


def test_a_per_instance_list_that_differs_declines(backend):
    B, dt = 64, 5e-3
    model, q, tasks = _stack(B)
    per = []
    for b in range(B):
        mt = ManipulabilityTask("tool0", model, cost=0.8, gain=0.6, lm_damping=1e-3, manipulability_rate=0.2 if b != 5 else 0.3)
        per.append([tasks[0], mt, tasks[-1]])
    with pytest.raises(PinkError, match="ManipulabilityTask slot"):  # (the host route refuses the slot as it does frame slots)
        solve_ik_batch(ConfigurationBatch(model, q), per, dt)
    for b in range(B):  # ... and one that differs in nothing but the objects is served
        per[b][1] = ManipulabilityTask("tool0", model, cost=0.8, gain=0.6, lm_damping=1e-3, manipulability_rate=0.2)
    V = solve_ik_batch(ConfigurationBatch(model, q), per, dt)
    assert pink_amd.last_solve_stats()["route"] == "hybrid"
    assert np.abs(V - solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)).max() * dt < 1e-12


def test_a_positive_rate_raises_the_manipulability(backend):
    """The task alone with a small posture cost, five steps of the hybrid route: m rises with every step for every robot."""
    B, dt = 64, 1e-2
    model, _ = models()["arm6"]
    rng = np.random.default_rng(11)
    q = rng.uniform(-1.0, 1.0, size=(B, model.nq))
    mt = ManipulabilityTask("tool0", model, cost=1.0, manipulability_rate=0.5)
    ft = FrameTask("tool0", 0.0, 0.0)  # (a weightless FrameTask: the hybrid route is chosen by its presence)
    ft.set_target(Configuration(model, q[0]).get_transform_frame_to_world("tool0"))
    po = PostureTask(cost=1e-3)
    po.set_target(model.neutral())
    ms = []
    for _ in range(6):
        cfgs = [Configuration(model, q[b]) for b in range(B)]
        ms.append([mt.compute_manipulability(c) for c in cfgs])
        V = solve_ik_batch(ConfigurationBatch(model, q), [ft, mt, po], dt)
        assert pink_amd.last_solve_stats()["route"] == "hybrid"
        q = q + V * dt
    ms = np.array(ms)
    assert (np.diff(ms, axis=0) > 0.0).all(), np.diff(ms, axis=0).min()


# ---- closed loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_manip", [1, 2])
def test_closed_loop_with_manipulability_tasks_matches_the_host_loop(backend, n_manip):
    """DeviceRollout(manipulability_tasks=...), five steps: step kernel -> manipulability kernel(s) -> solve (fused=True)
    agrees with the five-launch step (fused=False) to the 1e-11 of tests/test_com_task_routes.py and follows the host loop
    of solve_ik + integrate to its 1e-8; the whole-step kernel is refused."""
    from pink_amd import solve_ik
    from pink_amd.rollout import DeviceRollout, pose12

    api = backend
    B, dt, steps = 5, 5e-3, 5
    model, q0, _ = _stack(B, seed=9, n_manip=2)
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    specs = [("tool0", 0.2, 0.1, 1.0, 1e-3)]
    targets = np.array([[pose12(c.get_transform_frame_to_world("tool0"))] for c in cfgs])
    mts = [ManipulabilityTask("tool0", model, cost=0.8, gain=0.6, lm_damping=1e-3, manipulability_rate=0.2),
           ManipulabilityTask("joint_5", model, cost=0.3, mask="position", reference_frame=ReferenceFrame.WORLD, manipulability_rate=-0.1)][:n_manip]
    with pytest.raises(ValueError, match="whole-step kernel does not form manipulability rows"):
        DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused="kernel", manipulability_tasks=mts)
    runs = {}
    for fused in (True, False):
        ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused=fused, manipulability_tasks=mts)
        ro.set_targets(targets)
        m0 = ro.manipulability()
        assert m0.shape == (n_manip, B)
        assert np.abs(m0[0] - [mts[0].compute_manipulability(c) for c in cfgs]).max() < 1e-12
        traj = []
        for _ in range(steps):
            ro.step()
            traj.append(ro.configurations())
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        ro.free()
        runs[fused] = np.array(traj)
    assert np.abs(runs[True] - runs[False]).max() < 1e-11
    assert np.abs(runs[True][-1] - q0).max() > 1e-5  # (the robots moved)
    for b, cfg in enumerate(cfgs):
        ft = FrameTask("tool0", 0.2, 0.1, lm_damping=1e-3, gain=1.0)
        ft.set_target(cfg.get_transform_frame_to_world("tool0"))
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        for k in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, [ft] + mts + [p], dt), dt)
            assert np.abs(runs[True][k, b] - cfg.q).max() < 1e-8, (b, k)
