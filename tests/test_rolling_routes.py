"""RollingTask / OmniwheelTask through solve_ik_batch and DeviceRollout: the wheels beside a FrameTask take the hybrid route
-- their rows are formed on the device by pinkhip_rolling_tasks_device, all wheels in one launch, behind the FrameTask,
ComTask and ManipulabilityTask rows -- and agree with the all-host evaluation to the 1e-10 of tests/test_com_task_routes.py;
slots that differ per instance and stacks of nine wheels go to the host route; the closed loop's launch variants agree to
1e-11 and the whole-step kernel is refused."""
import numpy as np
import pytest

import pink_amd
from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, OmniwheelTask, PostureTask, RollingTask, solve_ik_batch
from pink_amd.exceptions import PinkError
from pink_amd.lie import exp6
from pink_amd.runtime import set_default_solver
from tests.rolling_cases import configurations, models, tasks_of
from tests.row_kernel_kit import with_row_kernels

B, DT = 11, 5e-3


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    s = with_row_kernels(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))
    set_default_solver(s)
    yield s
    pink_amd.clear_device_cache()
    set_default_solver(None)


def _stack(seed=3):
    """The biped inside its joint limits: a FrameTask on the base with per-instance targets, the two wheels with cost
    vectors, gain 0.7 and lm_damping 1e-3, a PostureTask."""
    model, _ = models()["biped"]
    rng = np.random.default_rng(seed)
    q = 0.15 * configurations("biped", B=B, seed=seed)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    cfgs = [Configuration(model, q[b]) for b in range(B)]
    base = FrameTask("base", 1.0, 0.5, lm_damping=1e-3, gain=0.9)
    R, t = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b, c in enumerate(cfgs):
        T = c.get_transform_frame_to_world("base") * exp6(0.05 * rng.normal(size=6))
        R[b], t[b] = T.rotation, T.translation
    base.set_target_poses(R, t)
    wheels = tasks_of("biped", gain=0.7, lm_damping=1e-3)
    wheels[0].cost, wheels[1].cost = [1.0, 0.5, 2.0], [0.8, 1.5]
    po = PostureTask(cost=5e-2)
    po.set_target(model.neutral())
    return model, q, cfgs, base, wheels, po


def _both_routes(model, q, tasks, want):
    # (below 64 instances solve_ik_batch takes the host route by default; device_kinematics="frame_rows" asks for the hybrid one)
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, DT, device_kinematics="frame_rows")
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == want, stats
    assert stats["failed"] == 0 and stats["instances"] == B
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, DT, device_kinematics=False)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated" and pink_amd.last_solve_stats()["failed"] == 0
    err = np.abs(V - V_host).max() * DT
    print(f"{want} vs all-host max|dq| difference {err:.3e}")
    assert err < 1e-10 and np.abs(V).max() * DT > 1e-4
    return V


def test_the_wheels_take_the_hybrid_route(api):
    """Base FrameTask + Rolling + Omniwheel + PostureTask, default limits, B = 11."""
    model, q, cfgs, base, wheels, po = _stack()
    V = _both_routes(model, q, [base] + wheels + [po], "hybrid")
    # ... and the wheels' share is in there
    V0 = solve_ik_batch(ConfigurationBatch(model, q), [base, po], DT)
    assert np.abs(V - V0).max() * DT > 1e-5


def test_per_instance_radii_go_to_the_host_route(api):
    model, q, cfgs, base, wheels, po = _stack()
    col = [RollingTask("left_hub", "world", 0.1 if b % 2 else 0.13, [1.0, 0.5, 2.0], gain=0.7, lm_damping=1e-3) for b in range(B)]
    V = _both_routes(model, q, [[base, col[b], wheels[1], po] for b in range(B)], "host-evaluated")
    # every instance against its own single-instance solve
    from pink_amd import solve_ik

    for b in (0, 1, B - 1):
        ft = FrameTask("base", 1.0, 0.5, lm_damping=1e-3, gain=0.9)
        p = base.poses12()[b]
        ft.set_target(pink_amd.lie.SE3(p[:9].reshape(3, 3), p[9:]))
        v = solve_ik(cfgs[b], [ft, col[b], wheels[1], po], DT)
        assert np.abs(v - V[b]).max() * DT < 1e-10


def test_nine_wheels_go_to_the_host_route(api):
    model, q, cfgs, base, wheels, po = _stack()
    nine = [(OmniwheelTask if i % 2 else RollingTask)("right_hub" if i % 3 else "left_hub", "ramp" if i % 2 else "world", 0.05 + 0.02 * i, 0.3,
                                                       gain=0.7) for i in range(9)]
    _both_routes(model, q, [base] + nine + [po], "host-evaluated")
    _both_routes(model, q, [base] + nine[:8] + [po], "hybrid")


def test_the_whole_step_route_declines_the_wheels(api):
    model, q, cfgs, base, wheels, po = _stack()
    with pytest.raises(PinkError):
        solve_ik_batch(ConfigurationBatch(model, q), [base] + wheels + [po], DT, strict_route="device")


def test_rows_in_the_order_frame_com_rolling(api):
    """A ComTask in the same stack, listed behind the wheels: the device stack puts frame, centre-of-mass, then wheel rows, and
    the result is the all-host one."""
    model, q, cfgs, base, wheels, po = _stack()
    rng = np.random.default_rng(5)
    for j in model.joints:
        j.mass, j.com = float(rng.uniform(0.5, 2.0)), 0.05 * rng.normal(size=3)
    try:
        com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
        com.set_target(np.mean([c.center_of_mass() for c in cfgs], axis=0) + [0.01, -0.02, 0.03])
        V = _both_routes(model, q, [wheels[0], base, wheels[1], com, po], "hybrid")
        V1 = solve_ik_batch(ConfigurationBatch(model, q), [base] + wheels + [po], DT, device_kinematics="frame_rows")
        assert np.abs(V - V1).max() * DT > 1e-6  # (the ComTask's share)
    finally:
        for j in model.joints:
            j.mass, j.com = 0.0, np.zeros(3)


def test_closed_loop_launch_variants_agree(api):
    """DeviceRollout(rolling_tasks=...): step kernel -> rolling kernel -> solve (fused=True) and the launch-per-stage step
    (fused=False) agree over three steps to 1e-11, follow the host loop of solve_ik + integrate to 1e-8, bring the hubs
    towards their floors, and the whole-step kernel is refused."""
    from pink_amd import solve_ik
    from pink_amd.rollout import DeviceRollout, pose12

    steps, Bl = 3, 5
    model, q, cfgs, base, wheels, po = _stack(seed=9)
    q0, cfgs = q[:Bl], cfgs[:Bl]
    for t in wheels:
        t.gain = 0.5
    specs = [("base", 0.2, 0.1, 1.0, 1e-3)]
    targets = np.array([[pose12(c.get_transform_frame_to_world("base"))] for c in cfgs])
    with pytest.raises(ValueError, match="whole-step kernel does not form wheel-contact rows"):
        DeviceRollout(api, model, q0, specs, DT, posture_cost=1e-2, fused="kernel", rolling_tasks=wheels)
    with pytest.raises(ValueError, match="at most eight"):
        DeviceRollout(api, model, q0, specs, DT, posture_cost=1e-2, fused=True, rolling_tasks=wheels * 5)
    runs = {}
    for fused in (True, False):
        ro = DeviceRollout(api, model, q0, specs, DT, posture_cost=1e-2, fused=fused, rolling_tasks=wheels)
        ro.set_targets(targets)
        z0 = ro.wheel_heights()
        want = np.array([[t.compute_error(c)[-1] + t.wheel_radius for t in wheels] for c in cfgs])
        assert np.abs(z0 - want).max() < 1e-13
        traj = []
        for _ in range(steps):
            ro.step()
            traj.append(ro.configurations())
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        gap0, gap1 = np.abs(z0 - [t.wheel_radius for t in wheels]), np.abs(ro.wheel_heights() - [t.wheel_radius for t in wheels])
        assert (gap1 < gap0).all()
        ro.free()
        runs[fused] = np.array(traj)
    assert np.abs(runs[True] - runs[False]).max() < 1e-11  # (as the launch variants of tests/test_rollout.py)
    for b, cfg in enumerate(cfgs):
        ft = FrameTask("base", 0.2, 0.1, lm_damping=1e-3, gain=1.0)
        ft.set_target(cfg.get_transform_frame_to_world("base"))
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        for k in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, [ft] + wheels + [p], DT), DT)
            qd = runs[True][k, b].copy()
            if qd[3:7] @ cfg.q[3:7] < 0.0:
                qd[3:7] = -qd[3:7]  # (q and -q are one rotation: the host's integrate picks w > 0, the device keeps the sign)
            assert np.abs(qd - cfg.q).max() < 1e-8, (b, k)


def test_closed_loop_composes_with_com_rows(api):
    """rolling_tasks= beside com_task=: the wheel rows sit behind the centre-of-mass rows, and the two launch variants agree."""
    from pink_amd.rollout import DeviceRollout, pose12

    Bl = 3
    model, q, cfgs, base, wheels, po = _stack(seed=11)
    q0, cfgs = q[:Bl], cfgs[:Bl]
    rng = np.random.default_rng(5)
    for j in model.joints:
        j.mass, j.com = float(rng.uniform(0.5, 2.0)), 0.05 * rng.normal(size=3)
    try:
        com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.3)
        com.set_target_batch(np.array([c.center_of_mass() for c in cfgs]) + 0.01)
        specs = [("base", 0.2, 0.1, 1.0, 1e-3)]
        targets = np.array([[pose12(c.get_transform_frame_to_world("base"))] for c in cfgs])
        runs = {}
        for fused in (True, False):
            ro = DeviceRollout(api, model, q0, specs, DT, posture_cost=1e-2, fused=fused, com_task=com, rolling_tasks=wheels)
            assert ro.Kd == 6 + 3 + 5
            ro.set_targets(targets)
            for _ in range(2):
                ro.step()
            _, st, _ = ro.last_step()
            assert (st == 0).all()
            runs[fused] = ro.configurations()
            ro.free()
        assert np.abs(runs[True] - runs[False]).max() < 1e-11
        # against the batched solve of the same stack from the start configuration: one step
        ro = DeviceRollout(api, model, q0, specs, DT, posture_cost=1e-2, fused=True, com_task=com, rolling_tasks=wheels)
        ro.set_targets(targets)
        ro.step()
        q1 = ro.configurations()
        ro.free()
        ft = FrameTask("base", 0.2, 0.1, lm_damping=1e-3, gain=1.0)
        ft.set_target_poses(np.array([c.get_transform_frame_to_world("base").rotation for c in cfgs]),
                            np.array([c.get_transform_frame_to_world("base").translation for c in cfgs]))
        p = [PostureTask(cost=1e-2) for _ in range(Bl)]
        for b in range(Bl):
            p[b].set_target(q0[b])
        V = solve_ik_batch(ConfigurationBatch(model, q0), [[ft, com] + wheels + [p[b]] for b in range(Bl)], DT, device_kinematics=False)
        for b in range(Bl):
            qh = model.integrate(q0[b], V[b] * DT)
            if qh[3:7] @ q1[b, 3:7] < 0.0:
                qh[3:7] = -qh[3:7]
            assert np.abs(qh - q1[b]).max() < 1e-8
    finally:
        for j in model.joints:
            j.mass, j.com = 0.0, np.zeros(3)
