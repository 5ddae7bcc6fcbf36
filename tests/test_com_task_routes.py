"""ComTask through solve_ik_batch: one ComTask beside FrameTasks takes the hybrid route -- its rows are formed on the
device by pinkhip_com_task_device behind the FrameTask rows -- two take the host-evaluated route; both agree with the
all-host evaluation and with the C Goldfarb-Idnani oracle on a stack built on the host, to the 1e-10 of the device routes."""
import numpy as np
import pytest

import pink_amd
from oracle import c_oracle
from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, PostureTask, build_ik, solve_ik_batch
from pink_amd.lie import exp6
from pink_amd.runtime import set_default_solver
from tests.com_task_cases import configurations, models, with_com


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    s = with_com(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))
    set_default_solver(s)
    yield request.param
    pink_amd.clear_device_cache()
    set_default_solver(None)


def _stack(name, B, seed=3, per_instance_com=False):
    model, frames = models()[name]
    rng = np.random.default_rng(seed)
    q = 0.15 * configurations(name, B=B, seed=seed)  # (inside the joint limits of +-3)
    for j in model.joints:
        if j.kind == "free_flyer":
            q[:, j.idx_q + 3:j.idx_q + 7] /= np.linalg.norm(q[:, j.idx_q + 3:j.idx_q + 7], axis=1, keepdims=True)
    cfgs = [Configuration(model, q[b]) for b in range(B)]
    tasks = []
    for k, f in enumerate(frames):
        ft = FrameTask(f, 1.0, 0.5 if k == 0 else 0.0, lm_damping=1e-3, gain=0.9)
        R, t = np.zeros((B, 3, 3)), np.zeros((B, 3))
        for b, c in enumerate(cfgs):
            T = c.get_transform_frame_to_world(f) * exp6(0.05 * rng.normal(size=6))
            R[b], t[b] = T.rotation, T.translation
        ft.set_target_poses(R, t)
        tasks.append(ft)
    com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
    c0 = np.array([c.center_of_mass() for c in cfgs])
    if per_instance_com:
        com.set_target_batch(c0 + 0.03 * rng.normal(size=(B, 3)))
    else:
        com.set_target(c0.mean(axis=0) + [0.01, -0.02, 0.03])
    po = PostureTask(cost=5e-2)
    po.set_target(model.neutral())
    return model, q, cfgs, tasks, com, po


def _host_qp(cfg, tasks, dt, damping=1e-12):
    """P, q of pink/solve_ik.py:54-90 in NumPy from the tasks' own host methods (pink/tasks/task.py:145-167)."""
    nv = cfg.model.nv
    P, c = damping * np.eye(nv), np.zeros(nv)
    for t in tasks:
        J, e = t.compute_jacobian(cfg), t.compute_error(cfg)
        W = np.diag(np.broadcast_to(np.asarray(t.cost, dtype=float), (J.shape[0],)))
        we = W @ (-t.gain * e)
        P += (W @ J).T @ (W @ J) + t.lm_damping * (we @ we) * np.eye(nv)
        c += -we @ (W @ J)
    return P, c


def _single_instance_tasks(tasks, com, po, b):
    out = []
    for t in tasks:
        if isinstance(t, FrameTask):
            ft = FrameTask(t.frame, t.position_cost.copy(), t.orientation_cost.copy(), lm_damping=t.lm_damping, gain=t.gain)
            p = t.poses12()[b]
            from pink_amd.lie import SE3

            ft.set_target(SE3(p[:9].reshape(3, 3), p[9:]))
            out.append(ft)
    for cm in com:
        c1 = ComTask(cm.cost.copy(), lm_damping=cm.lm_damping, gain=cm.gain)
        c1.set_target(cm.target_com if cm.target_coms is None else cm.target_coms[b])
        out.append(c1)
    return out + [po]


@pytest.mark.parametrize("per_instance", [False, True])
def test_one_com_task_takes_the_hybrid_route(backend, per_instance):
    B, dt = 64, 5e-3
    model, q, cfgs, frame_tasks, com, po = _stack("tree12", B, per_instance_com=per_instance)
    tasks = frame_tasks + [com, po]
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "hybrid"
    assert stats["failed"] == 0 and stats["instances"] == B
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, device_kinematics=False)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated"
    assert pink_amd.last_solve_stats()["failed"] == 0  # (the same statuses: every instance solved on both routes)
    err = np.abs(V - V_host).max() * dt
    print(f"{backend}: hybrid vs host-evaluated max|dq| difference {err:.3e}")
    assert err < 1e-10 and np.abs(V).max() * dt > 1e-4
    # the oracle on the stack built on the host
    worst = 0.0
    for b in range(0, B, 8):
        mine = _single_instance_tasks(frame_tasks, [com], po, b)
        P, c = _host_qp(cfgs[b], mine, dt)
        prob = build_ik(cfgs[b], mine, dt)
        x, status, _, _ = c_oracle.gi_solve(P, c, prob.G, prob.h)
        assert status == 0
        worst = max(worst, np.abs(V[b] * dt - x).max())
    print(f"{backend}: hybrid vs oracle max|dq| difference {worst:.3e}")
    assert worst < 1e-10


def test_two_com_tasks_take_the_host_evaluated_route(backend):
    B, dt = 64, 5e-3
    model, q, cfgs, frame_tasks, com, po = _stack("tree12", B)
    com2 = ComTask(0.3, gain=0.4)
    com2.set_target(com.target_com + [0.0, 0.05, 0.0])
    tasks = frame_tasks + [com, com2, po]
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated"
    worst = 0.0
    for b in range(0, B, 16):
        mine = _single_instance_tasks(frame_tasks, [com, com2], po, b)
        P, c = _host_qp(cfgs[b], mine, dt)
        prob = build_ik(cfgs[b], mine, dt)
        x, status, _, _ = c_oracle.gi_solve(P, c, prob.G, prob.h)
        assert status == 0
        worst = max(worst, np.abs(V[b] * dt - x).max())
    assert worst < 1e-10


def test_the_whole_step_route_declines_a_com_task(backend):
    """device_kinematics=True insists on the whole-step kernel, which does not form centre-of-mass rows."""
    from pink_amd.exceptions import PinkError

    B, dt = 64, 5e-3
    model, q, cfgs, frame_tasks, com, po = _stack("tree12", B)
    with pytest.raises(PinkError):
        solve_ik_batch(ConfigurationBatch(model, q), frame_tasks + [com, po], dt, strict_route="device")


def test_a_mass_edit_is_not_served_from_the_cached_device_state(backend):
    B, dt = 64, 5e-3
    model, q, cfgs, frame_tasks, com, po = _stack("tree12", B)
    tasks = frame_tasks + [com, po]
    V0 = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    old = model.joints[5].mass
    try:
        model.joints[5].mass = 3.0 * old
        V1 = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
        assert pink_amd.last_solve_stats()["route"] == "hybrid"
        V1_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, device_kinematics=False)
        assert np.abs(V1 - V1_host).max() * dt < 1e-10 and np.abs(V1 - V0).max() * dt > 1e-8
    finally:
        model.joints[5].mass = old


# ---- closed loop ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def loop_api(request):
    s = with_com(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))
    set_default_solver(s)
    yield s
    pink_amd.clear_device_cache()
    set_default_solver(None)


# (tree34 on the GPU only: the emulator takes 0.17 s per QP of 39 coordinates, 80 of them in this test)
@pytest.mark.parametrize("loop_api, name", [("emu", "tree12"), pytest.param("gpu", "tree12", marks=pytest.mark.gpu),
                                            pytest.param("gpu", "tree34", marks=pytest.mark.gpu)], indirect=["loop_api"])
def test_closed_loop_with_a_com_task_matches_the_host_loop(loop_api, name):
    """DeviceRollout(com_task=...): step kernel -> centre-of-mass kernel -> solve (fused=True) follows the host loop of
    solve_ik + integrate to the 1e-8 tests/test_rollout.py holds its closed loops to, |com - target| falls with every
    step, the five-launch step (fused=False) agrees, and the whole-step kernel is refused."""
    from pink_amd import solve_ik
    from pink_amd.rollout import DeviceRollout, pose12

    api = loop_api
    B, dt, steps = 5, 5e-3, 8
    model, q0, cfgs, _, _, _ = _stack(name, B, seed=9)
    frames = models()[name][1]
    rng = np.random.default_rng(17)
    specs = [(f, 0.2, 0.1 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    targets = np.array([[pose12(c.get_transform_frame_to_world(f)) for f in frames] for c in cfgs])
    c0 = np.array([c.center_of_mass() for c in cfgs])
    shift = rng.normal(size=(B, 3))
    com_targets = c0 + 0.03 * shift / np.linalg.norm(shift, axis=1, keepdims=True)  # 3 cm from the start
    # (gain 0.3: eight steps leave 0.7^8 = 6 % of the 3 cm, far above the residual at which the frame tasks, held where
    # they started, balance the ComTask -- up to there the distance falls with every step)
    com = ComTask([4.0, 5.0, 3.0], lm_damping=1e-4, gain=0.3)
    com.set_target_batch(com_targets)
    with pytest.raises(ValueError, match="whole-step kernel does not form centre-of-mass rows"):
        DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused="kernel", com_task=com)
    runs = {}
    for fused in (True, False):
        ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused=fused, com_task=com)
        ro.set_targets(targets)
        traj, dist = [], [np.linalg.norm(ro.center_of_mass() - com_targets, axis=1)]
        for _ in range(steps):
            ro.step()
            traj.append(ro.configurations())
            dist.append(np.linalg.norm(ro.center_of_mass() - com_targets, axis=1))
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        ro.free()
        runs[fused] = np.array(traj)
        dist = np.array(dist)
        assert abs(dist[0] - 0.03).max() < 1e-12 and (np.diff(dist, axis=0) < 0.0).all(), dist
    assert np.abs(runs[True] - runs[False]).max() < 1e-11  # (as the launch variants of tests/test_rollout.py)
    # host loop: the same steps with per-instance solve_ik + integrate
    for b, cfg in enumerate(cfgs):
        tl = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            t.set_target(cfg.get_transform_frame_to_world(f))
            tl.append(t)
        cm = ComTask(com.cost.copy(), lm_damping=com.lm_damping, gain=com.gain)
        cm.set_target(com_targets[b])
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        for k in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, tl + [cm, p], dt), dt)
            qd = runs[True][k, b].copy()
            if model.root_joint is not None and qd[3:7] @ cfg.q[3:7] < 0.0:
                qd[3:7] = -qd[3:7]  # (q and -q are one rotation: the host's integrate picks w > 0, the device keeps the sign)
            assert np.abs(qd - cfg.q).max() < 1e-8, (b, k)
