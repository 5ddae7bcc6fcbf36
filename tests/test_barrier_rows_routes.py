"""Barriers beside a ComTask: solve_ik_batch takes the hybrid route with the barrier rows formed on the device by
pinkhip_barrier_rows_device -- no forward kinematics on the host -- and DeviceRollout(com_task=..., position_barriers=[...])
closes the loop with fused=True / False; both agree with the all-host evaluation to the bars tests/test_com_task_routes.py
holds its routes to (1e-10 on dq of one solve, 1e-8 on the closed loop)."""
import numpy as np
import pytest

import pink_amd
from pink_amd import ComTask, Configuration, ConfigurationBatch, FrameTask, PostureTask, solve_ik, solve_ik_batch
from pink_amd.barriers import BodySphericalBarrier, PositionBarrier, SelfCollisionBarrier
from pink_amd.barriers.self_collision_barrier import SpherePairs
from pink_amd.lie import exp6
from pink_amd.runtime import set_default_solver
from tests.barrier_rows_cases import configurations, models, with_barrier_rows
from tests.row_kernel_kit import with_com

NAME = "B"  # free-flyer root, two branches, one prismatic joint, every joint with mass


def _solver(request, which):
    return with_barrier_rows(with_com(request.getfixturevalue("emu" if which == "emu" else "gpu_solver")))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    set_default_solver(_solver(request, request.param))
    yield request.param
    pink_amd.clear_device_cache()
    set_default_solver(None)


def _start(B, seed=3, spread=0.15):
    model, what = models()[NAME]
    q = spread * configurations(NAME, B=B, seed=seed)  # (inside the joint limits)
    for j in model.joints:
        if j.kind == "free_flyer":
            q[:, j.idx_q + 3:j.idx_q + 7] /= np.linalg.norm(q[:, j.idx_q + 3:j.idx_q + 7], axis=1, keepdims=True)
    return model, what, q


def _sphere_barrier(what, n_rows=2):
    ja, jb, jc = what["sphere_joints"]
    s0, s1, s2 = (ja, [0.05, -0.02, 0.03], 0.03), (jb, [-0.04, 0.03, 0.02], 0.02), (jc, [0.02, 0.01, -0.03], 0.025)
    return SelfCollisionBarrier(n_rows, gain=1.6, d_min=0.01, distance_query=SpherePairs([(*s0, *s1), (*s0, *s2), (*s1, *s2)]))


def _stack(B, class_k=None):
    """FrameTasks on the two branch tips (targets 5 cm off), a PostureTask, a ComTask, and barriers of all three kinds; the
    PositionBarrier's p_max sits 2 mm in front of the right tip of the robot that is furthest along x."""
    model, what, q = _start(B)
    rng = np.random.default_rng(5)
    cfgs = [Configuration(model, q[b]) for b in range(B)]
    tasks = []
    for k, f in enumerate(what["branches"]):
        ft = FrameTask(f, 1.0, 0.5 if k == 0 else 0.0, lm_damping=1e-3, gain=0.9)
        R, t = np.zeros((B, 3, 3)), np.zeros((B, 3))
        for b, c in enumerate(cfgs):
            T = c.get_transform_frame_to_world(f) * exp6(0.05 * rng.normal(size=6))
            R[b], t[b] = T.rotation, T.translation
        ft.set_target_poses(R, t)
        tasks.append(ft)
    com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
    com.set_target(np.array([c.center_of_mass() for c in cfgs]).mean(axis=0) + [0.01, -0.02, 0.03])
    po = PostureTask(cost=5e-2)
    po.set_target(model.neutral())
    tip = np.array([c.get_transform_frame_to_world(what["tip"]).translation for c in cfgs])
    pb = PositionBarrier(what["tip"], indices=[0, 2], p_min=tip.min(axis=0)[[0, 2]] - 0.5, p_max=tip.max(axis=0)[[0, 2]] + 0.002,
                         gain=np.array([1.0, 0.8, 1.2, 0.9]))
    if class_k is not None:
        pb.gain_function, pb.identity_gain_function = class_k, False
    barriers = [pb, BodySphericalBarrier(what["branches"], d_min=0.05, gain=1.5), _sphere_barrier(what)]
    return model, q, tasks + [com, po], barriers


def test_barriers_beside_a_com_task_are_formed_on_the_device(backend, monkeypatch):
    """route hybrid, barrier_rows device, no BatchKinematics on the way, dq of the all-host evaluation."""
    from pink_amd.kinematics_batch import BatchKinematics

    B, dt = 64, 5e-3
    model, q, tasks, barriers = _stack(B)
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, barriers=barriers, gpu_frame_tasks=False)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "host-evaluated" and stats["barrier_rows"] == "host" and stats["failed"] == 0

    def never(self, *a, **k):
        raise AssertionError("forward kinematics on the host")

    with monkeypatch.context() as mp:
        mp.setattr(BatchKinematics, "__init__", never)
        V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, barriers=barriers)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "hybrid" and stats["barrier_rows"] == "device"
    assert stats["failed"] == 0 and stats["instances"] == B
    err = np.abs(V - V_host).max() * dt
    print(f"{backend}: hybrid with device barrier rows vs all-host max|dq| difference {err:.3e}")
    assert err < 1e-10 and np.abs(V).max() * dt > 1e-4
    # the barriers matter: without them the answer is another one
    V_free = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt)
    assert pink_amd.last_solve_stats()["barrier_rows"] is None
    assert np.abs(V_free - V).max() * dt > 1e-6


def test_a_class_k_function_of_the_callers_keeps_the_barriers_on_the_host(backend):
    B, dt = 64, 5e-3
    model, q, tasks, barriers = _stack(B, class_k=lambda h: h / (1.0 + np.abs(h)))
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, barriers=barriers)
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "hybrid" and stats["barrier_rows"] == "host" and stats["failed"] == 0
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, dt, barriers=barriers, gpu_frame_tasks=False)
    assert np.abs(V - V_host).max() * dt < 1e-10


def test_what_the_kernel_does_not_form_stays_on_the_host(backend):
    """device_barriers: a user subclass, a second SelfCollisionBarrier, a custom distance query, a safe displacement of the
    barrier's own -- each sends every barrier of the call to the host evaluation."""
    from pink_amd.hybrid import device_barriers
    from pink_amd.runtime import default_solver

    model, what, _ = _start(1)
    api = default_solver()
    ok = [PositionBarrier(what["tip"], p_min=np.array([-1.0, -1.0, -1.0])), BodySphericalBarrier(what["branches"], d_min=0.05), _sphere_barrier(what)]
    order = device_barriers(model, [ok[2], ok[0], ok[1]], api)
    assert order == [ok[0], ok[1], ok[2]]  # (Pink's order, the sphere pairs last)

    class Mine(PositionBarrier):
        pass

    class Pushing(PositionBarrier):
        def compute_safe_displacement(self, configuration):
            return np.ones(configuration.model.nv)

    custom_query = _sphere_barrier(what)
    custom_query.distance_query = lambda configuration: SpherePairs([])(configuration)
    for extra in (Mine(what["tip"], p_min=np.zeros(3)), Pushing(what["tip"], p_min=np.zeros(3)), _sphere_barrier(what), custom_query,
                  PositionBarrier("no_such_frame", p_min=np.zeros(3))):
        assert device_barriers(model, ok + [extra], api) is None, type(extra).__name__
    assert device_barriers(model, [], api) is None


# ---- closed loop ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def loop_api(request):
    s = _solver(request, request.param)
    set_default_solver(s)
    yield s
    pink_amd.clear_device_cache()
    set_default_solver(None)


@pytest.mark.parametrize("loop_api", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)], indirect=True)
def test_closed_loop_with_a_com_task_and_barriers_matches_the_host_loop(loop_api):
    """DeviceRollout(com_task=..., position_barriers=[...]): step kernel -> centre-of-mass kernel -> barrier kernel -> solve
    (fused=True) follows the host loop of solve_ik + integrate over three steps to 1e-8, the five-launch step (fused=False)
    agrees, a barrier row is active on the way, and the whole-step kernel is still refused."""
    from pink_amd.rollout import DeviceRollout, pose12

    api = loop_api
    B, dt, steps = 5, 5e-3, 3
    model, what, q0 = _start(1, seed=9)
    rng = np.random.default_rng(17)
    q0 = np.repeat(q0, B, axis=0)
    movable = [j.idx_q for j in model.joints if j.kind != "free_flyer"]
    q0[:, movable] += 1e-3 * rng.normal(size=(B, len(movable)))  # (five robots within a millimetre of each other)
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    frames = list(what["branches"])
    specs = [(f, 1.0, 0.1 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    targets = np.array([[pose12(c.get_transform_frame_to_world(f)) for f in frames] for c in cfgs])
    targets[:, 1, 9] += 0.05  # the right tip is asked 5 cm along x ...
    tip = np.array([c.get_transform_frame_to_world(frames[1]).translation for c in cfgs])
    # ... and the barrier stops it 2 mm from where the foremost robot starts
    pb = PositionBarrier(frames[1], indices=[0], p_max=np.array([tip[:, 0].max() + 0.002]), gain=np.array([1.0]))
    barriers = [pb, BodySphericalBarrier((frames[0], frames[1]), d_min=0.05, gain=1.5), _sphere_barrier(what)]
    com = ComTask([4.0, 5.0, 3.0], lm_damping=1e-4, gain=0.3)
    com.set_target_batch(np.array([c.center_of_mass() for c in cfgs]) + [0.01, -0.01, 0.02])
    with pytest.raises(ValueError, match="whole-step kernel does not form centre-of-mass rows"):
        DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused="kernel", com_task=com, position_barriers=barriers)
    runs = {}
    for fused in (True, False):
        ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused=fused, com_task=com, position_barriers=barriers)
        ro.set_targets(targets)
        traj = []
        for _ in range(steps):
            ro.step()
            traj.append(ro.configurations())
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        ro.free()
        runs[fused] = np.array(traj)
    assert np.abs(runs[True] - runs[False]).max() < 1e-11  # (as the launch variants of tests/test_rollout.py)
    # host loop: the same steps with per-instance solve_ik + integrate
    least_slack = np.inf
    for b, cfg in enumerate(cfgs):
        tl = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            t.set_target(cfg.get_transform_frame_to_world(f))
            if i == 1:
                t.transform_target_to_world.translation[0] += 0.05
            tl.append(t)
        cm = ComTask(com.cost.copy(), lm_damping=com.lm_damping, gain=com.gain)
        cm.set_target(com.target_coms[b])
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        for k in range(steps):
            G, h = pb.compute_qp_inequalities(cfg, dt)
            v = solve_ik(cfg, tl + [cm, p], dt, barriers=barriers)
            least_slack = min(least_slack, float((h - G @ (v * dt)).min()))
            cfg.integrate_inplace(v, dt)
            qd = runs[True][k, b].copy()
            if qd[3:7] @ cfg.q[3:7] < 0.0:
                qd[3:7] = -qd[3:7]  # (q and -q are one rotation: the host's integrate picks w > 0, the device keeps the sign)
            assert np.abs(qd - cfg.q).max() < 1e-8, (b, k)
    print(f"least slack of the position barrier's row over the host loop: {least_slack:.3e}")
    assert abs(least_slack) < 1e-9  # the row G dq <= h holds with equality: the barrier is active
