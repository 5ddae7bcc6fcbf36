"""Device-side kinematics and the closed IK loop against the host
pipeline (NumPy Configuration + per-instance solve_ik), on the CPU wave emulator and on the GPU."""
import numpy as np
import pytest

import pink_amd
from pink_amd import Configuration, FrameTask, PostureTask, build_chain, solve_ik
from pink_amd.lie import SE3, exp3, exp6
from pink_amd.rollout import DeviceRollout, ModelArrays, pose12
from pink_amd.runtime import set_default_solver


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    s = request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver")
    set_default_solver(s)
    yield s
    set_default_solver(None)


def _models():
    arm = build_chain(6)
    humanoid = build_chain(9, free_flyer=True, seed=3)  # free-flyer root + 9 revolute joints: nv = 15
    humanoid.add_frame("mid", 4, SE3(np.eye(3), [0.05, 0.0, 0.1]))
    arm12 = build_chain(12, seed=5)  # nv = 12: a 16-lane group whose kinematics scratch exceeds the solve's LDS share
    # free flyer + 24 joints: nv = 30, the headline shape -- with barrier rows 30 + md tableau rows on a 32-lane group
    # (virtual dense rows, ik_sweepx.h)
    big = build_chain(24, free_flyer=True, seed=2)
    return [(arm, ["tool0"]), (humanoid, ["tool0", "mid"]), (arm12, ["tool0", "joint_6"]), (big, ["tool0", "joint_12"])]


def _edge_models():
    """Trees with PRISMATIC joints at the joint counts of ``_models()`` (the same kernel instantiations): the
    ``angular`` / ``lin`` branch of the Jacobian columns, ``joint_transform``'s translation and the whole-step kernel's
    sink run with a joint type that ``build_chain`` never makes.  Generic unit axes, rotated placements.
      tree15   free-flyer + 9 joints, every third one prismatic; two branches of different depth leave joint_3 (pointer
               jumping sees unequal depths); frames on both tips and mid-chain
      arm12p   12 joints, four prismatic (the 16-lane group)
      big30p   free-flyer + 24 joints, four prismatic (the 32-lane group)
    Limits leave room around the start configurations of the loops below (|q| <= 0.6 on a revolute, 0.3 on a
    prismatic joint)."""

    def add(model, i, parent, rng, prismatic):
        off = SE3(exp3(0.4 * rng.normal(size=3)), [0.2 + 0.1 * (i % 2), 0.03 * (i % 3 - 1), 0.05 * (i % 3)])
        if prismatic:
            return model.add_joint(f"joint_{i}", "prismatic", parent, off, rng.normal(size=3), -0.8, 0.8, 1.0)
        return model.add_joint(f"joint_{i}", "revolute", parent, off, rng.normal(size=3), -np.pi, np.pi, 3.15)

    tip = SE3(exp3([0.2, -0.1, 0.3]), [0.15, 0.02, -0.04])
    rng = np.random.default_rng(21)
    tree = pink_amd.configuration.Model()
    p = tree.add_joint("root_joint", "free_flyer")
    for i in (1, 2, 3):
        p = add(tree, i, p, rng, i % 3 == 0)
    fork = p
    for i in (4, 5, 6, 7):  # the long branch
        p = add(tree, i, p, rng, i % 3 == 0)
    tree.add_frame("tip_a", p, tip)
    p = fork
    for i in (8, 9):  # the short one
        p = add(tree, i, p, rng, i % 3 == 0)
    tree.add_frame("tip_b", p, tip)

    rng = np.random.default_rng(22)
    arm = pink_amd.configuration.Model()
    p = -1
    for i in range(1, 13):
        p = add(arm, i, p, rng, i % 3 == 0)
    arm.add_frame("tool0", p, tip)

    rng = np.random.default_rng(23)
    big = pink_amd.configuration.Model()
    p = big.add_joint("root_joint", "free_flyer")
    for i in range(1, 25):
        p = add(big, i, p, rng, i % 6 == 0)
    big.add_frame("tool0", p, tip)
    return {"tree15": (tree, ["tip_a", "tip_b", "joint_2"]), "arm12p": (arm, ["tool0", "joint_6"]),
            "big30p": (big, ["tool0", "joint_12"])}


def _pick(which):
    """``_models()[which]`` for an index, ``_edge_models()[which]`` for a name."""
    return _edge_models()[which] if isinstance(which, str) else _models()[which]


def _random_q(model, B, rng):
    q = np.tile(model.neutral(), (B, 1))
    for j in model.joints:
        if j.kind == "free_flyer":
            for b in range(B):
                M = exp6(rng.normal(size=6) * 0.5)
                q[b, j.idx_q:j.idx_q + 3] = M.translation
                from pink_amd.configuration import _rot_to_quat
                q[b, j.idx_q + 3:j.idx_q + 7] = _rot_to_quat(M.rotation)
        else:
            q[:, j.idx_q] = rng.uniform(-1.2, 1.2, size=B)
    return q


def test_fk_frame_jacobians_limits_integrate_match_host(api):
    rng = np.random.default_rng(0)
    for model, frames in _models():
        B = 5
        q = _random_q(model, B, rng)
        arrays = ModelArrays(model, frames)
        dm = api.model_create(arrays.desc)
        nf, nv, nq = len(frames), model.nv, model.nq
        d_q, d_T, d_J = api.alloc(8 * B * nq), api.alloc(8 * B * nf * 12), api.alloc(8 * B * nf * 6 * nv)
        api.put(d_q, q)
        api.fk(dm, B, d_q, d_T, d_J)
        api.sync()
        T = np.zeros((B, nf, 12))
        J = np.zeros((B, nf, 6, nv))
        api.get(T, d_T)
        api.get(J, d_J)
        cfgs = [Configuration(model, q[b]) for b in range(B)]
        for b, cfg in enumerate(cfgs):
            for f, name in enumerate(frames):
                assert np.abs(T[b, f] - pose12(cfg.get_transform_frame_to_world(name))).max() < 1e-13
                assert np.abs(J[b, f] - cfg.get_frame_jacobian(name)).max() < 1e-13
        # limits + posture error
        d_lb, d_ub, d_e, d_qt = api.alloc(8 * B * nv), api.alloc(8 * B * nv), api.alloc(8 * B * nv), api.alloc(8 * nq)
        qt = model.neutral()
        api.put(d_qt, qt)
        root_nv = pink_amd.utils.get_root_joint_dim(model)[1]
        api.limits_posture(dm, B, 5e-3, 0.5, d_q, d_qt, 0, d_lb, d_ub, d_e, nv, 0)
        api.sync()
        lb, ub, e = np.zeros((B, nv)), np.zeros((B, nv)), np.zeros((B, nv))
        api.get(lb, d_lb), api.get(ub, d_ub), api.get(e, d_e)
        for b, cfg in enumerate(cfgs):
            lo, hi = np.full(nv, -np.inf), np.full(nv, np.inf)
            for lim in (model.configuration_limit, model.velocity_limit):
                idx, l_, u_ = lim.compute_box(cfg, 5e-3)
                lo[idx], hi[idx] = np.maximum(lo[idx], l_), np.minimum(hi[idx], u_)
            assert np.array_equal(lb[b], lo) and np.array_equal(ub[b], hi)
            post = PostureTask(cost=1.0)
            post.set_target(qt)
            assert np.abs(e[b, :nv - root_nv] - post.compute_error(cfg)).max() < 1e-15
        # integrate
        dq = 0.1 * rng.normal(size=(B, nv))
        d_dq = api.alloc(8 * B * nv)
        api.put(d_dq, dq)
        api.integrate(dm, B, d_q, d_dq)
        api.sync()
        q2 = np.zeros((B, nq))
        api.get(q2, d_q)
        for b in range(B):
            ref = model.integrate(q[b], dq[b])
            for j in model.joints:  # quaternions are defined up to sign: compare the transforms
                a_ = model.joint_transform(j, q2[b])
                r_ = model.joint_transform(j, ref)
                assert np.abs(a_.rotation - r_.rotation).max() < 1e-13 and np.abs(a_.translation - r_.translation).max() < 1e-13
        for p in (d_q, d_T, d_J, d_lb, d_ub, d_e, d_qt, d_dq):
            api.release(p)
        api.model_destroy(dm)


def test_fk_and_integrate_against_the_independent_oracle(api):
    """Device kinematics vs oracle/kinematics_oracle.py (expm products, finite-difference Jacobians)."""
    from oracle import kinematics_oracle as ko

    rng = np.random.default_rng(4)
    for model, frames in _models():
        B = 3
        q = _random_q(model, B, rng)
        arr = ModelArrays(model, frames)
        dm = api.model_create(arr.desc)
        nf, nv, nq = len(frames), model.nv, model.nq
        d_q, d_T, d_J, d_dq = api.alloc(8 * B * nq), api.alloc(8 * B * nf * 12), api.alloc(8 * B * nf * 6 * nv), api.alloc(8 * B * nv)
        api.put(d_q, q)
        api.fk(dm, B, d_q, d_T, d_J)
        api.sync()
        T, J = np.zeros((B, nf, 12)), np.zeros((B, nf, 6, nv))
        api.get(T, d_T), api.get(J, d_J)
        for b in range(B):
            Tr = ko.frame_poses(arr, q[b])
            for f in range(nf):
                assert np.abs(T[b, f, :9].reshape(3, 3) - Tr[f][:3, :3]).max() < 1e-12
                assert np.abs(T[b, f, 9:] - Tr[f][:3, 3]).max() < 1e-12
            assert np.abs(J[b] - ko.frame_jacobians_fd(arr, q[b])).max() < 1e-6  # tests/test_jacobians.py tolerance 1e-5
        dq = 0.2 * rng.normal(size=(B, nv))
        api.put(d_dq, dq)
        api.integrate(dm, B, d_q, d_dq)
        api.sync()
        q2 = np.zeros((B, nq))
        api.get(q2, d_q)
        for b in range(B):
            assert np.abs(ko.frame_poses(arr, q2[b]) - ko.frame_poses(arr, ko.integrate(arr, q[b], dq[b]))).max() < 1e-12
        for p in (d_q, d_T, d_J, d_dq):
            api.release(p)
        api.model_destroy(dm)


@pytest.mark.parametrize("fused", [True, "kernel"])
@pytest.mark.parametrize("which", [0, 1, "tree15", "arm12p", "big30p"])
def test_closed_loop_matches_host_loop_and_converges(api, which, fused):
    """tests/test_solve_ik.py:160-210 / examples/inverse_kinematics_ur10.py:75-91, batched; with two launches per
    step (step kernel + solve) and with the whole step in one kernel.  The named models (``_edge_models``) carry
    prismatic joints."""
    model, frames = _pick(which)
    rng = np.random.default_rng(10 + (which if isinstance(which, int) else len(which) + model.nv))
    B, dt, steps = 4, 5e-3, (40 if isinstance(which, int) else 12)
    q0 = _random_q(model, B, rng) * 0.5 + 0.5 * np.tile(model.neutral(), (B, 1))
    if model.root_joint is not None:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    specs = [(f, 1.0, 0.5 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    targets = np.zeros((B, len(frames), 12))
    host_tasks = []
    for b, cfg in enumerate(cfgs):
        tl = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            tgt = cfg.get_transform_frame_to_world(f) * SE3(np.eye(3), 0.05 * rng.normal(size=3))
            t.set_target(tgt)
            targets[b, i] = pose12(tgt)
            tl.append(t)
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        tl.append(p)
        host_tasks.append(tl)
    ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused=fused)
    ro.set_targets(targets)
    ro.run(steps)
    # the one-kernel step exists for the floating-base model; the 6-dof arm (an 8-lane group) keeps two launches
    assert ro.fused == (fused if which != 0 else True)
    qd = ro.configurations()
    _, st, _ = ro.last_step()
    assert (st == 0).all()
    # host loop: same steps with per-instance solve_ik + integrate_inplace
    for b, cfg in enumerate(cfgs):
        e0 = np.linalg.norm(host_tasks[b][0].compute_error(cfg))
        for _ in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, host_tasks[b], dt), dt)
        cd = Configuration(model, qd[b])
        for f in frames:
            Ta, Tb = cd.get_transform_frame_to_world(f), cfg.get_transform_frame_to_world(f)
            assert np.abs(Ta.translation - Tb.translation).max() < 1e-8 and np.abs(Ta.rotation - Tb.rotation).max() < 1e-8
        assert np.linalg.norm(host_tasks[b][0].compute_error(cd)) < e0  # the loop makes progress on every robot
    ro.free()


@pytest.mark.parametrize("which", [1, 2, 3, "tree15", "arm12p", "big30p"])
def test_closed_loop_with_position_barriers_matches_host_loop(api, which):
    """PositionBarrier rows (pink/barriers/position_barrier.py:109-153; G = -J_h / dt, h = gain * barrier,
    pink/barriers/barrier.py:246-254) formed on chip by the whole-step kernel: the closed loop with two barriers --
    one of them active along the way, one with a safe-displacement gain -- follows the host loop (per-instance
    solve_ik(..., barriers=...) + integrate_inplace) to 1e-8, and solve_ik_batch takes the same device path.  On the
    named models (``_edge_models``) both barrier frames sit behind prismatic joints."""
    from pink_amd import solve_ik_batch
    from pink_amd.barriers import PositionBarrier

    model, frames = _pick(which)
    frames = frames[:2]
    rng = np.random.default_rng(70 + (which if isinstance(which, int) else len(which) + model.nv))
    B, dt, steps = 3, 5e-3, (25 if which in (1, 2) else 12)
    q0 = _random_q(model, B, rng) * 0.5 + 0.5 * np.tile(model.neutral(), (B, 1))
    if model.root_joint is not None:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    specs = [(f, 1.0, 0.5 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    p0 = np.array([[c.get_transform_frame_to_world(f).translation for f in frames] for c in cfgs])  # [B, nf, 3]
    # a ceiling 1 cm above the highest tool position while every target sits 8 cm above its tool: the barrier binds;
    # a box around the second frame that never binds but carries a safe-displacement gain (rho on the diagonal)
    bars = [PositionBarrier(frames[0], indices=[2], p_max=np.array([p0[:, 0, 2].max() + 0.01]), gain=np.array([50.0])),
            PositionBarrier(frames[1], indices=[0, 1], p_min=p0[:, 1, :2].min(axis=0) - 0.5, p_max=p0[:, 1, :2].max(axis=0) + 0.5,
                            gain=np.array([100.0, 100.0]), safe_displacement_gain=1.0)]
    targets = np.zeros((B, len(frames), 12))
    host_tasks = []
    for b, cfg in enumerate(cfgs):
        tl = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            tgt = cfg.get_transform_frame_to_world(f).copy()
            tgt.translation = tgt.translation + (np.array([0.0, 0.0, 0.08]) if i == 0 else 0.02 * rng.normal(size=3))
            t.set_target(tgt)
            targets[b, i] = pose12(tgt)
            tl.append(t)
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        tl.append(p)
        host_tasks.append(tl)
    # one step through the API: the device path is taken (barriers no longer send the batch to the host path)
    V_dev = solve_ik_batch(cfgs, host_tasks, dt, barriers=bars, device_kinematics=True)
    for b, cfg in enumerate(cfgs):
        assert np.abs(V_dev[b] - solve_ik(cfg, host_tasks[b], dt, barriers=bars)).max() < 1e-8
    pink_amd.clear_device_cache()
    ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused="kernel", position_barriers=bars)
    ro.set_targets(targets)
    ro.run(steps)
    assert ro.fused == "kernel" and ro.md == 5
    qd = ro.configurations()
    _, st, it = ro.last_step()
    assert (st == 0).all()
    bound_hit = False
    for b, cfg in enumerate(cfgs):
        for _ in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, host_tasks[b], dt, barriers=bars), dt)
        cd = Configuration(model, qd[b])
        for f in frames:
            Ta, Tb = cd.get_transform_frame_to_world(f), cfg.get_transform_frame_to_world(f)
            assert np.abs(Ta.translation - Tb.translation).max() < 1e-8 and np.abs(Ta.rotation - Tb.rotation).max() < 1e-8
        z = cd.get_transform_frame_to_world(frames[0]).translation[2]
        assert z <= bars[0].p_max[0] + 1e-9  # the barrier holds
        bound_hit |= z > bars[0].p_max[0] - 5e-3
    assert bound_hit  # ... and it was needed: at least one robot ends up against it
    ro.free()


@pytest.mark.parametrize("placement", ["identity", "offset", "rotated"])
def test_closed_loop_with_floating_base_velocity_limit_matches_host_loop(api, placement):
    """FloatingBaseVelocityLimit (pink/limits/floating_base_velocity_limit.py:104-148) on the device: the Jacobian of
    a frame attached to the root joint is constant on the root columns, so its axis-aligned rows are a box on the root
    coordinates (identity placement: all twelve) and the others the first dense rows of the whole-step kernel
    (offset: six, rotated: twelve), stacked before a PositionBarrier's as Pink does.  The closed loop follows the host
    loop -- solve_ik with the limit attached to the model, as pink/solve_ik.py:94-105 picks it up -- to 1e-8, and the
    limit binds along the way."""
    from pink_amd import solve_ik_batch
    from pink_amd.barriers import PositionBarrier
    from pink_amd.limits import FloatingBaseVelocityLimit
    from pink_amd.rollout import _floating_base_rows

    model, frames = _models()[1]
    root_id = model.joints.index(model.root_joint)
    Rz = exp6(np.array([0, 0, 0, 0.3, -0.2, 0.5])).rotation
    T = {"identity": SE3(np.eye(3), np.zeros(3)), "offset": SE3(np.eye(3), [0.05, -0.02, 0.1]), "rotated": SE3(Rz, [0.05, -0.02, 0.1])}[placement]
    model.add_frame("pelvis", root_id, T)
    rng = np.random.default_rng(90)
    B, dt, steps = 3, 5e-3, 20
    q0 = _random_q(model, B, rng) * 0.5 + 0.5 * np.tile(model.neutral(), (B, 1))
    q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    limit = FloatingBaseVelocityLimit(model, "pelvis", max_linear_velocity=[0.2, 0.3, np.inf], max_angular_velocity=0.5)
    box, rows, h = _floating_base_rows(model, limit, dt)
    assert len(h) == {"identity": 0, "offset": 4, "rotated": 10}[placement]
    assert np.isfinite(box).sum() == {"identity": 10, "offset": 6, "rotated": 0}[placement]
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    specs = [(f, 1.0, 0.5 if i == 0 else 0.0, 1.0, 1e-3) for i, f in enumerate(frames)]
    p0 = np.array([[c.get_transform_frame_to_world(f).translation for f in frames] for c in cfgs])
    bars = [PositionBarrier(frames[0], indices=[2], p_max=np.array([p0[:, 0, 2].max() + 0.05]), gain=np.array([50.0]))]
    targets = np.zeros((B, len(frames), 12))
    host_tasks = []
    for b, cfg in enumerate(cfgs):
        tl = []
        for i, (f, pc, oc, gain, lm) in enumerate(specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            tgt = cfg.get_transform_frame_to_world(f).copy()
            tgt.translation = tgt.translation + np.array([0.3, -0.2, 0.1])  # far: the base wants to move fast
            t.set_target(tgt)
            targets[b, i] = pose12(tgt)
            tl.append(t)
        p = PostureTask(cost=1e-1)
        p.set_target(q0[b])
        tl.append(p)
        host_tasks.append(tl)
    model.floating_base_velocity_limit = limit
    try:
        V_dev = solve_ik_batch(cfgs, host_tasks, dt, barriers=bars, device_kinematics=True)
        bound = False
        for b, cfg in enumerate(cfgs):
            v = solve_ik(cfg, host_tasks[b], dt, barriers=bars)
            assert np.abs(V_dev[b] - v).max() < 1e-8
            twist = cfg.get_frame_jacobian("pelvis")[:, :6] @ v[:6]
            assert (np.abs(twist) <= limit.twist_max + 1e-9).all()
            bound |= bool((np.abs(twist) > limit.twist_max - 1e-6).any())
        assert bound  # the limit is active in the first step of at least one robot
        pink_amd.clear_device_cache()
        ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-1, fused="kernel", position_barriers=bars, floating_base_limit=limit)
        ro.set_targets(targets)
        ro.run(steps)
        assert ro.fused == "kernel" and ro.md == len(h) + 1
        qd = ro.configurations()
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        for b, cfg in enumerate(cfgs):
            for _ in range(steps):
                cfg.integrate_inplace(solve_ik(cfg, host_tasks[b], dt, barriers=bars), dt)
            assert np.abs(qd[b] - cfg.q).max() < 1e-8
        ro.free()
        if placement == "identity":  # a box only: the two-launch path (step kernel + solve) takes it too
            ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-1, fused=True, floating_base_limit=limit)
            ro.set_targets(targets)
            ro.step(integrate=False)
            dq2, st2, _ = ro.last_step()
            for b in range(B):
                v = solve_ik(Configuration(model, q0[b]), host_tasks[b], dt)
                assert st2[b] == 0 and np.abs(dq2[b] / dt - v).max() < 1e-8
            ro.free()
    finally:
        model.floating_base_velocity_limit = None


@pytest.mark.parametrize("which", [0, 1])
def test_fused_fk_frame_tasks_equal_separate_launches(api, which):
    """pinkhip_fk_frame_tasks_device writes the same e / J rows into the packed streams as
    pinkhip_fk_device followed by one pinkhip_frame_task_strided_device per task."""
    model, frames = _models()[which]
    rng = np.random.default_rng(30 + which)
    B = 5
    q0 = _random_q(model, B, rng)
    if which == 1:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    specs = [(f, 1.0, 0.5, 1.0, 1e-3) for f in frames]
    targets = np.zeros((B, len(frames), 12))
    for b in range(B):
        cfg = Configuration(model, q0[b])
        for i, f in enumerate(frames):
            tgt = cfg.get_transform_frame_to_world(f) * SE3(exp3(0.4 * rng.normal(size=3)), 0.1 * rng.normal(size=3))
            targets[b, i] = pose12(tgt)
    rows = []
    for fused in (True, False):
        ro = DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=1e-2, fused=fused)
        ro.set_targets(targets)
        ro.step()
        api.sync()
        e = np.zeros((B, ro.K))
        J = np.zeros((B, ro.Kd, ro.nv))
        api.get(e, ro.d_e)
        api.get(J, ro.d_J)
        rows.append((e, J, ro.frame_poses()))
        ro.free()
    assert np.abs(rows[0][0] - rows[1][0]).max() < 1e-13
    assert np.abs(rows[0][1] - rows[1][1]).max() < 1e-13
    assert np.abs(rows[0][2] - rows[1][2]).max() < 1e-14
    # and the rows are the host FrameTask's (frame_task.py:176-227)
    for b in range(B):
        cfg = Configuration(model, q0[b])
        for i, f in enumerate(frames):
            t = FrameTask(f, 1.0, 0.5)
            t.set_target(SE3(targets[b, i, :9].reshape(3, 3), targets[b, i, 9:]))
            assert np.abs(t.compute_error(cfg) - rows[0][0][b, 6 * i:6 * i + 6]).max() < 1e-10
            assert np.abs(t.compute_jacobian(cfg) - rows[0][1][b, 6 * i:6 * i + 6]).max() < 1e-9


@pytest.mark.parametrize("mode", [True, "kernel"])
def test_failed_solves_are_not_integrated_and_stay_visible(api, mode):
    """A robot whose QP fails (here: iteration cap of one active-set step) must keep its configuration -- the
    reference raises NoSolutionFound before integrating (pink/solve_ik.py:271-275) -- and the failure must
    survive later steps (first failure is sticky); run() raises listing those robots."""
    from pink_amd.exceptions import NoSolutionFound, NotWithinConfigurationLimits

    model, frames = _models()[0]
    rng = np.random.default_rng(77)
    B, dt = 6, 5e-3
    q0 = _random_q(model, B, rng) * 0.5 + 0.5 * np.tile(model.neutral(), (B, 1))
    specs = [(f, 1.0, 0.5, 1.0, 1e-3) for f in frames]
    targets = np.zeros((B, len(frames), 12))
    for b in range(B):
        cfg = Configuration(model, q0[b])
        for i, f in enumerate(frames):
            # robots 0..2: far targets (velocity limits become active: more than one active-set step);
            # robots 3..5: target = current pose (no active constraint, solved without any step)
            far = SE3(np.eye(3), (2.0 if b < 3 else 0.0) * np.ones(3))
            targets[b, i] = pose12(cfg.get_transform_frame_to_world(f) * far)
    ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=None, max_iter=1, fused=mode)
    ro.set_targets(targets)
    with pytest.raises(NoSolutionFound) as info:
        ro.run(3)
    idx, status, step = ro.failures()
    assert np.array_equal(info.value.indices, idx) and set(idx) <= {0, 1, 2} and idx.size >= 1
    # STATUS_MAX_ITER, still visible after 3 steps, with the step it happened at (which one depends on how many exchanges
    # the solver needs from ITS starting basis: the principal pivoting of round 6 starts from a guessed active set and
    # may get through a first step that Goldfarb-Idnani's start at the unconstrained minimum did not)
    assert (status == 1).all() and (step >= 0).all() and (step <= 2).all()
    q = ro.configurations()
    first = idx[step == 0]
    assert np.array_equal(q[first], q0[first])  # frozen: the partial iterate was never applied
    ok = np.setdiff1d(np.arange(B), idx)
    assert np.isfinite(q).all() and ok.size >= 3
    # ... and frozen for good: further steps raise again and leave the failed robots where they were
    with pytest.raises(NoSolutionFound):
        ro.run(2)
    idx2, status2, step2 = ro.failures()
    assert set(idx) <= set(idx2) and np.array_equal(ro.configurations()[idx], q[idx])
    assert np.array_equal(step2[np.isin(idx2, idx)], step) and np.array_equal(status2[np.isin(idx2, idx)], status)
    ro.free()
    # initial configurations outside the joint limits are refused like solve_ik's check_limits does
    bad = q0.copy()
    j = int(np.nonzero(np.isfinite(model.upperPositionLimit))[0][0])
    bad[2, j] = model.upperPositionLimit[j] + 0.5
    with pytest.raises(NotWithinConfigurationLimits) as lim:
        DeviceRollout(api, model, bad, specs, dt)
    assert lim.value.instance == 2 and lim.value.joint == j


@pytest.mark.parametrize("which", [0, 1, 2, "tree15", "arm12p", "big30p"])
def test_one_kernel_step_equals_two_launch_step(api, which):
    """pinkhip_rollout_step_device forms the task rows on chip (world twists x per-frame blocks) instead of reading
    them from HBM: after every step dq, status and the configurations must agree with the step-kernel + solve loop
    to round-off (the rows are the same numbers computed in a different order).  The named models (``_edge_models``)
    carry prismatic joints: their columns' world twists go through the kernel's sink as [u; 0]."""
    model, frames = _pick(which)
    rng = np.random.default_rng(50 + (which if isinstance(which, int) else len(which) + model.nv))
    B = 5
    q0 = _random_q(model, B, rng) * 0.6 + 0.4 * np.tile(model.neutral(), (B, 1))
    if model.root_joint is not None:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    specs = [(f, 1.0, 0.5, 0.9, 1e-3) for f in frames]
    targets = np.zeros((B, len(frames), 12))
    for b in range(B):
        cfg = Configuration(model, q0[b])
        for i, f in enumerate(frames):
            targets[b, i] = pose12(cfg.get_transform_frame_to_world(f) * SE3(exp3(0.3 * rng.normal(size=3)), 0.08 * rng.normal(size=3)))
    runs = {}
    for mode in (True, "kernel"):
        ro = DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=5e-2, fused=mode)
        ro.set_targets(targets)
        hist = []
        for _ in range(6):
            ro.step()
            api.sync()
            dq, st, it = ro.last_step()
            hist.append((dq.copy(), st.copy(), ro.configurations().copy()))
        assert ro.fused == (mode if which != 0 else True)
        runs[mode] = hist
        ro.free()
    for (dq_a, st_a, q_a), (dq_b, st_b, q_b) in zip(runs[True], runs["kernel"]):
        assert np.array_equal(st_a, st_b) and (st_a == 0).all()
        assert np.abs(dq_a - dq_b).max() < 1e-11 and np.abs(q_a - q_b).max() < 1e-11


def test_device_path_against_host_path_on_random_robots(api, request):
    """scripts/gpu_fuzz_rollout.py as a test: random chains (fixed / floating base), configurations, FrameTask
    targets, optionally a PositionBarrier and a FloatingBaseVelocityLimit -- the whole-step kernel against the
    host-evaluated path, to 1e-8 scaled by the conditioning of each instance.  The range holds seed 14 (cond(H) = 4e13:
    on the GPU the closing refinement once "corrected" x by 6e7 radians and reported optimal; a step that does not
    contract is no longer applied)."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import gpu_fuzz_rollout as fz

    on_gpu = "gpu" in request.node.name
    for sd in (range(0, 400) if on_gpu else (3, 14, 20, 31, 47, 58)):
        note, err = fz.one(sd)
        assert note in (None, "same failure"), (sd, note)
        assert err <= 1e-8, (sd, err)
        pink_amd.clear_device_cache()


def test_hand_over_with_barrier_rows_reads_the_frame_positions_it_needs(api):
    """Round 3's open item: the whole-step kernel reported "inconsistent" on one or two
    of 6 000 random robots where the host-evaluated path solves -- seeds 24680 and 14626 of scripts/gpu_fuzz_rollout.py
    (cond(H) = 2e13: no posture task, a PositionBarrier row at dt = 1e-3).  Cause: a group handed over to the
    Goldfarb-Idnani code formed the barrier rows from the frame positions the kinematics left in LDS while its own staged
    copy of those rows already overlaid them (12 joints + 3 frames, nv = 12: Gs starts inside frame 0's pose), so the
    right-hand side of the barrier row read back an entry of G.  The positions now live behind the shared area
    (dispatch.h: rollout_tail_doubles).  Reproduced on the emulator once the conditioning estimate routed the instance
    to that code."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import gpu_fuzz_rollout as fz

    for sd in (24680, 14626):
        note, err = fz.one(sd)
        assert note is None, (sd, note)
        assert err <= 1e-8, (sd, err)
        pink_amd.clear_device_cache()


@pytest.mark.parametrize("which", [0, 1, 3])
def test_closed_loop_with_table_tasks_and_a_relative_slot_matches_host_loop(api, which):
    """The tasks the whole-step kernel forms from tables since round 4 -- a JointCouplingTask (constant rows, error
    A (q - q_0) - b from the configuration of THIS step), a DampingTask, a RelativeFrameTask (relative slot: its target
    rides on the root frame's current pose) -- and an AccelerationLimit table, inside the closed loop: every step's rows
    come from the configuration the previous step integrated.  Follows the host loop (solve_ik + integrate_inplace per
    robot) to 1e-8 over the rollout; the 6-dof arm runs the kernel at NV = 12 because the stack needs it."""
    from pink_amd import DampingTask
    from pink_amd.limits import AccelerationLimit, ConfigurationLimit, VelocityLimit
    from pink_amd.tasks import JointCouplingTask, RelativeFrameTask

    model, frames = _models()[which]
    rng = np.random.default_rng(90 + which)
    B, dt, steps = 3, 5e-3, (20 if which != 3 else 10)
    q0 = _random_q(model, B, rng) * 0.5 + 0.5 * np.tile(model.neutral(), (B, 1))
    if model.root_joint is not None:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    cfgs = [Configuration(model, q0[b]) for b in range(B)]
    nj = len(model.joints) - (1 if model.root_joint is not None else 0)
    rel = ("tool0", f"joint_{max(nj // 2, 1)}")
    specs = [(frames[0], 1.0, 0.5, 1.0, 1e-3), (rel, 0.8, 0.3, 0.9, 1e-3)]
    jc = JointCouplingTask(["joint_2", "joint_3"], [1.0, -0.5], 20.0, cfgs[0], lm_damping=5e-7, gain=0.8)
    damp = DampingTask(cost=3e-2)
    root_nv = 6 if model.root_joint is not None else 0
    a_max = np.r_[np.full(root_nv, np.inf), np.full(model.nv - root_nv, 40.0)]
    acc = AccelerationLimit(model, a_max)  # (Delta_q_prev = 0 throughout: the table is the same for every step)
    limits = [ConfigurationLimit(model), VelocityLimit(model), acc]
    targets = np.zeros((B, 2, 12))
    host_tasks = []
    for b, cfg in enumerate(cfgs):
        ft = FrameTask(frames[0], 1.0, 0.5, lm_damping=1e-3, gain=1.0)
        tgt = cfg.get_transform_frame_to_world(frames[0]) * exp6(0.08 * rng.normal(size=6))
        ft.set_target(tgt)
        rt = RelativeFrameTask(rel[0], rel[1], 0.8, 0.3, lm_damping=1e-3, gain=0.9)
        rtg = cfg.get_transform(rel[0], rel[1]) * exp6(0.05 * rng.normal(size=6))
        rt.set_target(rtg)
        targets[b, 0], targets[b, 1] = pose12(tgt), pose12(rtg)
        p = PostureTask(cost=1e-2)
        p.set_target(q0[b])
        host_tasks.append([ft, rt, jc, p, damp])
    acc_tables = np.zeros((3, model.nv))
    acc_tables[0, acc.indices], acc_tables[2, acc.indices] = acc.a_max, acc.has_configuration_limit
    ro = DeviceRollout(api, model, q0, specs, dt, posture_cost=1e-2, fused="kernel",
                       const_tasks=[(jc.A, jc.b, jc.q_0, jc.cost, jc.gain, jc.lm_damping)],
                       diag_tasks=[(root_nv, np.zeros(model.nv - root_nv), damp.cost, damp.gain, damp.lm_damping)],
                       acceleration_limit=acc_tables)
    ro.set_targets(targets)
    ro.run(steps)
    assert ro.fused == "kernel"
    qd = ro.configurations()
    _, st, _ = ro.last_step()
    assert (st == 0).all()
    moved = 0.0
    for b, cfg in enumerate(cfgs):
        for _ in range(steps):
            cfg.integrate_inplace(solve_ik(cfg, host_tasks[b], dt, limits=limits), dt)
        cd = Configuration(model, qd[b])
        for f in (frames[0], rel[0], rel[1]):
            Ta, Tb = cd.get_transform_frame_to_world(f), cfg.get_transform_frame_to_world(f)
            assert np.abs(Ta.translation - Tb.translation).max() < 1e-8 and np.abs(Ta.rotation - Tb.rotation).max() < 1e-8
        moved = max(moved, np.abs(cfg.q - q0[b]).max())
    assert moved > 1e-3
    ro.free()
