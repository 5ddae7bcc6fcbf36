"""The layout of the dense-row groups (pink_amd/row_groups.py), pinned to numbers derived by hand, through both callers:
solve_ik_batch on the hybrid route and DeviceRollout with fused=True / fused=False.

The stack, on the 12-joint tree of tests/manipulability_cases.py (every joint carries mass; "hand" and "foot" hang on
all-revolute paths and serve as the two hubs), B = 5:

    task                       rows   row0
    FrameTask "hand"              6      0      fk_frame_tasks / the step kernel
    ComTask                       3      6      com_task
    ManipulabilityTask "hand"     1      9      manipulability_task
    ManipulabilityTask "foot"     1     10      manipulability_task
    RollingTask  foot on deep     3     11      rolling_tasks, ONE launch for both wheels
    OmniwheelTask hand on foot    2     14
    PostureTask                  12     16      (diagonal: behind the Kd = 16 dense rows; K = 28, sJ = 16 nv = 192)

    PositionBarrier "hand" with p_min and p_max on x (2 rows), BodySphericalBarrier (1 row): the last three of the md dense
    rows on the hybrid route (barrier row0 = md - 3), all of them in the rollout (md = 3, barrier row0 = 0).

A rollout takes the frames of its barriers from the slots of its frame tasks, and the numbers above leave it one slot: the
BodySphericalBarrier joins "hand" to itself with d_min = 0 and no safe-displacement regulariser (its weight is the gain over
|J_h|^2, and J_h = 0 here) -- the row 0 dq <= 0, which holds for every dq and moves no minimiser; what is pinned here is where
the row lies, not what it says.  The PositionBarrier beside it is an ordinary one.

A thin recorder around the solver notes the kernel methods in the order they are called with their integer sE, sJ and row0
arguments, and what solve_raw finds in the descriptor, then delegates."""
import numpy as np
import pytest

import pink_amd
from pink_amd import (ComTask, Configuration, ConfigurationBatch, FrameTask, ManipulabilityTask, OmniwheelTask, PostureTask, ReferenceFrame,
                      RollingTask, solve_ik_batch)
from pink_amd.barriers import BodySphericalBarrier, PositionBarrier
from pink_amd.lie import exp6
from pink_amd.runtime import set_default_solver
from tests.manipulability_cases import cond_A, models
from tests.row_kernel_kit import with_row_kernels

B, DT, NV = 5, 5e-3, 12
# name -> positions of (sE, sJ, row0) among the arguments (barrier_rows: the pitches of Gd and hd -- md nv, md -- and row0)
ROW_CALLS = {"fk_frame_tasks": (6, 8, None), "com_task": (7, 9, 10), "manipulability_task": (8, 10, 11), "rolling_tasks": (7, 9, 10),
             "barrier_rows": (9, 7, 10)}
OTHER_CALLS = ("step_kernel", "fk", "frame_task_strided", "limits_posture", "solve_raw")
ROWS = [("com_task", 6), ("manipulability_task", 9), ("manipulability_task", 10), ("rolling_tasks", 11)]


class Recorder:
    """The solver behind it, with ``calls``: ``(name, sE, sJ, row0)`` of every row kernel, ``(name,)`` of the other launches,
    and ``descs``: ``(Kd, K, md, task_rows[:T + 1])`` of every solve_raw."""

    def __init__(self, api, without=()):
        self._api, self._without, self.calls, self.descs = api, without, [], []

    def __getattr__(self, name):
        if name in self._without:
            raise AttributeError(name)
        fn = getattr(self._api, name)
        if name not in ROW_CALLS and name not in OTHER_CALLS:
            return fn

        def noted(*args, **kw):
            self.calls.append((name,) + tuple(None if i is None else int(args[i]) for i in ROW_CALLS.get(name, ())))
            if name == "solve_raw":
                d = args[0]
                self.descs.append((d.Kd, d.K, d.md, [int(d.task_rows[i]) for i in range(d.T + 1)]))
            return fn(*args, **kw)

        return noted

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    s = Recorder(with_barrier_rows(with_row_kernels(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))))
    set_default_solver(s)
    yield s
    pink_amd.clear_device_cache()
    set_default_solver(None)


def with_barrier_rows(api):
    from tests.barrier_rows_cases import with_barrier_rows as bind

    return bind(api)


def _stack(n_manip=2, n_wheels=2):
    model, _ = models()["tree12"]
    rng = np.random.default_rng(3)
    manip = [dict(cost=0.8, gain=0.6, lm_damping=1e-3, manipulability_rate=0.2),
             dict(cost=0.3, mask="position", reference_frame=ReferenceFrame.WORLD, manipulability_rate=-0.1)]
    mframes = ["hand", "foot"]
    # (the regular band of tests/manipulability_cases.py, as tests/test_manipulability_routes.py: the routes form A = J J^T
    # in different orders and differ by eps cond(A))
    q = rng.uniform(-1.0, 1.0, size=(64 * B, model.nq))
    ok = np.ones(len(q), bool)
    for f, spec in zip(mframes, manip):
        ok &= cond_A(model, f, spec.get("reference_frame", ReferenceFrame.LOCAL), spec.get("mask"), q) <= 1e4
    q = q[ok][:B]
    assert q.shape[0] == B
    cfgs = [Configuration(model, q[b]) for b in range(B)]
    ft = FrameTask("hand", 1.0, 0.5, lm_damping=1e-3, gain=0.9)
    R, t = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b, c in enumerate(cfgs):
        T = c.get_transform_frame_to_world("hand") * exp6(0.05 * rng.normal(size=6))
        R[b], t[b] = T.rotation, T.translation
    ft.set_target_poses(R, t)
    com = ComTask([1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
    com.set_target(np.mean([c.center_of_mass() for c in cfgs], axis=0) + [0.01, -0.02, 0.03])
    mts = [ManipulabilityTask(mframes[i % 2], model, **{**manip[i % 2], "manipulability_rate": 0.2 - 0.05 * i}) for i in range(n_manip)]
    wheels = [(OmniwheelTask if i % 2 else RollingTask)("hand" if i % 2 else "foot", "foot" if i % 2 else "deep", 0.07 + 0.01 * i,
                                                        [0.8, 1.5] if i % 2 else [1.0, 0.5, 2.0], gain=0.7, lm_damping=1e-3) for i in range(n_wheels)]
    po = PostureTask(cost=5e-2)
    po.set_target(model.neutral())
    # one p_min and one p_max row on x, the latter 2 mm in front of the foremost hand
    x = np.array([c.get_transform_frame_to_world("hand").translation[0] for c in cfgs])
    barriers = [PositionBarrier("hand", indices=[0], p_min=np.array([x.min() - 0.5]), p_max=np.array([x.max() + 0.002]), gain=np.array([1.0, 0.8])),
                BodySphericalBarrier(("hand", "hand"), d_min=0.0, gain=1.5, safe_displacement_gain=0.0)]
    return model, q, cfgs, ft, com, mts, wheels, po, barriers


def test_hybrid_route_lays_the_rows_out(api):
    model, q, cfgs, ft, com, mts, wheels, po, barriers = _stack()
    tasks = [ft, com] + mts + wheels + [po]
    V = solve_ik_batch(ConfigurationBatch(model, q), tasks, DT, barriers=barriers, device_kinematics="frame_rows")
    stats = pink_amd.last_solve_stats()
    assert stats["route"] == "hybrid" and stats["barrier_rows"] == "device" and stats["failed"] == 0 and stats["instances"] == B
    assert api.names() == ["fk_frame_tasks", "com_task", "manipulability_task", "manipulability_task", "rolling_tasks", "barrier_rows", "solve_raw"]
    (Kd, K, md, task_rows), = api.descs
    assert (Kd, K) == (16, 28) and task_rows == [0, 6, 9, 10, 11, 14, 16, 28]
    assert api.calls[0] == ("fk_frame_tasks", K, 16 * NV, None)
    assert api.calls[1:5] == [(name, K, 16 * NV, row0) for name, row0 in ROWS]
    assert api.calls[5] == ("barrier_rows", md, md * NV, md - 3)
    V_host = solve_ik_batch(ConfigurationBatch(model, q), tasks, DT, barriers=barriers, device_kinematics=False)
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated" and pink_amd.last_solve_stats()["failed"] == 0
    err = np.abs(V - V_host).max() * DT
    print(f"hybrid vs all-host max|dq| difference {err:.3e}")
    assert err < 1e-10 and np.abs(V).max() * DT > 1e-4


def test_rollout_lays_the_rows_out(api):
    from pink_amd.rollout import DeviceRollout, pose12

    model, q, cfgs, ft, com, mts, wheels, po, barriers = _stack()
    # the FrameTask and the PostureTask of the hybrid stack as the rollout takes them
    specs = [(ft.frame, 1.0, 0.5, ft.gain, ft.lm_damping)]
    targets = ft.poses12()[:, None, :]
    head = {True: ["step_kernel"], False: ["fk", "frame_task_strided", "limits_posture"]}
    runs = {}
    for fused in (True, False):
        ro = DeviceRollout(api, model, q, specs, DT, posture_cost=5e-2, q_posture=model.neutral(), fused=fused, com_task=com,
                           manipulability_tasks=mts, rolling_tasks=wheels, position_barriers=barriers)
        assert (ro.Kd, ro.K, ro.md) == (16, 28, 3)
        ro.set_targets(targets)
        del api.calls[:], api.descs[:]
        ro.step()
        assert api.names() == head[fused] + [name for name, _ in ROWS] + ["barrier_rows", "solve_raw"]
        n = len(head[fused])
        assert api.calls[n:n + 4] == [(name, 28, 16 * NV, row0) for name, row0 in ROWS]
        assert api.calls[n + 4] == ("barrier_rows", 3, 3 * NV, 0)
        assert api.descs == [(16, 28, 3, [0, 6, 9, 10, 11, 14, 16, 28])]
        traj = [ro.configurations()]
        for _ in range(2):
            ro.step()
            traj.append(ro.configurations())
        _, st, _ = ro.last_step()
        assert (st == 0).all()
        ro.free()
        runs[fused] = np.array(traj)
    assert np.abs(runs[True] - runs[False]).max() < 1e-11  # (as the launch variants of tests/test_rollout.py)
    assert np.abs(runs[True][-1] - q).max() > 1e-5  # (the robots moved)


def test_one_question_admits_a_stack_for_both_callers(api):
    """What a kind refuses, the rollout raises and hybrid.plan declines -- the reason comes from one call."""
    from pink_amd import hybrid, row_groups
    from pink_amd.rollout import DeviceRollout

    model, q, cfgs, ft, com, mts, wheels, po, barriers = _stack(n_manip=5, n_wheels=9)
    specs = [("hand", 1.0, 0.5, 0.9, 1e-3)]
    for kw, tasks, kind, word in ((dict(manipulability_tasks=mts), mts, row_groups.ManipulabilityGroup, "at most four"),
                                  (dict(rolling_tasks=wheels), wheels, row_groups.WheelGroup, "at most eight")):
        why = kind.declined(model, tasks, api)
        assert why is not None and word in why and kind.declined(model, tasks[:kind.max_tasks], api) is None
        with pytest.raises(ValueError) as ex:
            DeviceRollout(api, model, q, specs, DT, posture_cost=5e-2, fused=True, **kw)
        assert str(ex.value) == why
        solve_ik_batch(ConfigurationBatch(model, q), [ft] + tasks + [po], DT, device_kinematics="frame_rows")
        assert pink_amd.last_solve_stats()["route"] == "host-evaluated"
        solve_ik_batch(ConfigurationBatch(model, q), [ft] + tasks[:kind.max_tasks] + [po], DT, device_kinematics="frame_rows")
        assert pink_amd.last_solve_stats()["route"] == "hybrid"
    # a solver without rolling_tasks
    slots = [[t] * B for t in [ft] + wheels[:2] + [po]]
    bare = Recorder(api._api, without=("rolling_tasks",))
    assert hybrid.plan(model, slots, [], api) == [0] and hybrid.plan(model, slots, [], bare) is None
    assert "pinkhip_rolling_tasks_device" in row_groups.WheelGroup.declined(model, wheels[:2], bare)
    pink_amd.clear_device_cache()
    set_default_solver(bare)
    solve_ik_batch(ConfigurationBatch(model, q), [ft] + wheels[:2] + [po], DT, device_kinematics="frame_rows")
    assert pink_amd.last_solve_stats()["route"] == "host-evaluated" and "rolling_tasks" not in bare.names()
