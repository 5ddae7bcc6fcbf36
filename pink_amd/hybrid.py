"""Host-evaluated route with the FrameTask rows formed on the device.

A task stack the whole-step kernel does not form on chip (``pink_amd/solve_ik.py``: anything beyond FrameTasks + one
PostureTask under the default limits) used to be evaluated entirely on the host: forward kinematics, body Jacobians,
``log6`` / ``Jlog6`` and the 6 x 6 by 6 x nv products of every FrameTask for the whole batch in NumPy, then ~6 kB per
instance across PCIe.  When every task with a dense Jacobian is a FrameTask or a RelativeFrameTask -- the other tasks of the stack being the
identity-Jacobian ones (PostureTask, DampingTask, LowAccelerationTask, JointVelocityTask: ``pink/tasks/posture_task.py``,
``damping_task.py``, ``low_acceleration_task.py``, ``joint_velocity_task.py``) -- that part needs nothing but ``q`` and
the targets: ``pinkhip_fk_frame_tasks_device`` writes the rows straight into the packed ``J`` / ``e`` streams in HBM
(``pink/tasks/frame_task.py:176-227``), the host only evaluates what is cheap and irregular -- the errors of the
diagonal tasks, the limits (any list: explicit gains, AccelerationLimit, user subclasses), barriers -- and
``pinkhip_solve_device`` stacks and solves.  ``J`` never exists on the host and never crosses PCIe.  Barriers the device forms (:func:`device_barriers`) do not reach the
host either: ``pinkhip_barrier_rows_device`` writes their rows into ``Gd`` / ``hd`` behind the equality and limit rows.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import batch_eval as be
from ._lib import Desc, Problem, Result, c_double_p, c_int32_p
from .batch import DiagonalTaskTerm, pack_terms
from .batch_solver import split_iters
from .exceptions import PinkError
from .row_groups import (KINDS, MAX_BARRIER_ROWS, MAX_MANIPULABILITY_TASKS, MAX_WHEELS, BarrierRows, Layout, ManipulabilityGroup,  # noqa: F401
                         WheelGroup, barrier_frames, barrier_rows_declined, declined, wheel_tables)  # (the limits and wheel_tables: re-exported)

MAX_FRAME_TASKS = 16


def plan(kin_model, slots: Sequence, constraints, api=None) -> Optional[List[int]]:
    """Indices of the FrameTask slots when the hybrid route serves this stack, else ``None``: at least one FrameTask,
    the slots of every kind of :data:`pink_amd.row_groups.KINDS` admitted by that kind on the solver ``api`` (at most one
    ComTask on a model that carries mass -- two or more: the host evaluates them --, at most four ManipulabilityTask slots,
    each with one frame, mask, reference frame and rate for the whole batch, at most eight RollingTask / OmniwheelTask
    slots, each with one class, hub, floor, radius, gain, cost and lm_damping for the whole batch), every other task of a class
    whose batched evaluator yields a diagonal term; equality constraints (slots of ``constraints=``) made of FrameTasks /
    RelativeFrameTasks."""
    from .tasks.frame_task import FrameTask
    from .tasks.linear_holonomic_task import JointVelocityTask
    from .tasks.posture_task import DampingTask, LowAccelerationTask, PostureTask
    from .tasks.relative_frame_task import RelativeFrameTask

    if not hasattr(kin_model, "joints"):
        return None
    for col in constraints or ():  # equality constraints (pink/solve_ik.py:125-149): frame tasks only, one frame per slot
        c0 = col[0]
        if type(c0) not in (FrameTask, RelativeFrameTask):
            return None
        if not getattr(col, "shared", False) and any(
                type(t) is not type(c0) or t.frame != c0.frame or getattr(t, "root", None) != getattr(c0, "root", None) or t.gain != c0.gain
                for t in col):
            return None
    if constraints and len(constraints) > MAX_FRAME_TASKS:
        return None
    frames = [k for k, col in enumerate(slots) if type(col[0]) in (FrameTask, RelativeFrameTask)]
    for k in frames:  # (one frame -- and root -- per slot: the device model holds them)
        t0 = slots[k][0]
        if getattr(slots[k], "shared", False):  # (one task object for the whole batch: nothing to compare)
            continue
        if any(type(t) is not type(t0) or t.frame != t0.frame or getattr(t, "root", None) != getattr(t0, "root", None) for t in slots[k]):
            return None
    if not frames or len(frames) > MAX_FRAME_TASKS:
        return None
    coms, manips, wheels = kslots = group_slots(slots)
    if declined(kin_model, [[slots[k][0] for k in ks] for ks in kslots], api) is not None:
        return None
    for k in manips:  # (a per-instance list that differs in frame / mask / reference frame / rate / gain / cost: the host route, as frame slots)
        if any(type(t) not in ManipulabilityGroup.types for t in slots[k]) or not be.manipulability_slot_is_uniform(slots[k], with_weights=True):
            return None
    for k in wheels:  # (a per-instance list that differs in class / hub / floor / radius / gain / cost: the host route)
        if not be.rolling_slot_is_uniform(slots[k], with_weights=True):
            return None
    dense = set(frames).union(*kslots)
    if any(k not in dense and type(col[0]) not in (PostureTask, DampingTask, LowAccelerationTask, JointVelocityTask) for k, col in enumerate(slots)):
        return None
    return frames


def group_slots(slots: Sequence) -> List[List[int]]:
    """Per kind of :data:`pink_amd.row_groups.KINDS` -- ComTask, ManipulabilityTask, RollingTask / OmniwheelTask -- the indices
    of its slots of a stack, in stack order."""
    return [[k for k, col in enumerate(slots) if type(col[0]) in kind.types] for kind in KINDS]


def device_barriers(model, barriers, api) -> Optional[list]:
    """The barriers of a call in the order their rows take on the device -- Pink's, the SelfCollisionBarrier last -- when
    ``pinkhip_barrier_rows_device`` forms ALL of them: the barriers the whole-step kernel forms
    (:func:`pink_amd.solve_ik._barriers_declined`: PositionBarriers with the identity class-K function, BodySphericalBarriers,
    at most one SelfCollisionBarrier of sphere pairs with one gain, none with a safe displacement of its own) on frames of the
    model, a solver that has the call, at most 64 joints and ``PINKHIP_MAX_MD`` rows.  Else ``None``: the host evaluates
    every barrier, as before."""
    from .solve_ik import _barriers_declined

    barriers = list(barriers or ())
    if not barriers or barrier_rows_declined(model, api) is not None:
        return None
    if _barriers_declined(model, barriers, api, "barrier_rows") is not None:
        return None
    names = {fr.name for fr in getattr(model, "frames", ())}
    if any(f not in names for f in barrier_frames(barriers)):
        return None  # (an unknown frame: the host evaluation raises what it raises)
    if sum(int(bar.dim) for bar in barriers) > MAX_BARRIER_ROWS:
        return None
    sc = [bar for bar in barriers if hasattr(bar, "distance_query")]
    return [bar for bar in barriers if bar not in sc] + sc


class HybridState:
    """Device buffers and model tables of one call shape (kept by :func:`pink_amd.solve_ik.solve_ik_batch` like the
    device-resident states)."""

    def __init__(self, api, model, frames: Sequence[str], B: int):
        from .rollout import ModelArrays

        self.api, self.model, self.B = api, model, int(B)
        self.arrays = ModelArrays(model, list(frames))
        self.dmodel = api.model_create(self.arrays.desc)
        self.bufs = {}
        # further device models by name -- "constraints": the equality constraints' frames; the name of a row group
        # (pink_amd/row_groups.py): the slots of its tasks; "barriers": the barriers' frames -- as (frames, arrays, handle)
        self.models = {}
        self.dcom, self.com_key = None, None  # device copy of the model's mass tables (a ComTask slot)
        self.barrier_rows = None  # where the last call's barrier rows were formed: "device" / "host" / None (no barriers)

    def com_tables(self) -> int:
        """The device mass tables of the model as it is NOW (an edit of a mass or a centre builds them anew)."""
        mass, com = self.model.mass_tables()
        key = (mass.tobytes(), com.tobytes())
        if self.com_key != key:
            if self.dcom is not None:
                self.api.com_destroy(self.dcom)
                self.dcom = None
            self.dcom = self.api.com_create(self.dmodel, mass, com)
            self.com_key = key
        return self.dcom

    def _frames_model(self, name: str, frames) -> int:
        """Device model ``name`` whose frame slots are ``frames`` (an entry ``(frame, root)``: a relative slot); built anew
        when the frames change."""
        frames = tuple(frames)
        if name not in self.models or self.models[name][0] != frames:
            from .rollout import ModelArrays

            self._destroy_frames_model(name)
            arrays = ModelArrays(self.model, list(frames))  # (kept: the descriptor points into its arrays)
            self.models[name] = (frames, arrays, self.api.model_create(arrays.desc))
        return self.models[name][2]

    def _destroy_frames_model(self, name: str) -> None:
        if name in self.models:
            self.api.model_destroy(self.models.pop(name)[2])

    def buf(self, name: str, nbytes: int) -> int:
        have = self.bufs.get(name)
        if have is None or have[1] < nbytes:
            if have is not None:
                self.api.release(have[0])
            have = (self.api.alloc(max(int(nbytes), 8)), int(nbytes))
            self.bufs[name] = have
        return have[0]

    def upload(self, name: str, a: np.ndarray) -> int:
        """Device address of the buffer ``name`` after ``a`` went into it."""
        self.api.put(self.buf(name, a.nbytes), a)
        return self.bufs[name][0]

    def free(self) -> None:
        for ptr, _ in self.bufs.values():
            self.api.release(ptr)
        self.bufs = {}
        for name in list(self.models):
            self._destroy_frames_model(name)
        if self.dcom is not None:
            self.api.com_destroy(self.dcom)
            self.dcom = None
        self.api.model_destroy(self.dmodel)


def solve(state: HybridState, kin_q: np.ndarray, kin, slots: Sequence, frame_slots: List[int], limits, barriers, dt: float,
          damping: float, max_iter: int, constraints: Sequence = ()):
    """One batched solve on the hybrid route; returns ``(dq, status, iters, path)``.  ``kin`` is a callable that
    yields the host :class:`~pink_amd.kinematics_batch.BatchKinematics` -- forward kinematics on the host are only run
    if something asks for them (barriers, limits without a batched evaluator)."""
    api, model, B = state.api, state.model, state.B
    nv, nq, nf = model.nv, model.nq, len(frame_slots)
    kq = _QOnly(model, kin_q, kin)
    # diagonal tasks, limits, barriers: host (vectorised, pink_amd/batch_eval.py)
    kslots = group_slots(slots)
    dense = set(frame_slots).union(*kslots)
    diag = [be.task_term(kq, col, None) for k, col in enumerate(slots) if k not in dense]
    if any(not isinstance(t, DiagonalTaskTerm) for t in diag):
        raise PinkError("hybrid route: a task outside the FrameTasks produced a dense Jacobian")
    lb = np.full((B, nv), -np.inf)
    ub = np.full((B, nv), np.inf)
    dense_rows = []
    for limit in limits:
        rows = be.limit_rows(kq, limit, dt, lb, ub)
        if rows is not None:
            dense_rows.append(rows)
    # barriers: all of them by pinkhip_barrier_rows_device (below; the host only reserves their rows), or all of them here
    dbars = device_barriers(model, barriers, api)
    barrier_terms = [] if dbars is not None else [be.barrier_term(kq, bar) for bar in (barriers or [])]
    state.barrier_rows = "device" if dbars is not None else ("host" if barriers else None)
    # equality constraints made of frame tasks (pink/solve_ik.py:125-149: A = J, b = -gain e): their rows are the leading
    # dense rows of the QP; the device writes them there (below), the host only reserves the space
    ccols = list(constraints or ())
    n_eq = 6 * len(ccols)
    eq = [(np.zeros((B, n_eq, nv)), np.zeros((B, n_eq)))] if n_eq else ()
    b0 = pack_terms(nv, diag, dt, damping, boxes=[(lb, ub)], dense_rows=dense_rows, barriers=barrier_terms, batch_size=B,
                    equality_rows=eq)

    def weights(col, w, none=None):
        # (gain / lm_damping are read off the first task of a slot: the same refusal as the host route)
        be._check_slot(col)
        c = be._costs(col, w)
        return col[0].gain, col[0].lm_damping, none if c is None else c

    # the dense part of the descriptor: one task of six rows per FrameTask slot, in slot order, then the row groups -- three
    # rows of the ComTask, one per ManipulabilityTask slot, three (Rolling) or two (Omniwheel) per wheel slot
    fcols = [slots[k] for k in frame_slots]
    frame_weights = [weights(col, 6) for col in fcols]
    groups = []
    for kind, ks in zip(KINDS, kslots):
        cols = [slots[k] for k in ks]
        # (cost=None of a wheel: identity weights, pink/tasks/task.py:148-156)
        groups.append(kind([col[0] for col in cols], [weights(col, kind.width(col[0]), 1.0 if kind is WheelGroup else None) for col in cols]))
    lay = Layout(frame_weights, groups)
    com = groups[0]
    if com.tasks:
        ctarget = np.ascontiguousarray(be.com_targets(slots[kslots[0][0]], B), dtype=np.float64)
    Kd, K = lay.Kd, lay.Kd + b0.K
    batched = b0.cost.ndim == 2 or any(np.ndim(c) == 2 for c in lay.costs)
    cost = np.ascontiguousarray(np.concatenate(lay.cost_segments((B,) if batched else ())
                                               + [np.broadcast_to(b0.cost, (B, b0.K)) if batched else b0.cost], axis=-1))
    e_full = np.zeros((B, K))  # (the kernel overwrites the FrameTask rows: one contiguous upload instead of a strided one)
    e_full[:, Kd:] = b0.e
    # (a RelativeFrameTask's target lives in its root frame: a relative slot of the device model, include/pinkhip.h)
    targets = np.ascontiguousarray(np.stack([_targets_of(col, B) for col in fcols], axis=1))  # [B, nf, 12]
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    task_rows = i32(lay.task_rows + [Kd + int(r) for r in b0.task_rows[1:]])
    task_kind, task_col0 = i32(lay.task_kind + list(b0.task_kind)), i32(lay.task_col0 + list(b0.task_col0))
    gain, lm = f64(lay.gain + list(b0.gain)), f64(lay.lm_damping + list(b0.lm_damping))
    md, n_bar, s = b0.md, int(b0.barrier_safe_gain.size), state
    brow, bsafe = i32(b0.barrier_rows), f64(b0.barrier_safe_gain if b0.barrier_safe_gain.size else [0.0])
    if dbars is not None:  # their rows behind the equality and limit rows b0 holds, one group per barrier, on a device model
        # of the barriers' own frames (sphere pairs alone ride on joints: any model of the robot)
        frames = barrier_frames(dbars)
        bar = BarrierRows(model, dbars, lambda name, what: frames.index(name))
        bar.upload(s.upload, s._frames_model("barriers", frames) if frames else s.dmodel, b0.md)
        brow, bsafe, n_bar = i32([b0.md + int(r) for r in np.cumsum([0] + bar.sizes)]), f64(bar.safe), len(dbars)
        md = b0.md + int(sum(bar.sizes))
    d = Desc()
    d.B, d.nv, d.T, d.Kd, d.K, d.md, d.n_eq = B, nv, lay.n_tasks + len(diag), Kd, K, md, n_eq
    d.task_rows, d.task_kind, d.task_col0 = (a.ctypes.data_as(c_int32_p) for a in (task_rows, task_kind, task_col0))
    d.gain, d.lm_damping = gain.ctypes.data_as(c_double_p), lm.ctypes.data_as(c_double_p)
    d.n_barriers = n_bar
    d.barrier_rows, d.barrier_safe_gain = brow.ctypes.data_as(c_int32_p), bsafe.ctypes.data_as(c_double_p)
    d.damping, d.dt, d.cost_is_batched, d.max_iter = float(damping), float(dt), int(batched), int(max_iter)
    # device side
    d_q, d_Tt = s.buf("q", 8 * B * nq), s.buf("Tt", 8 * B * nf * 12)
    d_J, d_e, d_cost = s.buf("J", 8 * B * Kd * nv), s.buf("e", 8 * B * K), s.buf("cost", cost.nbytes)
    d_lb, d_ub = s.buf("lb", 8 * B * nv), s.buf("ub", 8 * B * nv)
    d_dq, d_st, d_it = s.buf("dq", 8 * B * nv), s.buf("status", 4 * B), s.buf("iters", 4 * B)
    api.put(d_q, np.ascontiguousarray(kin_q))
    api.put(d_Tt, targets)
    api.put(d_e, e_full)
    api.put(d_cost, cost)
    api.put(d_lb, b0.lb)
    api.put(d_ub, b0.ub)
    p = Problem()
    p.J, p.e, p.cost, p.lb, p.ub = d_J, d_e, d_cost, d_lb, d_ub
    p.Gd = p.hd = p.c_extra = None
    if md:
        p.Gd, p.hd = s.buf("Gd", 8 * B * md * nv), s.buf("hd", 8 * B * md)
        if md == b0.md:
            api.put(p.Gd, b0.Gd)
            api.put(p.hd, b0.hd)
        elif b0.md:  # (equality / limit rows in front of rows the device forms: one upload at the pitch of all rows)
            Gd, hd = np.zeros((B, md, nv)), np.zeros((B, md))
            Gd[:, :b0.md], hd[:, :b0.md] = b0.Gd, b0.hd
            api.put(p.Gd, Gd)
            api.put(p.hd, hd)
    if b0.c_extra is not None:
        p.c_extra = s.buf("c_extra", b0.c_extra.nbytes)
        api.put(p.c_extra, b0.c_extra)
    api.fk_frame_tasks(s.dmodel, B, d_q, d_Tt, None, d_e, K, d_J, Kd * nv)
    # the rows of the groups behind the frame rows of the same streams; the state keeps their device models, and the mass
    # tables as the model has them NOW
    for g in lay.groups:
        g.dmodel = s.dmodel if g.frames() is None else s._frames_model(g.name, g.frames())
    if com.tasks:
        com.dcom, com.d_target, com.batched = s.com_tables(), s.upload("com_target", ctarget), ctarget.ndim == 2
    lay.launch_all(api, B, d_q, d_e, K, d_J, Kd * nv)
    if n_eq:
        # the same kernel on the constraints' frames, writing J into the leading rows of Gd and e into those of hd (row
        # pitches md nv and md); hd then becomes -gain e on the host: [B, md] doubles go home and back
        cmodel = s._frames_model("constraints", (_frame_name(col[0]) for col in ccols))
        ctargets = np.ascontiguousarray(np.stack([_targets_of(col, B) for col in ccols], axis=1))
        d_Tc = s.upload("Ttc", ctargets)
        api.fk_frame_tasks(cmodel, B, d_q, d_Tc, None, p.hd, md, p.Gd, md * nv)
        api.sync()
        hd = np.empty((B, md))
        api.get(hd, p.hd)
        for k, col in enumerate(ccols):
            hd[:, 6 * k:6 * k + 6] *= -float(col[0].gain)
        api.put(p.hd, hd)
    if dbars is not None:  # ONE launch: the rows of every barrier behind the equality and limit rows
        bar.launch(api, B, d_q, dt, p.Gd, md * nv, p.hd, md)
    r = Result()
    r.dq, r.status, r.iters = d_dq, d_st, d_it
    api.solve_raw(d, p, r)
    api.sync()
    dq, st, it = np.empty((B, nv)), np.empty(B, np.int32), np.empty(B, np.int32)
    api.get(dq, d_dq)
    api.get(st, d_st)
    api.get(it, d_it)
    return dq, st, it, split_iters(it)


def _frame_name(task):
    """Entry of a device model's frame list: the frame, or ``(frame, root)`` for a relative slot."""
    return (task.frame, task.root) if hasattr(task, "root") else task.frame


def _targets_of(col, B: int) -> np.ndarray:
    """``[B, 12]`` targets of a frame-task slot (a RelativeFrameTask's lives in its root frame: a relative slot)."""
    if hasattr(col[0], "root"):
        return be._frame_targets(col, B, "transform_target_to_root", "target pose of frame '{0.frame}' in frame '{0.root}' is undefined")
    return be._frame_targets(col, B, "transform_target_to_world", "no target set for frame '{0.frame}'")


class _QOnly:
    """What the batched evaluators read of a :class:`~pink_amd.kinematics_batch.BatchKinematics` when the stack
    needs no forward kinematics on the host (diagonal tasks, joint-space limits): ``q``, the model and the
    manifold difference.  Anything else builds the real thing on first use."""

    def __init__(self, model, q, make):
        self.model, self.q, self.B, self._make, self._kin = model, q, q.shape[0], make, None

    def _full(self):
        if self._kin is None:
            self._kin = self._make()
        return self._kin

    def difference(self, q0, q1, from_v: int = 0):
        from .kinematics_batch import BatchKinematics

        return BatchKinematics.difference(self, q0, q1, from_v)  # (reads the model and q only: no forward kinematics)

    def __getattr__(self, name):
        return getattr(self._full(), name)
