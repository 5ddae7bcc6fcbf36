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

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import batch_eval as be
from ._lib import Desc, Problem, Result, c_double_p, c_int32_p
from .batch import DiagonalTaskTerm, pack_terms
from .batch_solver import split_iters
from .exceptions import PinkError

MAX_FRAME_TASKS = 16
MAX_MANIPULABILITY_TASKS = 4
MAX_WHEELS = 8  # include/pinkhip.h: PINKHIP_MAX_WHEELS


def plan(kin_model, slots: Sequence, constraints) -> Optional[List[int]]:
    """Indices of the FrameTask slots when the hybrid route serves this stack, else ``None``: at least one FrameTask,
    at most one ComTask on a model that carries mass (two or more: the host evaluates them), at most four
    ManipulabilityTask slots (each with one frame, mask, reference frame and rate for the whole batch), at most eight
    RollingTask / OmniwheelTask slots (each with one class, hub, floor, radius, gain, cost and lm_damping for the whole batch),
    every other task of a
    class whose batched evaluator yields a diagonal term; equality constraints (slots of ``constraints=``) made of
    FrameTasks / RelativeFrameTasks."""
    from .tasks.com_task import ComTask
    from .tasks.frame_task import FrameTask
    from .tasks.linear_holonomic_task import JointVelocityTask
    from .tasks.manipulability_task import ManipulabilityTask
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
    coms = [k for k, col in enumerate(slots) if type(col[0]) is ComTask]
    if len(coms) > 1 or (coms and not (kin_model.total_mass > 0.0 and len(kin_model.joints) <= 64)):
        return None
    manips = manipulability_slots(slots)
    if len(manips) > MAX_MANIPULABILITY_TASKS or (manips and len(kin_model.joints) > 64):
        return None
    for k in manips:  # (a per-instance list that differs in frame / mask / reference frame / rate / gain / cost: the host route, as frame slots)
        if any(type(t) is not ManipulabilityTask for t in slots[k]) or not be.manipulability_slot_is_uniform(slots[k], with_weights=True):
            return None
    wheels = rolling_slots(slots)
    if len(wheels) > MAX_WHEELS or (wheels and len(kin_model.joints) > 64):
        return None
    for k in wheels:  # (a per-instance list that differs in class / hub / floor / radius / gain / cost: the host route)
        if not be.rolling_slot_is_uniform(slots[k], with_weights=True):
            return None
    for k, col in enumerate(slots):
        if k not in frames and k not in coms and k not in manips and k not in wheels and type(col[0]) not in (PostureTask, DampingTask, LowAccelerationTask, JointVelocityTask):
            return None
    return frames


def com_slot(slots: Sequence) -> Optional[int]:
    """Index of the ComTask slot of a stack :func:`plan` accepted, or ``None``."""
    from .tasks.com_task import ComTask

    return next((k for k, col in enumerate(slots) if type(col[0]) is ComTask), None)


def manipulability_slots(slots: Sequence) -> List[int]:
    """Indices of the ManipulabilityTask slots of a stack, in stack order."""
    from .tasks.manipulability_task import ManipulabilityTask

    return [k for k, col in enumerate(slots) if type(col[0]) is ManipulabilityTask]


def rolling_slots(slots: Sequence) -> List[int]:
    """Indices of the RollingTask / OmniwheelTask slots of a stack, in stack order."""
    from .tasks.rolling_task import OmniwheelTask, RollingTask

    return [k for k, col in enumerate(slots) if type(col[0]) in (RollingTask, OmniwheelTask)]


def wheel_tables(tasks) -> tuple:
    """``(frames, kinds, radii)`` of the wheels ``tasks`` for ``pinkhip_rolling_tasks_device``: the ``(hub, floor)`` pairs that
    become the relative slots of a device model, 0 (rolling) / 1 (omniwheel), and the radii."""
    from .tasks.rolling_task import OmniwheelTask

    return (tuple((t.hub_frame, t.floor_frame) for t in tasks), [1 if type(t) is OmniwheelTask else 0 for t in tasks],
            [float(t.wheel_radius) for t in tasks])


def device_barriers(model, barriers, api) -> Optional[list]:
    """The barriers of a call in the order their rows take on the device -- Pink's, the SelfCollisionBarrier last -- when
    ``pinkhip_barrier_rows_device`` forms ALL of them: the barriers the whole-step kernel forms
    (:func:`pink_amd.solve_ik._barriers_declined`: PositionBarriers with the identity class-K function, BodySphericalBarriers,
    at most one SelfCollisionBarrier of sphere pairs with one gain, none with a safe displacement of its own) on frames of the
    model, a solver that has the call, at most 64 joints and ``PINKHIP_MAX_MD`` rows.  Else ``None``: the host evaluates
    every barrier, as before."""
    from .solve_ik import _barriers_declined

    barriers = list(barriers or ())
    if not barriers or not hasattr(api, "barrier_rows") or len(getattr(model, "joints", ())) > 64:
        return None
    if _barriers_declined(model, barriers, api, "barrier_rows") is not None:
        return None
    names = {fr.name for fr in getattr(model, "frames", ())}
    if any(f not in names for bar in barriers if not hasattr(bar, "distance_query")
           for f in (tuple(bar.frames) if hasattr(bar, "frames") else (bar.frame,))):
        return None  # (an unknown frame: the host evaluation raises what it raises)
    if sum(int(bar.dim) for bar in barriers) > MAX_BARRIER_ROWS:
        return None
    sc = [bar for bar in barriers if hasattr(bar, "distance_query")]
    return [bar for bar in barriers if bar not in sc] + sc


MAX_BARRIER_ROWS = 64  # include/pinkhip.h: PINKHIP_MAX_MD


class HybridState:
    """Device buffers and model tables of one call shape (kept by :func:`pink_amd.solve_ik.solve_ik_batch` like the
    device-resident states)."""

    def __init__(self, api, model, frames: Sequence[str], B: int):
        from .rollout import ModelArrays

        self.api, self.model, self.B = api, model, int(B)
        self.arrays = ModelArrays(model, list(frames))
        self.dmodel = api.model_create(self.arrays.desc)
        self.bufs = {}
        self.cframes, self.carrays, self.cmodel = None, None, None  # device model of the equality constraints' frames
        self.dcom, self.com_key = None, None  # device copy of the model's mass tables (a ComTask slot)
        self.mframes, self.marrays, self.mmodel = None, None, None  # device model of the ManipulabilityTask slots' frames
        self.rframes, self.rarrays, self.rmodel = None, None, None  # device model of the wheels' (hub, floor) slots
        self.bframes, self.barrays, self.bmodel = None, None, None  # device model of the barriers' frames
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

    def _frames_model(self, p: str, frames) -> int:
        """Device model whose frame slots are ``frames``, behind the attributes ``<p>frames`` / ``<p>arrays`` / ``<p>model``;
        built anew when the frames change."""
        frames = tuple(frames)
        if getattr(self, p + "frames") != frames:
            from .rollout import ModelArrays

            self._destroy_frames_model(p)
            arrays = ModelArrays(self.model, list(frames))
            setattr(self, p + "arrays", arrays)  # (kept: the descriptor points into its arrays)
            setattr(self, p + "model", self.api.model_create(arrays.desc))
            setattr(self, p + "frames", frames)
        return getattr(self, p + "model")

    def _destroy_frames_model(self, p: str) -> None:
        if getattr(self, p + "model") is not None:
            self.api.model_destroy(getattr(self, p + "model"))
            setattr(self, p + "model", None)
            setattr(self, p + "frames", None)

    def manipulability_model(self, frames) -> int:
        """Device model whose frame slots are the frames of the ManipulabilityTask slots (the frame-task model's slots each
        own six rows of the frame kernel)."""
        return self._frames_model("m", frames)

    def rolling_model(self, frames) -> int:
        """Device model whose slots are the ``(hub, floor)`` pairs of the RollingTask / OmniwheelTask slots: relative slots,
        frame = hub, root = floor."""
        return self._frames_model("r", frames)

    def barrier_model(self, frames) -> int:
        """Device model whose frame slots are the frames of the PositionBarriers / BodySphericalBarriers."""
        return self._frames_model("b", frames)

    def barrier_tables(self, bars, dt: float):
        """``(model, rows, pairs, sizes, safe gains)`` of ``pinkhip_barrier_rows_device`` for the barriers ``bars``
        (:func:`device_barriers`): the device model of their frames, the ``pinkhip_barrier_rows`` / ``pinkhip_sphere_pairs``
        structs on device tables (either may be ``None``), rows and safe-displacement gain per barrier."""
        from ._lib import BarrierRowsArgs
        from .rollout import barrier_row_tables, sphere_pair_tables, sphere_pairs_args

        sc = next((bar for bar in bars if hasattr(bar, "distance_query")), None)
        frames = []
        for bar in bars:
            for f in (() if bar is sc else tuple(bar.frames) if hasattr(bar, "frames") else (bar.frame,)):
                if f not in frames:
                    frames.append(f)
        tables, sizes, bsafe = barrier_row_tables(bars, lambda name, what: frames.index(name), sc)
        model = self.barrier_model(frames) if frames else self.dmodel  # (sphere pairs alone ride on joints: any model of the robot)
        up = lambda name, a: (self.api.put(self.buf(name, a.nbytes), a), self.bufs[name][0])[1]  # noqa: E731
        rows = None
        if tables[0]:
            rows = BarrierRowsArgs()
            rows.n_rows = len(tables[0])
            rows.frame, rows.axis, rows.sign, rows.bound, rows.gain, rows.frame2 = (
                up("bar%d" % i, np.ascontiguousarray(v, dtype=t))
                for i, (v, t) in enumerate(zip(tables, (np.int32, np.int32, np.float64, np.float64, np.float64, np.int32))))
        pairs = None
        if sc is not None:
            host = sphere_pair_tables(self.model, sc.distance_query.pairs)
            pairs = sphere_pairs_args([up("pairs%d" % i, a) for i, a in enumerate(host)], host, sc)
        return model, rows, pairs, sizes, bsafe

    def constraint_model(self, frames) -> int:
        return self._frames_model("c", frames)

    def buf(self, name: str, nbytes: int) -> int:
        have = self.bufs.get(name)
        if have is None or have[1] < nbytes:
            if have is not None:
                self.api.release(have[0])
            have = (self.api.alloc(max(int(nbytes), 8)), int(nbytes))
            self.bufs[name] = have
        return have[0]

    def free(self) -> None:
        for ptr, _ in self.bufs.values():
            self.api.release(ptr)
        self.bufs = {}
        self._destroy_frames_model("c")
        if self.dcom is not None:
            self.api.com_destroy(self.dcom)
            self.dcom = None
        self._destroy_frames_model("m")
        self._destroy_frames_model("r")
        self._destroy_frames_model("b")
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
    kc = com_slot(slots)
    ccol = None if kc is None else slots[kc]
    nc = 0 if ccol is None else 1
    km = manipulability_slots(slots)
    mcols = [slots[k] for k in km]
    nm = len(mcols)
    kr = rolling_slots(slots)
    rcols = [slots[k] for k in kr]
    rwidths = [len(col[0].rows) for col in rcols]
    nr = sum(rwidths)
    diag = [be.task_term(kq, col, None) for k, col in enumerate(slots) if k not in frame_slots and k != kc and k not in km and k not in kr]
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
    # the FrameTask part of the descriptor: one dense task of six rows per slot, in slot order
    fcols = [slots[k] for k in frame_slots]
    for col in fcols:  # (gain / lm_damping are read off the first task of a slot: the same refusal as the host route)
        be._check_slot(col)
    # ... and the ComTask's: one dense task of three rows behind them
    if ccol is not None:
        be._check_slot(ccol)
        ctarget = np.ascontiguousarray(be.com_targets(ccol, B), dtype=np.float64)
    # ... and one dense task of one row per ManipulabilityTask slot behind those
    for col in mcols:
        be._check_slot(col)
    # ... and one dense task of three (Rolling) or two (Omniwheel) rows per wheel slot behind those
    for col in rcols:
        be._check_slot(col)
    Kd = 6 * nf + 3 * nc + nm + nr
    K = Kd + b0.K
    fcost = [be._costs(col, 6) for col in fcols]
    widths = [6] * nf + [3] * nc + [1] * nm + rwidths
    if ccol is not None:
        fcost.append(be._costs(ccol, 3))
        fcols = fcols + [ccol]
    for col in mcols:
        fcost.append(be._costs(col, 1))
        fcols = fcols + [col]
    for col, w in zip(rcols, rwidths):
        c = be._costs(col, w)
        fcost.append(1.0 if c is None else c)  # (cost=None: identity weights, pink/tasks/task.py:148-156)
        fcols = fcols + [col]
    batched = b0.cost.ndim == 2 or any(np.ndim(c) == 2 for c in fcost)
    if batched:
        cost = np.concatenate([np.broadcast_to(np.asarray(c, dtype=float), (B, w)) for c, w in zip(fcost, widths)]
                              + [np.broadcast_to(b0.cost, (B, b0.K))], axis=1)
    else:
        cost = np.concatenate([np.broadcast_to(np.asarray(c, dtype=float), (w,)) for c, w in zip(fcost, widths)] + [b0.cost])
    cost = np.ascontiguousarray(cost)
    e_full = np.zeros((B, K))  # (the kernel overwrites the FrameTask rows: one contiguous upload instead of a strided one)
    e_full[:, Kd:] = b0.e
    # (a RelativeFrameTask's target lives in its root frame: a relative slot of the device model, include/pinkhip.h)
    targets = np.ascontiguousarray(np.stack([_targets_of(col, B) for col in fcols[:nf]], axis=1))  # [B, nf, 12]
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    nw = len(rcols)
    task_rows = i32([6 * i for i in range(nf + 1)] + [6 * nf + 3] * nc + [6 * nf + 3 * nc + i + 1 for i in range(nm)]
                    + [6 * nf + 3 * nc + nm + int(r) for r in np.cumsum(rwidths)] + [Kd + int(r) for r in b0.task_rows[1:]])
    task_kind = i32([0] * (nf + nc + nm + nw) + list(b0.task_kind))
    task_col0 = i32([0] * (nf + nc + nm + nw) + list(b0.task_col0))
    gain = f64([col[0].gain for col in fcols] + list(b0.gain))
    lm = f64([col[0].lm_damping for col in fcols] + list(b0.lm_damping))
    md, n_bar = b0.md, int(b0.barrier_safe_gain.size)
    brow, bsafe = i32(b0.barrier_rows), f64(b0.barrier_safe_gain if b0.barrier_safe_gain.size else [0.0])
    if dbars is not None:  # their rows behind the equality and limit rows b0 holds, one group per barrier
        bmodel, brows, bpairs, sizes, safe = state.barrier_tables(dbars, dt)
        brow, bsafe, n_bar = i32([b0.md + int(r) for r in np.cumsum([0] + sizes)]), f64(safe), len(dbars)
        md = b0.md + int(sum(sizes))
    d = Desc()
    d.B, d.nv, d.T, d.Kd, d.K, d.md, d.n_eq = B, nv, nf + nc + nm + nw + len(diag), Kd, K, md, n_eq
    d.task_rows, d.task_kind, d.task_col0 = (a.ctypes.data_as(c_int32_p) for a in (task_rows, task_kind, task_col0))
    d.gain, d.lm_damping = gain.ctypes.data_as(c_double_p), lm.ctypes.data_as(c_double_p)
    d.n_barriers = n_bar
    d.barrier_rows, d.barrier_safe_gain = brow.ctypes.data_as(c_int32_p), bsafe.ctypes.data_as(c_double_p)
    d.damping, d.dt, d.cost_is_batched, d.max_iter = float(damping), float(dt), int(batched), int(max_iter)
    # device side
    s = state
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
    if ccol is not None:  # the three ComTask rows behind the frame rows of the same streams
        d_ct = s.buf("com_target", ctarget.nbytes)
        api.put(d_ct, ctarget)
        api.com_task(s.dmodel, s.com_tables(), B, d_q, d_ct, ctarget.ndim == 2, d_e, K, d_J, Kd * nv, 6 * nf)
    if nm:  # one row per ManipulabilityTask slot behind the centre-of-mass rows, one launch each
        mmodel = s.manipulability_model(col[0].frame for col in mcols)
        for i, col in enumerate(mcols):
            t0 = col[0]
            api.manipulability_task(mmodel, B, d_q, i, int(t0.reference_frame), t0.row_mask, float(t0.manipulability_rate), d_e, K,
                                    d_J, Kd * nv, 6 * nf + 3 * nc + i)
    if nw:  # the rows of all wheels behind the manipulability rows, ONE launch: the world poses are composed once
        frames, kinds, radii = wheel_tables([col[0] for col in rcols])
        api.rolling_tasks(s.rolling_model(frames), B, d_q, list(range(nw)), kinds, radii, d_e, K, d_J, Kd * nv, 6 * nf + 3 * nc + nm)
    if n_eq:
        # the same kernel on the constraints' frames, writing J into the leading rows of Gd and e into those of hd (row
        # pitches md nv and md); hd then becomes -gain e on the host: [B, md] doubles go home and back
        cmodel = s.constraint_model(_frame_name(col[0]) for col in ccols)
        ctargets = np.ascontiguousarray(np.stack([_targets_of(col, B) for col in ccols], axis=1))
        d_Tc = s.buf("Ttc", ctargets.nbytes)
        api.put(d_Tc, ctargets)
        api.fk_frame_tasks(cmodel, B, d_q, d_Tc, None, p.hd, md, p.Gd, md * nv)
        api.sync()
        hd = np.empty((B, md))
        api.get(hd, p.hd)
        for k, col in enumerate(ccols):
            hd[:, 6 * k:6 * k + 6] *= -float(col[0].gain)
        api.put(p.hd, hd)
    if dbars is not None:  # ONE launch: the rows of every barrier behind the equality and limit rows
        api.barrier_rows(bmodel, B, d_q, dt, brows, bpairs, p.Gd, md * nv, p.hd, md, b0.md)
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
