"""The dense rows that stand-alone kernels form behind the FrameTask rows, written once for the two callers that stack
them: the hybrid route of ``solve_ik_batch`` (:mod:`pink_amd.hybrid`) and :class:`pink_amd.rollout.DeviceRollout` with
``fused=True`` / ``fused=False``.

A *row group* is the tasks of one kind -- centre of mass, manipulability, wheel contact -- with what the callers need to
know of it: the rows a task takes, how many the kernel holds, the solver method that forms the rows, why a stack is refused,
the device resources and the launch.  :class:`Layout` puts the groups behind the FrameTask rows in the order of
:data:`KINDS` and hands out every row offset and the dense prefix of the task tables of the QP: nothing else computes an
offset.  The barrier rows go into ``Gd`` / ``hd`` instead of the ``J`` / ``e`` streams: :class:`BarrierRows`.  A new row
kind is a new subclass here and one more entry of :data:`KINDS`."""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .tasks.com_task import ComTask
from .tasks.manipulability_task import ManipulabilityTask, check_revolute_path
from .tasks.rolling_task import OmniwheelTask, RollingTask

MAX_JOINTS = 64  # lanes of a wavefront: the row kernels give every joint of a robot a lane
MAX_MANIPULABILITY_TASKS = 4
MAX_WHEELS = 8  # include/pinkhip.h: PINKHIP_MAX_WHEELS
MAX_BARRIER_ROWS = 64  # include/pinkhip.h: PINKHIP_MAX_MD


def _too_many_joints(model, rows: str) -> Optional[str]:
    if len(getattr(model, "joints", ())) > MAX_JOINTS:
        return f"{rows} on the device need a model of at most {MAX_JOINTS} joints"
    return None


class RowGroup:
    """The tasks of one kind in a stack: ``tasks`` (one per slot: what the device model and the launch read),
    ``weights`` -- ``(gain, lm_damping, cost)`` per task, from the route.  ``row0`` is set by the :class:`Layout`;
    ``dmodel`` by :meth:`create` (resources of the group's own) or by a caller that keeps the device model itself."""

    name = rows = needs = method = kernel = limit = None
    types, max_tasks = (), 1
    out_width = 1  # doubles per robot and task of the output buffer
    out_every_step = False  # (the centre of mass: written beside the rows by every launch of a rollout)

    def __init__(self, tasks: Sequence, weights: Sequence[tuple]):
        self.tasks, self.weights = list(tasks), list(weights)
        self.widths = [self.width(t) for t in self.tasks]
        self.row0 = self.api = self.dmodel = self.arrays = self.out = None

    @classmethod
    def declined(cls, model, tasks: Sequence, api) -> Optional[str]:
        """Why the device does not form the rows of ``tasks`` (``None``: it does).  The rollout raises the reason, the
        hybrid route leaves the stack to the host.  ``api=None``: no solver is asked for its methods."""
        if api is not None and not hasattr(api, cls.method):
            return f"this solver has no {cls.kernel}: {cls.needs} needs it"
        if len(tasks) > cls.max_tasks or any(type(t) not in cls.types for t in tasks):
            return cls.limit
        return cls.model_declined(model) or _too_many_joints(model, cls.rows)

    model_declined = staticmethod(lambda model: None)

    def validate(self, model) -> None:
        """Raise what the model raises for a task it cannot carry (an unknown frame, a joint of the wrong kind)."""

    def frames(self) -> Optional[list]:
        """Frame slots of the group's own device model (``None``: the caller's model serves)."""
        return None

    def create(self, api, model, dmodel: int, B: int) -> None:
        """Device resources of the group's own: its device model (else the caller's ``dmodel`` serves) and the output buffer."""
        from .rollout import ModelArrays

        self.api, self.dmodel = api, dmodel
        if self.frames() is not None:
            self.arrays = ModelArrays(model, self.frames())  # (kept: the descriptor points into its arrays)
            self.dmodel = api.model_create(self.arrays.desc)
        self.out = api.alloc(8 * max(B * self.out_width * len(self.tasks), 1))

    def free(self) -> None:
        if self.api is not None:
            if self.arrays is not None:
                self.api.model_destroy(self.dmodel)
            self.api.release(self.out)
            self.api = self.dmodel = self.arrays = self.out = None


class ComGroup(RowGroup):
    """One ComTask: three rows from the mass tables ``dcom`` (``pinkhip_com_create``) and the target at ``d_target``, which
    holds one target (``batched`` false) or one per robot."""

    name, rows, needs, limit = "com", "centre-of-mass rows", "a ComTask", "at most one ComTask"
    method, kernel, types = "com_task", "pinkhip_com_task_device", (ComTask,)
    out_width, out_every_step = 3, True
    width = staticmethod(lambda task: 3)
    model_declined = staticmethod(lambda model: None if model.total_mass > 0.0 else "the model carries no mass: its centre of mass is undefined")

    def create(self, api, model, dmodel, B):
        super().create(api, model, dmodel, B)
        self.dcom, self.d_target = api.com_create(dmodel, *model.mass_tables()), api.alloc(8 * B * 3)

    def free(self):
        if self.api is not None:
            self.api.release(self.d_target)
            self.api.com_destroy(self.dcom)
        super().free()

    def launch(self, api, B, d_q, d_e, sE, d_J, sJ, row0, out=None):
        api.com_task(self.dmodel, self.dcom, B, d_q, self.d_target, self.batched, d_e, sE, d_J, sJ, row0, out)


class ManipulabilityGroup(RowGroup):
    """Up to four ManipulabilityTasks: one row and one launch each, on a device model whose slots are their frames (the
    frame-task model's slots each own six rows of the frame kernel)."""

    name, rows, needs = "manipulability", "manipulability rows", "a ManipulabilityTask"
    method, kernel, types = "manipulability_task", "pinkhip_manipulability_task_device", (ManipulabilityTask,)
    max_tasks, limit = MAX_MANIPULABILITY_TASKS, "manipulability_tasks: at most four ManipulabilityTask objects"
    width = staticmethod(lambda task: 1)

    def validate(self, model):
        for t in self.tasks:
            check_revolute_path(model, t.frame)

    def frames(self):
        return [t.frame for t in self.tasks]

    def launch(self, api, B, d_q, d_e, sE, d_J, sJ, row0, out=None):
        for i, t in enumerate(self.tasks):
            api.manipulability_task(self.dmodel, B, d_q, i, int(t.reference_frame), t.row_mask, float(t.manipulability_rate), d_e, sE,
                                    d_J, sJ, row0 + i, None if out is None else out + 8 * B * i)


class WheelGroup(RowGroup):
    """Up to eight RollingTasks (three rows) / OmniwheelTasks (two): ONE launch for all wheels -- the world poses are
    composed once -- on a device model whose slots are the ``(hub, floor)`` pairs: relative slots, frame = hub, root = floor."""

    name, rows, needs = "wheels", "wheel-contact rows", "a RollingTask / OmniwheelTask"
    method, kernel, types = "rolling_tasks", "pinkhip_rolling_tasks_device", (RollingTask, OmniwheelTask)
    max_tasks, limit = MAX_WHEELS, "rolling_tasks: at most eight RollingTask / OmniwheelTask objects"
    width = staticmethod(lambda task: len(task.rows))

    def __init__(self, tasks, weights):
        super().__init__(tasks, weights)
        self.pairs, self.kinds, self.radii = wheel_tables(self.tasks)

    def validate(self, model):
        for t in self.tasks:  # (an unknown frame: what a FrameTask raises)
            model.getFrameId(t.hub_frame), model.getFrameId(t.floor_frame)

    def frames(self):
        return list(self.pairs)

    def launch(self, api, B, d_q, d_e, sE, d_J, sJ, row0, out=None):
        api.rolling_tasks(self.dmodel, B, d_q, list(range(len(self.tasks))), self.kinds, self.radii, d_e, sE, d_J, sJ, row0, out)


KINDS = (ComGroup, ManipulabilityGroup, WheelGroup)  # the order of their rows behind the FrameTask rows


def wheel_tables(tasks) -> tuple:
    """``(frames, kinds, radii)`` of the wheels ``tasks`` for ``pinkhip_rolling_tasks_device``: the ``(hub, floor)`` pairs that
    become the relative slots of a device model, 0 (rolling) / 1 (omniwheel), and the radii."""
    return (tuple((t.hub_frame, t.floor_frame) for t in tasks), [1 if type(t) is OmniwheelTask else 0 for t in tasks],
            [float(t.wheel_radius) for t in tasks])


def declined(model, tasks_of_kind: Sequence[Sequence], api) -> Optional[str]:
    """The first reason a kind of :data:`KINDS` gives against its tasks (``tasks_of_kind``: one list per kind; an empty one
    asks nothing), or ``None``."""
    return next((why for why in (kind.declined(model, tasks, api) for kind, tasks in zip(KINDS, tasks_of_kind) if tasks) if why), None)


class Layout:
    """Where the dense rows of a stack lie: ``frame_weights`` -- ``(gain, lm_damping, cost of the six rows)`` per FrameTask,
    whose rows come first (``pinkhip_fk_frame_tasks_device`` or the step kernel forms them) -- then the rows of ``groups``
    (one per kind of :data:`KINDS`, in that order; a group without tasks takes no part).  ``Kd``: the dense rows;
    ``task_rows`` (``n + 1`` boundaries), ``task_kind``, ``task_col0``, ``gain``, ``lm_damping``: the dense prefix of the
    task tables of the QP (``include/pinkhip.h``), as lists; every group gets its ``row0``."""

    def __init__(self, frame_weights: Sequence[tuple], groups: Sequence[RowGroup]):
        self.groups = [g for g in groups if g.tasks]
        self.widths, weights = [6] * len(frame_weights), list(frame_weights)
        for g in self.groups:
            g.row0 = sum(self.widths)
            self.widths += g.widths
            weights += g.weights
        self.Kd, self.n_tasks = sum(self.widths), len(self.widths)
        self.task_rows = [0] + [int(r) for r in np.cumsum(self.widths)]
        self.task_kind, self.task_col0 = [0] * self.n_tasks, [0] * self.n_tasks
        self.gain, self.lm_damping, self.costs = ([w[i] for w in weights] for i in range(3))

    def cost_segments(self, batch: tuple = ()) -> list:
        """The weights of the dense rows, one array ``batch + (rows of the task,)`` per task."""
        return [np.broadcast_to(np.asarray(c, dtype=float), batch + (w,)) for c, w in zip(self.costs, self.widths)]

    def launch_all(self, api, B: int, d_q: int, d_e: int, sE: int, d_J: int, sJ: int) -> None:
        for g in self.groups:
            g.launch(api, B, d_q, d_e, sE, d_J, sJ, g.row0, g.out if g.out_every_step else None)

    def free(self) -> None:
        for g in self.groups:
            g.free()


# ---- barrier rows: into Gd / hd -------------------------------------------------------------------------------------------
def barrier_rows_declined(model, api) -> Optional[str]:
    """Why ``pinkhip_barrier_rows_device`` does not serve this solver and model (the barriers: ``solve_ik._barriers_declined``)."""
    if not hasattr(api, "barrier_rows"):
        return 'this solver has no pinkhip_barrier_rows_device: position barriers need it, or the whole-step kernel (fused="kernel")'
    return _too_many_joints(model, "barrier rows")


def barrier_frames(bars: Sequence) -> list:
    """The frames of the PositionBarriers / BodySphericalBarriers among ``bars``, each once, in order of appearance."""
    frames = []
    for bar in bars:
        for f in (() if hasattr(bar, "distance_query") else tuple(bar.frames) if hasattr(bar, "frames") else (bar.frame,)):
            if f not in frames:
                frames.append(f)
    return frames


class BarrierRows:
    """The rows of ``bars`` (Pink's order, the SelfCollisionBarrier of sphere pairs last) for
    ``pinkhip_barrier_rows_device``: ``sizes`` -- rows per barrier, ``safe`` -- safe-displacement gain per barrier,
    ``n_rows`` -- position and spherical rows; ``slot_of(frame name, what)`` is a frame's slot of the device model the
    launch runs on.  :meth:`upload` puts the six row tables and the five sphere-pair tables on the device and fills the
    ``pinkhip_barrier_rows`` / ``pinkhip_sphere_pairs`` structs (``rows`` / ``pairs``; either may stay ``None``)."""

    def __init__(self, model, bars: Sequence, slot_of, pair_tables=None):
        from .rollout import barrier_row_tables, sphere_pair_tables

        self.sc = next((bar for bar in bars if hasattr(bar, "distance_query")), None)
        self.tables, self.sizes, self.safe = barrier_row_tables(bars, slot_of, self.sc)
        self.n_rows = len(self.tables[0])
        self.pair_tables = pair_tables
        if self.sc is not None and pair_tables is None:
            self.pair_tables = sphere_pair_tables(model, self.sc.distance_query.pairs)
        self.d_rows, self.d_pairs, self.rows, self.pairs, self.dmodel, self.row0 = [], [], None, None, None, 0

    def upload(self, up, dmodel: int, row0: int) -> "BarrierRows":
        """``up(name, array)`` returns the device address of a copy of ``array``; the launch writes from row ``row0`` on."""
        from ._lib import BarrierRowsArgs
        from .rollout import sphere_pairs_args

        self.dmodel, self.row0 = dmodel, int(row0)
        if self.n_rows:
            self.d_rows = [up("bar%d" % i, np.ascontiguousarray(v, dtype=t)) for i, (v, t) in
                           enumerate(zip(self.tables, (np.int32, np.int32, np.float64, np.float64, np.float64, np.int32)))]
            self.rows = BarrierRowsArgs()
            self.rows.n_rows = self.n_rows
            self.rows.frame, self.rows.axis, self.rows.sign, self.rows.bound, self.rows.gain, self.rows.frame2 = self.d_rows
        if self.sc is not None:
            self.d_pairs = [up("pairs%d" % i, a) for i, a in enumerate(self.pair_tables)]
            self.pairs = sphere_pairs_args(self.d_pairs, self.pair_tables, self.sc)
        return self

    def launch(self, api, B: int, d_q: int, dt: float, d_Gd: int, sG: int, d_hd: int, sH: int) -> None:
        api.barrier_rows(self.dmodel, B, d_q, dt, self.rows, self.pairs, d_Gd, sG, d_hd, sH, self.row0)
