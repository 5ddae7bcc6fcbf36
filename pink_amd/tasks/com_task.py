"""Centre-of-mass task: regulate the position of the robot's centre of mass (``pink/tasks/com_task.py``)."""

from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np

from ..exceptions import TargetNotSet, TaskDefinitionError
from .task import Task


class ComTask(Task):
    """3-D task on the centre of mass in the world frame; ``cost`` is one value in [cost] / [m] or one per axis
    (``com_task.py:21-64``).  The masses are the model's (``Joint.mass`` / ``Joint.com``)."""

    def __init__(self, cost: Union[float, Sequence[float], np.ndarray], lm_damping: float = 0.0, gain: float = 1.0):
        super().__init__(cost=np.ones(3), gain=gain, lm_damping=lm_damping)
        self.target_com: Optional[np.ndarray] = None
        self.target_coms: Optional[np.ndarray] = None  # [B, 3] per-instance targets (set_target_batch)
        self.set_cost(cost)

    def set_cost(self, cost: Union[float, Sequence[float], np.ndarray]) -> None:
        """A scalar or three values, none negative (``com_task.py:66-86``)."""
        v = np.asarray(cost, dtype=float)
        if v.ndim > 0 and v.shape != (3,):
            raise TaskDefinitionError(f"CoM cost should be a float or a vector of 3, got shape {v.shape}")
        if not (v >= 0.0).all():
            raise TaskDefinitionError("CoM cost should be >= 0")
        self.cost[:] = v

    def set_target(self, target_com: np.ndarray) -> None:
        """Target position of the centre of mass in the world frame, copied (``com_task.py:88-94``)."""
        t = np.array(target_com, dtype=float)
        if t.shape != (3,):
            raise TaskDefinitionError(f"CoM target should be a vector of 3, got shape {t.shape}")
        self.target_com = t
        self.target_coms = None

    def set_target_batch(self, targets: np.ndarray) -> None:
        """One target per instance of a batch, ``[B, 3]`` (:func:`pink_amd.solve_ik_batch`); replaces a single target."""
        t = np.array(targets, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != 3:
            raise TaskDefinitionError(f"CoM targets should have shape [B, 3], got {t.shape}")
        self.target_coms = np.ascontiguousarray(t)
        self.target_com = None

    def set_target_from_configuration(self, configuration) -> None:
        """The centre of mass at ``configuration`` becomes the target (``com_task.py:96-104``)."""
        self.set_target(configuration.center_of_mass())

    def compute_error(self, configuration) -> np.ndarray:
        """Actual minus target position (``com_task.py:106-127``)."""
        if self.target_com is None:
            raise TargetNotSet("no target set for the centre of mass")
        return configuration.center_of_mass() - self.target_com

    def compute_jacobian(self, configuration) -> np.ndarray:
        """``pin.jacobianCenterOfMass``, ``[3, nv]`` (``com_task.py:129-150``)."""
        if self.target_com is None:
            raise TargetNotSet("no target set for the centre of mass")
        return configuration.jacobian_center_of_mass()

    def __repr__(self):
        return f"ComTask(gain={self.gain}, cost={self.cost}, target_com={self.target_com}, lm_damping={self.lm_damping})"
