"""Wheel-contact tasks: roll without slipping on a plane (``pink/tasks/rolling_task.py``, ``omniwheel_task.py``).

With ``H`` the hub frame (world pose ``R_H, p_H``), ``F`` the floor frame (``R_F, p_F``) and ``rho`` the wheel radius, the
contact point ``p_C = p_H - rho R_F e_z`` is the point of the hub's body that sits ``rho`` below the hub along the floor's
normal.  The rows are

- ``e = (0, 0, z - rho)`` with ``z = (R_F^T (p_H - p_F))_z``;
- ``J``: the velocity of ``p_C``, carried by the hub's body, in the floor's axes, per unit tangent velocity.  For a joint
  ``k`` (world pose ``R_k, p_k``, world axis ``u = R_k axis_k``) between the root and the hub: ``R_F^T (u x (p_C - p_k))``
  (revolute), ``R_F^T u`` (prismatic), ``R_F^T R_k e_i`` and ``R_F^T ((R_k e_i) x (p_C - p_k))`` (free-flyer, linear and
  angular columns); every other column is exactly zero.

The floor is treated as inertial, as the reference treats it: ``R_F`` and ``p_F`` follow ``q`` when the floor frame hangs on
a moving joint, but only the hub's ancestors own columns.  An :class:`OmniwheelTask` keeps rows 0 and 2 (lateral motion is
free).
"""

from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np

from .task import Task


def rolling_rows(configuration, hub_frame: str, floor_frame: str, wheel_radius: float):
    """``(e [3], J [3, nv], z)`` of one wheel at ``configuration`` in the contact-point form of the module docstring."""
    m = configuration.model
    T_H = configuration.get_transform_frame_to_world(hub_frame)
    T_F = configuration.get_transform_frame_to_world(floor_frame)
    R_F = np.asarray(T_F.rotation, dtype=float)
    p_H = np.asarray(T_H.translation, dtype=float)
    z = float(R_F[:, 2] @ (p_H - np.asarray(T_F.translation, dtype=float)))
    p_C = p_H - wheel_radius * R_F[:, 2]
    J = np.zeros((3, m.nv))
    k = m.frames[m.getFrameId(hub_frame)].joint
    while k >= 0:
        jt, T_k = m.joints[k], configuration.oMi[k]
        R_k, d = np.asarray(T_k.rotation, dtype=float), p_C - np.asarray(T_k.translation, dtype=float)
        if jt.kind == "revolute":
            J[:, jt.idx_v] = R_F.T @ np.cross(R_k @ jt.axis, d)
        elif jt.kind == "prismatic":
            J[:, jt.idx_v] = R_F.T @ (R_k @ jt.axis)
        else:  # free-flyer: its tangent is its body twist
            J[:, jt.idx_v:jt.idx_v + 3] = R_F.T @ R_k
            J[:, jt.idx_v + 3:jt.idx_v + 6] = R_F.T @ np.cross(R_k.T, d).T  # column i: (R_k e_i) x d
        k = jt.parent
    return np.array([0.0, 0.0, z - wheel_radius]), J, z


class RollingTask(Task):
    """Roll without slipping on the xy-plane of ``floor_frame``: the contact point of the wheel around ``hub_frame`` does not
    move in the plane, and the hub stays ``wheel_radius`` above it (``rolling_task.py:17-151``).  ``cost`` is one value in
    [cost] / [m] or one per row."""

    rows = (0, 1, 2)  # rows of the three-row contact Jacobian / error this class keeps

    hub_frame: str
    floor_frame: str
    wheel_radius: float

    def __init__(self, hub_frame: str, floor_frame: str, wheel_radius: float,
                 cost: Optional[Union[float, Sequence[float], np.ndarray]], gain: float = 1.0, lm_damping: float = 0.0):
        super().__init__(cost=cost, gain=gain, lm_damping=lm_damping)
        self.floor_frame = floor_frame
        self.hub_frame = hub_frame
        self.wheel_radius = wheel_radius

    def compute_error(self, configuration) -> np.ndarray:
        """``(0, 0, z_hub - rho)`` in the floor's axes (``rolling_task.py:79-111``)."""
        return rolling_rows(configuration, self.hub_frame, self.floor_frame, self.wheel_radius)[0][list(self.rows)]

    def compute_jacobian(self, configuration) -> np.ndarray:
        """Velocity of the contact point in the floor's axes, ``[3, nv]`` (``rolling_task.py:113-139``)."""
        return rolling_rows(configuration, self.hub_frame, self.floor_frame, self.wheel_radius)[1][list(self.rows)]

    def __repr__(self):
        return (f"{type(self).__name__}(hub_frame={self.hub_frame}, floor_frame={self.floor_frame}, "
                f"wheel_radius={self.wheel_radius}, cost={self.cost}, gain={self.gain}, lm_damping={self.lm_damping})")


class OmniwheelTask(RollingTask):
    """A :class:`RollingTask` that leaves lateral motion free: rows 0 and 2 of its three (``omniwheel_task.py:14-77``)."""

    rows = (0, 2)
