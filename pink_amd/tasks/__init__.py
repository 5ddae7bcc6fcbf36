"""Kinematic tasks (``pink/tasks``)."""
from .com_task import ComTask
from .frame_task import FrameTask
from .manipulability_task import ManipulabilityTask
from .linear_holonomic_task import JointCouplingTask, JointVelocityTask, LinearHolonomicTask
from .posture_task import DampingTask, LowAccelerationTask, PostureTask
from .relative_frame_task import RelativeFrameTask
from .rolling_task import OmniwheelTask, RollingTask
from .task import Task

__all__ = ["Task", "ComTask", "FrameTask", "RelativeFrameTask", "ManipulabilityTask", "RollingTask", "OmniwheelTask", "PostureTask", "DampingTask", "LowAccelerationTask",
           "LinearHolonomicTask", "JointCouplingTask", "JointVelocityTask"]
