"""Golden vectors for the ComTask: P, q of the REFERENCE's own pink.build_ik (pink/solve_ik.py:152-203) over the reference's
own FrameTask x 2, ComTask (vector cost, gain 0.7, lm_damping 1e-3) and PostureTask objects, on the models arm6 and
tree12 of tests/com_task_cases.py (run once; needs a checkout of the reference, make_golden.py's PINK_REFERENCE).

The stub `pinocchio` of make_golden.py is extended by pin.centerOfMass / pin.jacobianCenterOfMass on this repo's
kinematics stand-in, pin.log / pin.Jlog6 by the independent SE(3) maps of oracle/se3_oracle.py (as make_golden_round4.py):
the kinematics are ours, which quantities the tasks ask for, their signs, weights, gains and Levenberg-Marquardt terms
and the stacking are the reference's.  Nothing of the reference is copied: only its OUTPUTS are stored
(tests/golden/com_task.npz, numeric arrays only); tests/test_com_task_golden.py holds pink_amd.build_ik to them.

    python tests/golden/make_golden_com.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


class ModelView:
    """This repo's model under the pin.Model names the reference reads."""

    def __init__(self, m):
        self.m, self.nv, self.nq = m, m.nv, m.nq
        self.joints = m.joints
        self.frames = [types.SimpleNamespace(name=f.name, parentJoint=f.joint) for f in m.frames]
        self.lowerPositionLimit, self.upperPositionLimit, self.velocityLimit = m.lowerPositionLimit, m.upperPositionLimit, m.velocityLimit

    def hasConfigurationLimit(self):
        return np.isfinite(self.m.upperPositionLimit)

    def existJointName(self, name):
        return any(j.name == name for j in self.m.joints)

    def getJointId(self, name):
        return self.m.getJointId(name)

    def existFrame(self, name):
        return any(f.name == name for f in self.m.frames)

    def getFrameId(self, name):
        return self.m.getFrameId(name)


def main():
    mg.install_stubs()
    import pinocchio as pin

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import se3_oracle
    from pink_amd import Configuration
    from pink_amd.lie import exp6
    from tests.com_task_cases import configurations, models  # (before the reference, which has a `tests` of its own, is on the path)

    sys.path.insert(0, mg.REFERENCE)

    def mat(T):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = T.rotation, T.translation
        return M

    pin.ARG1 = 1
    pin.log = lambda T: types.SimpleNamespace(vector=se3_oracle.log6(mat(T)))
    pin.Jlog6 = lambda T: se3_oracle.jlog6_mp(mat(T))
    pin.difference = lambda model, q0, q1: model.m.difference(np.asarray(q0, dtype=float), np.asarray(q1, dtype=float))
    pin.neutral = lambda model: model.m.neutral()
    pin.dDifference = lambda model, q0, q1, arg: model.m.d_difference(np.asarray(q0, dtype=float), np.asarray(q1, dtype=float))
    # (data is the Configuration of this repo: q is the one it was built at)
    pin.centerOfMass = lambda model, data, q: np.array(Configuration(model.m, np.asarray(q, dtype=float)).center_of_mass())
    pin.jacobianCenterOfMass = lambda model, data, q: np.array(Configuration(model.m, np.asarray(q, dtype=float)).jacobian_center_of_mass())
    import pink
    from pink.limits import ConfigurationLimit, VelocityLimit
    from pink.tasks import ComTask, FrameTask, PostureTask

    rng = np.random.default_rng(20261020)
    out = {}
    for case, frames in (("arm6", ["tool0", "joint_3"]), ("tree12", ["hand", "foot"])):
        m = models()[case][0]
        q = 0.15 * configurations(case, B=1, seed=41)[0]  # (inside the joint limits)
        cfg = Configuration(m, q)
        view = ModelView(m)
        ref_cfg = types.SimpleNamespace(q=cfg.q, model=view, tangent=cfg.tangent, data=cfg, get_transform_frame_to_world=cfg.get_transform_frame_to_world,
                                        get_transform=cfg.get_transform, get_frame_jacobian=cfg.get_frame_jacobian)
        dt = 5e-3
        tasks = []
        for k, (frame, pc, oc, lm, gain) in enumerate(((frames[0], 1.0, 0.5, 1e-3, 0.9), (frames[1], [1.0, 2.0, 0.5], 0.0, 0.0, 0.85))):
            t = FrameTask(frame, position_cost=pc, orientation_cost=oc, lm_damping=lm, gain=gain)
            tgt = cfg.get_transform_frame_to_world(frame) * exp6(0.05 * rng.normal(size=6))
            t.set_target(tgt)
            out[f"{case}/target{k}"] = np.r_[np.asarray(tgt.rotation).ravel(), tgt.translation]
            tasks.append(t)
        com = ComTask(cost=[1.0, 2.0, 0.5], lm_damping=1e-3, gain=0.7)
        com_target = cfg.center_of_mass() + 0.03 * rng.normal(size=3)
        com.set_target(com_target)
        po = PostureTask(cost=5e-2, gain=0.8)
        q_star = rng.uniform(-0.3, 0.3, size=m.nq)
        po.set_target(q_star)
        problem = pink.build_ik(ref_cfg, tasks + [com, po], dt, damping=1e-12, limits=[ConfigurationLimit(view), VelocityLimit(view)])
        out[f"{case}/q"], out[f"{case}/dt"], out[f"{case}/com_target"], out[f"{case}/q_star"] = q, dt, com_target, q_star
        out[f"{case}/mass"], out[f"{case}/com"] = m.mass_tables()  # (the model the numbers belong to: tests/com_task_cases.py)
        out[f"{case}/com_e"], out[f"{case}/com_J"] = com.compute_error(ref_cfg), com.compute_jacobian(ref_cfg)
        out[f"{case}/P"], out[f"{case}/c"] = problem.P, problem.q
    path = os.path.join(HERE, "com_task.npz")
    np.savez(path, **out)
    print("wrote", path, "with", len(out), "arrays")


if __name__ == "__main__":
    main()
