"""Golden vectors for the ManipulabilityTask: m, Jm, e of the REFERENCE's own class (pink/tasks/manipulability_task.py) and
P, q of its pink.build_ik (pink/solve_ik.py:152-203) over FrameTask + ManipulabilityTask + PostureTask, on the models arm6
and tree12 of tests/manipulability_cases.py (run once; needs a checkout of the reference, make_golden.py's PINK_REFERENCE).

The stub `pinocchio` of make_golden.py is extended, as in make_golden_com.py, by pin.getFrameJacobian(model, data, frame_id,
rf) on this repo's kinematics (data is this repo's Configuration) and by what check_revolute_path reads of a pin.Model:
frames[].parentJoint, joints[].shortname(), names, parents -- Pinocchio's numbering, joint 0 the universe.  The kinematics
are ours; the Hessian, its index convention, det, pinv, the contraction, the sign of e and the stacking are the
reference's.  Nothing of the reference is copied: only its OUTPUTS are stored (tests/golden/manipulability_task.npz,
numeric arrays only); tests/test_manipulability_golden.py holds the host class and pink_amd.build_ik to them.

    python tests/golden/make_golden_manipulability.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_com import ModelView  # noqa: E402

SHORTNAME = {"revolute": "JointModelRevoluteUnaligned", "prismatic": "JointModelPrismaticUnaligned", "free_flyer": "JointModelFreeFlyer"}
# case -> (model, frame of the ManipulabilityTask, frame of the FrameTask, reference frame (0 LOCAL, 1 WORLD), mask)
CUSTOM = [1.0, 0.0, 1.0, 0.0, 1.0, 1.0]
GOLDEN_CASES = {
    "arm6_local": ("arm6", "tool0", "joint_3", 0, None),
    "arm6_world_position": ("arm6", "tool0", "tool0", 1, "position"),
    "arm6_local_planar": ("arm6", "joint_5", "tool0", 0, "planar_xy"),
    "arm6_world_custom": ("arm6", "tool0", "joint_4", 1, CUSTOM),
    "tree12_world": ("tree12", "hand", "foot", 1, None),
    "tree12_local_position": ("tree12", "hand", "deep", 0, "position"),
    "tree12_local_custom": ("tree12", "hand", "hand", 0, CUSTOM),
}


class PinTreeView:
    """What check_revolute_path reads of a pin.Model, in Pinocchio's numbering (joint 0 = universe)."""

    def __init__(self, m):
        self.m = m
        self.joints = [None] + [types.SimpleNamespace(shortname=(lambda k=j.kind: SHORTNAME[k])) for j in m.joints]
        self.names = ["universe"] + [j.name for j in m.joints]
        self.parents = [0] + [j.parent + 1 for j in m.joints]
        self.frames = [types.SimpleNamespace(name=f.name, parentJoint=f.joint + 1) for f in m.frames]

    def getFrameId(self, name):
        return self.m.getFrameId(name)


def main():
    mg.install_stubs()
    import pinocchio as pin

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import se3_oracle
    from pink_amd import Configuration
    from pink_amd.lie import exp6
    from tests.manipulability_cases import cond_A, models  # (before the reference, which has a `tests` of its own, is on the path)

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
    # (data is the Configuration of this repo, built at the q the task is asked about)
    pin.getFrameJacobian = lambda model, data, frame_id, rf: np.array(data.get_frame_jacobian(model.m.frames[frame_id].name, int(rf)))
    import pink
    from pink.limits import ConfigurationLimit, VelocityLimit
    from pink.tasks import FrameTask, ManipulabilityTask, PostureTask

    rng = np.random.default_rng(20261021)
    out = {}
    for case, (mname, frame, ft_frame, rf, mask) in GOLDEN_CASES.items():
        m = models()[mname][0]
        mask_arg = np.array(mask) if isinstance(mask, list) else mask
        # a configuration inside the joint limits with cond(A) <= 1e4, the first of a seeded stream
        qs = rng.uniform(-1.0, 1.0, size=(64, m.nq))
        cond = cond_A(m, frame, rf, mask_arg, qs)
        k = int(np.nonzero(cond <= 1e4)[0][0])
        q = qs[k]
        cfg = Configuration(m, q)
        view = ModelView(m)
        ref_cfg = types.SimpleNamespace(q=cfg.q, model=view, tangent=cfg.tangent, data=cfg, get_transform_frame_to_world=cfg.get_transform_frame_to_world,
                                        get_transform=cfg.get_transform, get_frame_jacobian=cfg.get_frame_jacobian)
        dt = 5e-3
        ft = FrameTask(ft_frame, position_cost=1.0, orientation_cost=0.5, lm_damping=1e-3, gain=0.9)
        tgt = cfg.get_transform_frame_to_world(ft_frame) * exp6(0.05 * rng.normal(size=6))
        ft.set_target(tgt)
        mt = ManipulabilityTask(frame, PinTreeView(m), cost=0.8, lm_damping=1e-3, gain=0.6,
                                reference_frame=pin.ReferenceFrame.WORLD if rf else pin.ReferenceFrame.LOCAL, manipulability_rate=0.2, mask=mask_arg)
        po = PostureTask(cost=5e-2, gain=0.8)
        q_star = rng.uniform(-0.3, 0.3, size=m.nq)
        po.set_target(q_star)
        problem = pink.build_ik(ref_cfg, [ft, mt, po], dt, damping=1e-12, limits=[ConfigurationLimit(view), VelocityLimit(view)])
        out[f"{case}/q"], out[f"{case}/dt"], out[f"{case}/q_star"] = q, dt, q_star
        out[f"{case}/target"] = np.r_[np.asarray(tgt.rotation).ravel(), tgt.translation]
        out[f"{case}/rf"] = rf
        out[f"{case}/mask"] = np.ones(6) if mt.mask is None else np.asarray(mt.mask, dtype=float)
        out[f"{case}/has_mask"] = mt.mask is not None
        out[f"{case}/cond"] = cond[k]
        out[f"{case}/m"] = mt.compute_manipulability(ref_cfg)
        out[f"{case}/Jm"], out[f"{case}/e"] = mt.compute_jacobian(ref_cfg), mt.compute_error(ref_cfg)
        out[f"{case}/P"], out[f"{case}/c"] = problem.P, problem.q
    # the reference refuses a prismatic joint on the path: the message the host class repeats
    try:
        ManipulabilityTask("deep", PinTreeView(models()["tree12"][0]))
        raise SystemExit("the reference accepted a prismatic joint on the path")
    except ValueError as e:
        assert "only supports revolute joints" in str(e)
    path = os.path.join(HERE, "manipulability_task.npz")
    np.savez(path, **out)
    print("wrote", path, "with", len(out), "arrays")


if __name__ == "__main__":
    main()
