"""Golden vectors for the RollingTask / OmniwheelTask: e and J of the REFERENCE's own classes (pink/tasks/rolling_task.py,
omniwheel_task.py) and P, q of its pink.build_ik (pink/solve_ik.py:152-203) over two FrameTasks + the wheels + a
PostureTask, on the models biped and tree34 of tests/rolling_cases.py -- tree34 with a floor on a moving joint (run once;
needs a checkout of the reference, make_golden.py's PINK_REFERENCE).

The stub `pinocchio` of make_golden.py is extended as in make_golden_manipulability.py; pin.SE3(rotation=, translation=),
.actInv and .action are pink_amd.lie.SE3's.  The kinematics (frame transforms, the hub's body Jacobian) are ours; the rim
frame, the adjoint product, the row choice and the stacking are the reference's.  The file also stores the reference
classes' rows, evaluated in fp64, on the anchor configurations of tests/rolling_cases.py: the exact-anchor tests count the
reference's own distance to the 60-digit rows from them.  Nothing of the reference is copied: only its OUTPUTS are stored
(tests/golden/rolling_task.npz, numeric arrays only); tests/test_rolling_golden.py holds the host classes and
pink_amd.build_ik to them.

    python tests/golden/make_golden_rolling.py
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

GOLDEN_MODELS = ("biped", "tree34")
FRAME_TASKS = {"biped": ("base", "right_hub"), "tree34": ("hand", "foot")}
COSTS = {0: [1.0, 0.5, 2.0], 1: [0.8, 1.5]}  # cost vector of a Rolling / an Omniwheel task
GAIN, LM = 0.7, 1e-3


def main():
    mg.install_stubs()
    import pinocchio as pin

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import se3_oracle
    from pink_amd import Configuration
    from pink_amd.lie import SE3, exp6
    from tests.rolling_cases import configurations, models  # (before the reference, which has a `tests` of its own, is on the path)

    sys.path.insert(0, mg.REFERENCE)

    def mat(T):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = T.rotation, T.translation
        return M

    pin.SE3 = SE3
    pin.ARG1 = 1
    pin.log = lambda T: types.SimpleNamespace(vector=se3_oracle.log6(mat(T)))
    pin.Jlog6 = lambda T: se3_oracle.jlog6_mp(mat(T))
    pin.difference = lambda model, q0, q1: model.m.difference(np.asarray(q0, dtype=float), np.asarray(q1, dtype=float))
    pin.neutral = lambda model: model.m.neutral()
    pin.dDifference = lambda model, q0, q1, arg: model.m.d_difference(np.asarray(q0, dtype=float), np.asarray(q1, dtype=float))
    import pink
    from pink.limits import ConfigurationLimit, VelocityLimit
    from pink.tasks import FrameTask, OmniwheelTask, PostureTask, RollingTask

    def reference_configuration(m, q):
        cfg = Configuration(m, q)
        return cfg, types.SimpleNamespace(q=cfg.q, model=ModelView(m), tangent=cfg.tangent, data=cfg,
                                          get_transform_frame_to_world=cfg.get_transform_frame_to_world,
                                          get_transform=cfg.get_transform, get_frame_jacobian=cfg.get_frame_jacobian)

    def wheel_tasks(wheels):
        return [(OmniwheelTask if k else RollingTask)(hub, floor, r, cost=np.array(COSTS[k]), gain=GAIN, lm_damping=LM) for k, hub, floor, r in wheels]

    rng = np.random.default_rng(20261021)
    out = {}
    for name in GOLDEN_MODELS:
        m, wheels = models()[name]
        # the reference's rows on the anchor configurations
        qa = configurations(name)
        es, Js = [], []
        for q in qa:
            _, ref_cfg = reference_configuration(m, q)
            ts = wheel_tasks(wheels)
            es.append(np.concatenate([t.compute_error(ref_cfg) for t in ts]))
            Js.append(np.vstack([t.compute_jacobian(ref_cfg) for t in ts]))
        out[f"{name}/anchor_q"], out[f"{name}/anchor_e"], out[f"{name}/anchor_J"] = qa, np.array(es), np.array(Js)
        # one stack through the reference's build_ik, inside the joint limits
        q = m.neutral()
        for j in m.joints:
            if j.kind == "free_flyer":
                quat = rng.normal(size=4)
                q[j.idx_q:j.idx_q + 3], q[j.idx_q + 3:j.idx_q + 7] = 0.3 * rng.normal(size=3), quat / np.linalg.norm(quat)
            else:
                q[j.idx_q] = rng.uniform(-1.0, 1.0)
        cfg, ref_cfg = reference_configuration(m, q)
        view = ref_cfg.model
        dt = 5e-3
        fts, targets = [], []
        for i, frame in enumerate(FRAME_TASKS[name]):
            ft = FrameTask(frame, position_cost=1.0 + i, orientation_cost=0.5, lm_damping=1e-3, gain=0.9)
            tgt = cfg.get_transform_frame_to_world(frame) * exp6(0.05 * rng.normal(size=6))
            ft.set_target(tgt)
            fts.append(ft)
            targets.append(np.r_[np.asarray(tgt.rotation).ravel(), tgt.translation])
        ts = wheel_tasks(wheels)
        po = PostureTask(cost=5e-2, gain=0.8)
        q_star = q + rng.uniform(-0.1, 0.1, size=m.nq)
        for j in m.joints:
            if j.kind == "free_flyer":
                q_star[j.idx_q:j.idx_q + 7] = q[j.idx_q:j.idx_q + 7]
        po.set_target(q_star)
        problem = pink.build_ik(ref_cfg, fts + ts + [po], dt, damping=1e-12, limits=[ConfigurationLimit(view), VelocityLimit(view)])
        out[f"{name}/q"], out[f"{name}/dt"], out[f"{name}/q_star"] = q, dt, q_star
        out[f"{name}/targets"] = np.array(targets)
        out[f"{name}/e"] = np.concatenate([t.compute_error(ref_cfg) for t in ts])
        out[f"{name}/J"] = np.vstack([t.compute_jacobian(ref_cfg) for t in ts])
        out[f"{name}/P"], out[f"{name}/c"] = problem.P, problem.q
    path = os.path.join(HERE, "rolling_task.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "with", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
