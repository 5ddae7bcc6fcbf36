"""ManipulabilityTask on the host: the reference's surface and refusals, the class against the literal formula of the
reference (n x 6 x n Hessian, pinv), the batched evaluator against the class, the singular rule, and the class against the
60-digit anchor the device tests use (tests/manipulability_cases.py)."""
import numpy as np
import pytest

import pink_amd
from pink_amd import Configuration, ManipulabilityTask, ReferenceFrame
from pink_amd import batch_eval as be
from pink_amd.kinematics_batch import BatchKinematics
from pink_amd.tasks.manipulability_task import manipulability_rows
from tests.manipulability_cases import CASES, bar, configurations, mask_array, models, note_ratios, worst, write_ratios


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()


def _literal(J, mask):
    """pink/tasks/manipulability_task.py restated naively: the Hessian entry by entry, np.linalg.det and pinv."""
    rows = np.arange(6) if mask is None else np.nonzero(mask)[0]
    n, v, w = J.shape[1], J[:3], J[3:]
    H = np.zeros((n, 6, n))
    for i in range(n):
        for k in range(n):
            if i <= k:
                H[i, :3, k], H[i, 3:, k] = np.cross(w[:, i], v[:, k]), np.cross(w[:, i], w[:, k])
            else:
                H[i, :3, k] = np.cross(w[:, k], v[:, i])
    Jr = J[rows]
    A = Jr @ Jr.T
    m = np.sqrt(np.linalg.det(A))
    Ai = np.linalg.pinv(A)
    return m, np.array([m * (Jr @ H[i][rows].T).flatten("F") @ Ai.flatten("F") for i in range(n)]), H[:, rows]


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n != "arm6_ill"])
def test_class_matches_the_literal_formula(name):
    mname, frame, rf, mask, B, _ = CASES[name]
    model = models()[mname][0]
    q, cond = configurations(name)
    t = ManipulabilityTask(frame, model, reference_frame=rf, mask=mask, manipulability_rate=0.3)
    for b in range(min(B, 2)):
        cfg = Configuration(model, q[b])
        m, Jm, H = _literal(cfg.get_frame_jacobian(frame, rf), t.mask)
        tol = 1e-13 * (1.0 + cond[b])
        assert abs(t.compute_manipulability(cfg) - m) <= tol * m
        got = t.compute_jacobian(cfg)
        assert got.shape == (1, model.nv) and np.abs(got[0] - Jm).max() <= tol * np.abs(Jm).max()
        assert np.array_equal(t.compute_kinematic_hessian(cfg), H)
        assert np.array_equal(t.compute_error(cfg), [-0.3])


@pytest.mark.parametrize("name", sorted(CASES))
def test_class_against_60_digits(name):
    mname, frame, rf, mask, B, _ = CASES[name]
    model = models()[mname][0]
    q, _ = configurations(name)
    m, Jm = manipulability_rows(BatchKinematics(model, q).frame_jacobian(frame, rf), mask_array(mask))
    rm, rj = worst(name, m, Jm)
    print(f"host {name:22s} m {rm:.3g}  J {rj:.3g}  bar {bar(name):.3g}")
    note_ratios("host", name, rm, rj)
    assert rm <= bar(name) and rj <= bar(name)


def test_world_jacobian_is_the_adjoint_of_the_pose_times_the_body_jacobian():
    from pink_amd.configuration import _adjoint

    model = models()["tree12"][0]
    q = np.random.default_rng(0).uniform(-1, 1, size=(3, model.nq))
    kin = BatchKinematics(model, q)
    for frame in ("hand", "deep"):
        for b in range(3):
            cfg = Configuration(model, q[b])
            Jl, Jw = cfg.get_frame_jacobian(frame), cfg.get_frame_jacobian(frame, ReferenceFrame.WORLD)
            assert np.array_equal(Jl, cfg.get_frame_jacobian(frame, ReferenceFrame.LOCAL))
            assert np.abs(Jw - _adjoint(cfg.get_transform_frame_to_world(frame)) @ Jl).max() < 1e-14
            assert np.abs(kin.frame_jacobian(frame, ReferenceFrame.WORLD)[b] - Jw).max() < 1e-14
            assert np.abs(kin.frame_jacobian(frame)[b] - Jl).max() < 1e-14
    with pytest.raises(ValueError):
        cfg.get_frame_jacobian("hand", 2)


def test_batched_evaluator_and_singular_rule():
    model = models()["tree12"][0]
    q = np.random.default_rng(1).uniform(-2, 2, size=(5, model.nq))
    kin = BatchKinematics(model, q)
    t = ManipulabilityTask("hand", model, cost=0.7, gain=0.5, lm_damping=1e-3, mask="position", reference_frame=ReferenceFrame.WORLD)
    term = be.task_term(kin, [t] * 5, None)
    assert term.J.shape == (5, 1, model.nv) and (term.e == -0.1).all()
    for b in range(5):
        # (the batched kinematics sum in another order: eps cond(A), cond <= 1e3 here, on entries below one)
        assert np.abs(term.J[b] - t.compute_jacobian(Configuration(model, q[b]))).max() <= 1e-12
    # six rows behind four joints: rank four -- m = 0 and a zero row, not the round-off of det / pinv
    s = ManipulabilityTask("foot", model)
    for b in range(5):
        cfg = Configuration(model, q[b])
        assert s.compute_manipulability(cfg) == 0.0 and (s.compute_jacobian(cfg) == 0.0).all()
    # two such tasks in one stack take the host-evaluated evaluator table, any number of them
    assert type(be.task_term(kin, [s] * 5, None)).__name__ == "DenseTaskTerm"


def test_constructor_refusals_and_surface():
    model = models()["tree12"][0]
    assert pink_amd.tasks.ManipulabilityTask is ManipulabilityTask and ReferenceFrame.LOCAL != ReferenceFrame.WORLD
    with pytest.raises(ValueError, match="only supports revolute joints"):
        ManipulabilityTask("deep", model)  # a prismatic joint on the path
    ManipulabilityTask("hand", model)  # ... on another branch: fine
    ff = pink_amd.build_chain(3, free_flyer=True)
    with pytest.raises(ValueError, match="only supports revolute joints"):
        ManipulabilityTask("tool0", ff)
    with pytest.raises(ValueError, match="invalid reference frame"):
        ManipulabilityTask("hand", model, reference_frame=2)
    with pytest.raises(ValueError, match="shape"):
        ManipulabilityTask("hand", model, mask=np.ones(5))
    with pytest.raises(ValueError, match="binary"):
        ManipulabilityTask("hand", model, mask=np.array([1, 0, 2, 0, 0, 0]))
    with pytest.raises(ValueError, match="invalid mask string"):
        ManipulabilityTask("hand", model, mask="planar")
    with pytest.raises(ValueError, match="mask must be"):
        ManipulabilityTask("hand", model, mask=[1, 1, 1, 0, 0, 0])
    t = ManipulabilityTask("hand", model, cost=2.0, lm_damping=1e-3, gain=0.5, manipulability_rate=0.2, mask="orientation")
    assert repr(t) == "ManipulabilityTask(frame=hand, cost=2.0, lm_damping=0.001, gain=0.5, manipulability_rate=0.2)"
    assert t.row_mask == 0b111000 and ManipulabilityTask("hand", model).row_mask == 63
