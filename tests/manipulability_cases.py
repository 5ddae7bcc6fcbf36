"""Models, cases and the 60-digit reference of the ManipulabilityTask tests (tests/test_manipulability_task.py,
test_manipulability_device.py, test_manipulability_routes.py): computed once per session, shared by all.

  planar2  a planar 2R arm, mask "planar_xy": r = n = 2, eight robots per wavefront on the device
  arm3     a 3R arm, mask "position": A = J J^T of a square J
  arm6     build_chain(6), no mask: r = n = 6
  arm7     build_chain(7): n > r
  tree12   two branches, nj = 12, a prismatic joint on the branch the frame "hand" is NOT on; "foot" sits behind four
           revolute joints: six rows of rank four, exactly singular
  tree36   a revolute tree of 36 joints: one robot per wavefront

A case is (model, frame, reference frame, mask); its configurations are drawn with a seed and kept where cond_2(A) <= 1e4
(regular) or 1e6 <= cond_2(A) <= 1e9 (the ill-conditioned band of arm6) -- the filter runs BEFORE anything is compared,
and every configuration it keeps is tested.
"""
import functools
import os

import mpmath as mp
import numpy as np

from oracle import exact_kinematics as ek
from pink_amd import ReferenceFrame, build_chain
from pink_amd.configuration import Model
from pink_amd.kinematics_batch import BatchKinematics
from pink_amd.lie import SE3, exp3
from pink_amd.rollout import ModelArrays
from tests.row_kernel_kit import EPS, RatioRecorder, _split, ratio, with_manipulability  # noqa: F401 (re-exported)
from tests.row_kernel_kit import cross as _cross

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_UNITS = 8.0  # the project's bar (tests/test_kinematics_exact.py, tests/com_task_cases.py)
LOCAL, WORLD = ReferenceFrame.LOCAL, ReferenceFrame.WORLD
CUSTOM = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 1.0])


def planar(n):
    m = Model()
    parent = -1
    for i in range(n):
        parent = m.add_joint(f"joint_{i + 1}", "revolute", parent, SE3(np.eye(3), [0.0 if i == 0 else 0.4 - 0.1 * i, 0.0, 0.0]), [0, 0, 1], -3.0, 3.0, 2.0)
    m.add_frame("tip", parent, SE3(np.eye(3), [0.25, 0.0, 0.0]))
    return m


def tree(n, seed, prismatic=None):
    """Joints 0..5 a chain, 6.. a second branch off joint 1 (further branches every fifth joint past 11); ``prismatic``:
    index of a prismatic joint.  "hand" sits on joint 5 (six revolute joints behind it), "foot" on the fourth joint of the
    second branch's side chain 0-1-6-7."""
    rng = np.random.default_rng(seed)
    m = Model()
    ids = []
    for i in range(n):
        if i == 0:
            parent = -1
        elif i == 6:
            parent = ids[1]
        elif i > 11 and i % 5 == 0:
            parent = ids[i - 7]
        else:
            parent = ids[-1]
        kind = "prismatic" if i == prismatic else "revolute"
        ids.append(m.add_joint(f"joint_{i + 1}", kind, parent, SE3(exp3(0.7 * rng.normal(size=3)), 0.3 * rng.normal(size=3)),
                               rng.normal(size=3), -3.0, 3.0, 2.0, mass=float(rng.uniform(0.5, 5.0)), com=0.1 * rng.normal(size=3)))
    m.add_frame("hand", ids[5], SE3(exp3([0.3, 0.2, -0.4]), [0.1, -0.05, 0.2]))
    m.add_frame("foot", ids[7], SE3(exp3([-0.1, 0.4, 0.2]), [0.0, 0.1, -0.1]))
    m.add_frame("deep", ids[-1], SE3(exp3([0.2, -0.1, 0.1]), [0.05, 0.0, 0.1]))
    return m


@functools.lru_cache(maxsize=None)
def models():
    return {
        "planar2": (planar(2), ["tip"]),
        "arm3": (build_chain(3), ["tool0"]),
        "arm6": (build_chain(6, mass_seed=3), ["tool0"]),
        "arm7": (build_chain(7, seed=4), ["tool0"]),
        "tree12": (tree(12, 21, prismatic=9), ["hand", "foot", "deep"]),  # joint 9 (prismatic) is on "deep"'s path only
        "tree36": (tree(36, 22), ["hand", "foot", "deep"]),
    }


# name -> (model, frame, reference frame, mask, B, cond band)
REGULAR, ILL = (0.0, 1e4), (1e6, 1e9)
CASES = {
    "planar2": ("planar2", "tip", LOCAL, "planar_xy", 11, REGULAR),
    "arm3": ("arm3", "tool0", LOCAL, "position", 5, REGULAR),
    "arm6": ("arm6", "tool0", LOCAL, None, 5, REGULAR),
    "arm6_world": ("arm6", "tool0", WORLD, None, 3, REGULAR),
    "arm6_custom": ("arm6", "tool0", LOCAL, CUSTOM, 3, REGULAR),
    "arm6_ill": ("arm6", "tool0", LOCAL, None, 3, ILL),
    "arm7": ("arm7", "tool0", LOCAL, None, 3, REGULAR),
    "arm7_planar_world": ("arm7", "tool0", WORLD, "planar_xy", 3, REGULAR),
    "tree12": ("tree12", "hand", LOCAL, None, 3, REGULAR),
    "tree12_position_world": ("tree12", "hand", WORLD, "position", 3, REGULAR),
    "tree36": ("tree36", "hand", LOCAL, None, 1, REGULAR),
}


# Worst ratio (m, dm/dq) of the host NumPy class on each case, measured first (profiles/manipulability_exact.json, "host").
# It stays below 2 on one case only: m is a smooth function of q, so one ulp on q moves the exact result by a few eps --
# the unit does NOT carry cond(A) -- while every route through A = J J^T and A^-1 (the reference's SVD as well as
# L D L^T) loses eps cond(A).  The bar of a case is therefore K_UNITS where the host stays below 2 and four times the host's
# worst ratio elsewhere, for the emulator and the GPU; m and dm/dq come out of one factorisation of A and share its error,
# so the worse of the two is the case's ratio.  (The host test holds the host class to the same bar: that only says that
# the recorded figures are reproduced within a factor of four on another machine's BLAS.)
HOST_WORST = {
    "planar2": 2.64, "arm3": 7.41, "arm6": 44.6, "arm6_world": 23.9, "arm6_custom": 10.3, "arm6_ill": 1.63e6, "arm7": 10.2,
    "arm7_planar_world": 1.68, "tree12": 14.2, "tree12_position_world": 9.02, "tree36": 31.9,
}


def bar(name):
    return K_UNITS if HOST_WORST[name] < 2.0 else 4.0 * HOST_WORST[name]


def mask_array(mask):
    from pink_amd.tasks.manipulability_task import ManipulabilityTask

    return ManipulabilityTask._get_validated_mask(mask)


def mask_bits(mask):
    m = mask_array(mask)
    return 63 if m is None else int(sum(1 << i for i in range(6) if m[i] != 0))


def cond_A(model, frame, rf, mask, q):
    """cond_2(J J^T) per configuration (fp64: it only sorts configurations into the bands)."""
    J = BatchKinematics(model, q).frame_jacobian(frame, rf)
    m = mask_array(mask)
    Jr = J if m is None else J[:, np.nonzero(m)[0]]
    s = np.linalg.svd(Jr @ np.swapaxes(Jr, 1, 2), compute_uv=False)
    return s[:, 0] / s[:, -1]


@functools.lru_cache(maxsize=None)
def configurations(name):
    """(q [B, nq], cond [B]): the first B draws of the case's seeded stream whose cond(A) lies in the case's band."""
    mname, frame, rf, mask, B, (lo, hi) = CASES[name]
    model = models()[mname][0]
    rng = np.random.default_rng(100 + sorted(CASES).index(name))
    n_draw = 200000 if lo > 0.0 else 64
    q = np.zeros((n_draw, model.nq))
    for j in model.joints:
        q[:, j.idx_q] = rng.uniform(-0.5, 0.5, size=n_draw) if j.kind == "prismatic" else rng.uniform(-3.0, 3.0, size=n_draw)
    c = cond_A(model, frame, rf, mask, q)
    keep = np.nonzero((c >= lo) & (c <= hi))[0][:B]
    assert len(keep) == B, (name, len(keep))
    return q[keep], c[keep]


# ---- the 60-digit reference ---------------------------------------------------------------------------------------------
def _adjoint_mp(T):
    R = [row[:3] for row in T[:3]]
    p = [T[0][3], T[1][3], T[2][3]]
    px = ek.hat3(p)
    pxR = ek.mm(px, R)
    z = mp.mpf(0)
    return [R[i] + pxR[i] for i in range(3)] + [[z, z, z] + R[i] for i in range(3)]


@ek.precise
def exact_rows(t, q, f, rf, rows):
    """(m, Jm [nv]) as mpf by the reference's own formula -- m sqrt(det A), Jm[i] = m vec(J H_i^T) . vec(A^-1) with the
    kinematic Hessian of the module docstring of pink_amd/tasks/manipulability_task.py -- from the exact body Jacobian and
    pose of frame slot ``f`` (oracle/exact_kinematics.kinematics); WORLD: the adjoint of the pose times the body Jacobian."""
    Ts, Js = ek.kinematics(t, q)
    J = Js[f]
    if rf == WORLD:
        J = ek.mm(_adjoint_mp(Ts[f]), J)
    n = len(J[0])
    v = [[J[r][k] for r in range(3)] for k in range(n)]
    w = [[J[3 + r][k] for r in range(3)] for k in range(n)]
    Jr = [J[r] for r in rows]
    r = len(rows)
    A = [[sum(Jr[a][k] * Jr[b][k] for k in range(n)) for b in range(r)] for a in range(r)]
    Am = mp.matrix(A)
    m = mp.sqrt(mp.det(Am))
    Ai = mp.inverse(Am)
    zero3 = [mp.mpf(0)] * 3
    out = []
    for i in range(n):
        # H_i [6][n], then JH = Jr (H_i rows)^T, then its contraction with A^-1
        H = [[None] * n for _ in range(6)]
        for k in range(n):
            lin = _cross(w[i], v[k]) if i <= k else _cross(w[k], v[i])
            ang = _cross(w[i], w[k]) if i <= k else zero3
            for c in range(3):
                H[c][k], H[3 + c][k] = lin[c], ang[c]
        s = mp.mpf(0)
        for a in range(r):
            for b in range(r):
                s += sum(Jr[a][k] * H[rows[b]][k] for k in range(n)) * Ai[a, b]
        out.append(m * s)
    return [m], out


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per configuration of the case: (m (hi, lo), S_m, Jm (hi, lo), S_J).  S: how far the exact result moves when q moves
    by one ulp (the unit already carries cond(A): that is how the ill-conditioned band is held to the same bar)."""
    mname, frame, rf, mask, B, _ = CASES[name]
    model, frames = models()[mname]
    arr = ModelArrays(model, frames)
    f = frames.index(frame)
    m = mask_array(mask)
    rows = list(range(6)) if m is None else [int(i) for i in np.nonzero(m)[0]]
    q, _ = configurations(name)
    t = ek.tables(arr)
    fn = lambda qb: exact_rows(t, qb, f, rf, rows)  # noqa: E731
    out = []
    for b in range(q.shape[0]):
        base = fn(q[b])
        S = ek.spread(fn, [q[b]], draws=1, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return out


def worst(name, m, Jm):
    ref = reference(name)
    return (max(ratio(m[b], ref[b][0], ref[b][1]) for b in range(len(ref))),
            max(ratio(Jm[b], ref[b][2], ref[b][3]) for b in range(len(ref))))


# ---- measured ratios: PINK_MANIPULABILITY_RATIOS=<file> (profiles/manipulability_exact.json), beside the bar of every case
# and the unit ---------------------------------------------------------------------------------------------------------------
_UNIT = ("what one ulp on q does to the exact result + eps max|exact| (tests/manipulability_cases.py); <case>_m: the "
         "manipulability, <case>_J: its gradient")
_RECORDER = RatioRecorder("PINK_MANIPULABILITY_RATIOS", "profiles/manipulability_exact.json", ("m", "J"),
                          extra=lambda: {"bar": {n: bar(n) for n in sorted(CASES)}, "unit": _UNIT})
RATIOS, note_ratios, write_ratios = _RECORDER.noted, _RECORDER.note, _RECORDER.write
