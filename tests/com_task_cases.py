"""Models, configurations and the 60-digit reference of the ComTask tests (tests/test_com_task.py, test_com_task_device.py,
test_com_task_routes.py): computed once per session, shared by all three.

  arm6    a 6-dof arm, nj = 6: eight robots per wavefront on the device
  tree12  a tree with branches of unequal depth and one prismatic joint, nj = 12; joints 2 and 9 massless, the leaf
          joint 8 holds 80 % of the mass; no centre lies on its joint's axis
  tree34  the same generator, 33 joints behind a free-flyer (nj = 34, nv = 39)
  pend    tests/golden/double_pendulum.urdf through load_urdf
  chain8, chain32  serial revolute chains of 8 and 32 joints, every joint with a mass: the deepest tree a group of 8 / 32 lanes
          admits (3 and 5 rounds of pointer jumping), no idle lane in the group (nj = W), and a partial last wavefront
          (B = 9: eight robots in one, the ninth alone in a second; B = 3 at two robots per wavefront)
"""
import functools
import os

import mpmath as mp
import numpy as np

from oracle import exact_kinematics as ek
from pink_amd import build_chain, load_urdf
from pink_amd.configuration import Model
from pink_amd.lie import SE3, exp3
from pink_amd.rollout import ModelArrays
from tests.row_kernel_kit import EPS, RatioRecorder, _split, random_configurations, ratio, with_com  # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_COM = 8.0  # the bar tests/test_kinematics_exact.py holds poses and body Jacobians to
H_FD = 1e-25


def tree(n, free_flyer, seed):
    rng = np.random.default_rng(seed)
    m = Model()
    root = m.add_joint("root_joint", "free_flyer") if free_flyer else -1
    ids = []
    for i in range(n):
        if i == 0 or i == 11:
            parent = root if i == 0 else ids[0]
        elif i == 4:
            parent = ids[1]
        elif i == 9:
            parent = ids[5]
        elif i > 11 and i % 5 == 0:
            parent = ids[i - 7]
        else:
            parent = ids[-1]
        kind = "prismatic" if i == 3 else "revolute"
        ids.append(m.add_joint(f"joint_{i + 1}", kind, parent, SE3(exp3(0.7 * rng.normal(size=3)), 0.3 * rng.normal(size=3)),
                               rng.normal(size=3), -3.0, 3.0, 2.0))
    m.add_frame("hand", ids[8], SE3(exp3([0.3, 0.2, -0.4]), [0.1, -0.05, 0.2]))
    m.add_frame("foot", ids[3], SE3(exp3([-0.1, 0.4, 0.2]), [0.0, 0.1, -0.1]))
    for j in m.joints:
        j.mass = float(rng.uniform(0.5, 5.0))
        j.com = 0.1 * rng.normal(size=3)
        if j.axis is not None:
            assert np.linalg.norm(np.cross(j.axis, j.com)) > 1e-3  # off the joint axis
    m.joints[ids[2]].mass = m.joints[ids[9]].mass = 0.0
    leaf = m.joints[ids[8]]
    leaf.mass = 0.0
    leaf.mass = 4.0 * m.total_mass  # 80 % of the total
    return m


def chain(n, seed):
    """A serial chain of n revolute joints with random axes and placements, every joint with a mass off its axis."""
    rng = np.random.default_rng(seed)
    m = Model()
    parent = -1
    for i in range(n):
        parent = m.add_joint(f"joint_{i + 1}", "revolute", parent, SE3(exp3(0.7 * rng.normal(size=3)), 0.3 * rng.normal(size=3)),
                             rng.normal(size=3), -3.0, 3.0, 2.0, mass=float(rng.uniform(0.5, 5.0)), com=0.1 * rng.normal(size=3))
    return m


@functools.lru_cache(maxsize=None)
def models():
    return {
        "arm6": (build_chain(6, mass_seed=3), ["tool0"]),
        "tree12": (tree(12, False, 12), ["hand", "foot"]),
        "tree34": (tree(33, True, 12), ["hand", "foot"]),
        "pend": (load_urdf(os.path.join(ROOT, "tests", "golden", "double_pendulum.urdf")), []),
        "chain8": (chain(8, 8), []),
        "chain32": (chain(32, 32), []),
    }


BATCH = {"arm6": 11, "tree12": 3, "tree34": 2, "pend": 3, "chain8": 9, "chain32": 3}


def configurations(name, B=None, seed=7):
    """Revolute angles over a few turns, prismatic coordinates in +-0.5, free-flyer quaternions with w < 0."""
    model = models()[name][0]
    B = BATCH[name] if B is None else B
    return random_configurations(model, B, np.random.default_rng(seed + len(name)))


# ---- the 60-digit reference ---------------------------------------------------------------------------------------------
def _moment(T, mk, c):
    return [mk * sum(T[i][l] * c[l] for l in range(4)) for i in range(3)]


def exact_com_of(t, motions, mass, com, base=None, k0=None):
    """sum_k m_k T_k c_k / M from the joints' motions (4 x 4, mpf), composed along the tree as exact_kinematics._chain.
    Returns (com, state); with the ``state`` of another call as ``base`` and ``k0`` the one joint whose motion differs,
    only the poses of the subtree of ``k0`` are composed again (the others do not move)."""
    nj = len(t.parent)
    mk = [mp.mpf(float(x)) for x in mass]
    cs = [[mp.mpf(float(x)) for x in com[k]] + [mp.mpf(1)] for k in range(nj)]
    M = sum(mk)
    if base is None:
        oM, w = [], []
        for k in range(nj):
            A = ek.mm(ek.pose_matrix(t.placement[k]), motions[k])
            p = int(t.parent[k])
            oM.append(A if p < 0 else ek.mm(oM[p], A))
            w.append(_moment(oM[k], mk[k], cs[k]))
        s = [sum(x[i] for x in w) for i in range(3)]
        return [x / M for x in s], (oM, w, s)
    oM0, w0, s0 = base
    oM, s = {}, list(s0)
    for k in range(k0, nj):
        p = int(t.parent[k])
        if k != k0 and p not in oM:
            continue
        A = ek.mm(ek.pose_matrix(t.placement[k]), motions[k])
        oM[k] = A if p < 0 else ek.mm(oM[p] if p in oM else oM0[p], A)
        wk = _moment(oM[k], mk[k], cs[k])
        s = [s[i] - w0[k][i] + wk[i] for i in range(3)]
    return [x / M for x in s], None


def moved(t, base_k, k, sub, h):
    """Motion of joint k at q (+) h e_j from its motion at q: times expm(h G), G the twist matrix of the tangent
    direction -- exact_kinematics.integrate's rule for the free-flyer, and the same matrix as its exp((q + h) G) for a
    scalar joint (one exponential of a tiny matrix instead of one of several radians; the test file holds the two to
    each other at 1e-55)."""
    v = [mp.mpf(0)] * 6
    if int(t.jtype[k]) == ek.FREE_FLYER:
        v[sub] = h
    else:
        a = [mp.mpf(float(c)) * h for c in t.axis[k]]
        v = (v[:3] + a) if int(t.jtype[k]) == ek.REVOLUTE else (a + v[3:])
    return ek.mm(base_k, ek.expm(ek.hat6(v)))


@ek.precise
def exact_com_and_jacobian(t, q, mass, com):
    """(com [3], J [3][nv]) as mpf: the centre from the exact joint poses, J by central differences of it at 1e-25 along
    q (+) h e_j."""
    nj = len(t.parent)
    base = [ek.joint_matrix(int(t.jtype[k]), t.axis[k], q[int(t.idx_q[k]):int(t.idx_q[k]) + (7 if int(t.jtype[k]) == ek.FREE_FLYER else 1)])
            for k in range(nj)]
    c, state = exact_com_of(t, base, mass, com)
    nv = sum(6 if int(x) == ek.FREE_FLYER else 1 for x in t.jtype)
    J = [[mp.mpf(0)] * nv for _ in range(3)]
    h = mp.mpf(H_FD)
    for k in range(nj):
        for sub in range(6 if int(t.jtype[k]) == ek.FREE_FLYER else 1):
            side = []
            for sg in (1, -1):
                mot = list(base)
                mot[k] = moved(t, base[k], k, sub, sg * h)
                side.append(exact_com_of(t, mot, mass, com, base=state, k0=k)[0])
            for i in range(3):
                J[i][int(t.idx_v[k]) + sub] = (side[0][i] - side[1][i]) / (2 * h)
    return c, J


@functools.lru_cache(maxsize=None)
def reference(name):
    """q and, per instance, (com (hi, lo), S_com, J (hi, lo), S_J): S is how far the exact result moves when every
    double it is computed from -- placements, axes, q, masses, centres -- moves by one ulp."""
    model, frames = models()[name]
    arr = ModelArrays(model, frames)
    mass, com = model.mass_tables()
    q = configurations(name)
    fn = lambda pl, ax, qb, ms, cm: exact_com_and_jacobian(ek.tables(arr, placement=pl, axis=ax, nf=0), qb, ms, cm)  # noqa: E731
    out = []
    for b in range(q.shape[0]):
        inputs = [arr.placement, arr.axis, q[b], mass, com]
        base = fn(*inputs)
        S = ek.spread(fn, inputs, draws=1, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return q, out


def worst(name, c, J):
    q, ref = reference(name)
    return (max(ratio(c[b], ref[b][0], ref[b][1]) for b in range(q.shape[0])),
            max(ratio(J[b], ref[b][2], ref[b][3]) for b in range(q.shape[0])))


# ---- measured ratios: PINK_COM_TASK_RATIOS=<file> (profiles/com_task_exact.json) -------------------------------------------------
_RECORDER = RatioRecorder("PINK_COM_TASK_RATIOS", "profiles/com_task_exact.json", ("com", "J"))
RATIOS, note_ratios, write_ratios = _RECORDER.noted, _RECORDER.note, _RECORDER.write
