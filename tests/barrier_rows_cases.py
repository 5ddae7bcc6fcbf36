"""Models, rows, configurations, the 60-digit reference and the emulator binding of the barrier-row tests
(tests/test_barrier_rows_device.py, test_barrier_rows_routes.py): computed once per session, shared by both.

  A   revolute -> prismatic -> revolute, nj = 3: eight robots per wavefront, B = 19 (three wavefronts, the last with three)
  B   free-flyer root with two branches of unequal depth (3 and 5 joints) and one prismatic joint, nj = 9, nv = 14: two robots
      per wavefront, B = 5 (a partial last wavefront); every joint carries mass (the route tests put a ComTask beside the
      barriers)
  C   a chain of 25 revolute joints with a side branch of 8 on joint 10, nj = 33: one robot per wavefront, B = 3

Rows per model: p_min and p_max rows on each axis on a frame of the root joint and on a frame of a branch tip; spherical
rows between frames on different branches and between a frame and its own ancestor (a frame on an ancestor joint of the
other frame's joint: the common ancestors contribute u x (p_f - p_f2)); 4 spheres / 5 pairs, of which pair 3 repeats pair 1
(bit-equal distances: the tie rule decides which of the two is kept) and pair 2 joins two touching spheres of one joint
(a zero row), with n_rows = 2 and n_rows = n_pairs.

Condition on the selection (asserted by :func:`reference`): apart from the deliberate duplicate, the gap between the
n_rows-th and the next distance of the 60-digit reference is at least 1e-6, so that the reference alone decides the
selection; and for n_rows = 2 the duplicate straddles the cut for at least one robot of every model.
"""
import ctypes
import functools

import mpmath as mp
import numpy as np

from oracle import exact_kinematics as ek
from pink_amd._lib import BarrierRowsArgs, SpherePairsArgs
from pink_amd.barriers import BodySphericalBarrier, PositionBarrier, SelfCollisionBarrier
from pink_amd.barriers.self_collision_barrier import SpherePairs
from pink_amd.configuration import Model
from pink_amd.lie import SE3, exp3
from pink_amd.rollout import ModelArrays, barrier_row_tables, sphere_pair_tables
from tests.row_kernel_kit import CI, EPS, LL, VP, RatioRecorder, _emu, _split, random_configurations, ratio  # noqa: F401 (re-exported)
from tests.row_kernel_kit import cross as _cross

K_BAR = 8.0  # the bar tests/test_kinematics_exact.py holds poses and body Jacobians to
DT = 5e-3
GAP = 1e-6
TIP = SE3(exp3([0.2, -0.3, 0.25]), [0.02, -0.03, 0.04])  # placement of a frame on its joint


def _joint(m, rng, name, kind, parent):
    return m.add_joint(name, kind, parent, SE3(exp3(0.6 * rng.normal(size=3)), 0.3 * rng.normal(size=3)), rng.normal(size=3), -7.0, 7.0, 2.0,
                       mass=float(rng.uniform(0.5, 3.0)), com=0.1 * rng.normal(size=3))


def _model_a():
    rng = np.random.default_rng(101)
    m = Model()
    a = _joint(m, rng, "turn", "revolute", -1)
    b = _joint(m, rng, "slide", "prismatic", a)
    c = _joint(m, rng, "wrist", "revolute", b)
    m.add_frame("base", a, SE3(exp3([0.1, 0.0, 0.2]), [0.05, 0.0, 0.1]))
    m.add_frame("mid", b, SE3(exp3([0.0, 0.2, 0.1]), [0.0, 0.1, 0.0]))
    m.add_frame("tip", c, TIP)
    return m, dict(root="base", tip="tip", branches=("mid", "tip"), ancestor=("tip", "base"), sphere_joints=(b, a, c))


def _model_b():
    rng = np.random.default_rng(102)
    m = Model()
    root = m.add_joint("root_joint", "free_flyer")
    m.joints[root].mass, m.joints[root].com = 4.0, np.array([0.02, -0.01, 0.05])
    left = [root]
    for i in range(3):
        left.append(_joint(m, rng, f"left_{i}", "revolute", left[-1]))
    right = [root]
    for i in range(5):
        right.append(_joint(m, rng, f"right_{i}", "prismatic" if i == 2 else "revolute", right[-1]))
    m.add_frame("base", root, SE3(exp3([0.1, 0.0, 0.2]), [0.05, 0.0, 0.1]))
    m.add_frame("left_tip", left[-1], TIP)
    m.add_frame("right_tip", right[-1], SE3(exp3([-0.3, 0.1, 0.2]), [0.01, 0.04, -0.02]))
    m.add_frame("right_knee", right[2], SE3(exp3([0.3, 0.3, -0.2]), [0.1, 0.0, -0.1]))
    return m, dict(root="base", tip="right_tip", branches=("left_tip", "right_tip"), ancestor=("right_tip", "right_knee"),
                   sphere_joints=(left[-1], right[3], right[-1]))


def _model_c():
    rng = np.random.default_rng(103)
    m = Model()
    main = [-1]
    for i in range(25):
        main.append(_joint(m, rng, f"main_{i}", "revolute", main[-1]))
    side = [main[10]]
    for i in range(8):
        side.append(_joint(m, rng, f"side_{i}", "revolute", side[-1]))
    m.add_frame("base", main[1], SE3(exp3([0.1, 0.0, 0.2]), [0.05, 0.0, 0.1]))
    m.add_frame("main_tip", main[-1], TIP)
    m.add_frame("side_tip", side[-1], SE3(exp3([-0.3, 0.1, 0.2]), [0.01, 0.04, -0.02]))
    m.add_frame("main_mid", main[15], SE3(exp3([0.3, 0.3, -0.2]), [0.1, 0.0, -0.1]))
    return m, dict(root="base", tip="side_tip", branches=("main_tip", "side_tip"), ancestor=("main_tip", "main_mid"),
                   sphere_joints=(main[6], main[-1], side[-1]))


NAMES = ["A", "B", "C"]
BATCH = {"A": 19, "B": 5, "C": 3}
WIDTH = {"A": 8, "B": 32, "C": 64}


@functools.lru_cache(maxsize=None)
def models():
    """name -> (model, what): frames of the rows and joints of the spheres."""
    out = {"A": _model_a(), "B": _model_b(), "C": _model_c()}
    assert [len(out[n][0].joints) for n in NAMES] == [3, 9, 33]
    return out


def barriers_of(name, n_pairs_rows=2, position_gain_function=None):
    """The barriers of a model, in Pink's order: two PositionBarriers (p_min and p_max on every axis, on a frame of the root
    joint and on a branch tip), two BodySphericalBarriers (different branches; a frame and its own ancestor) and one
    SelfCollisionBarrier of 4 spheres / 5 pairs that keeps ``n_pairs_rows`` rows (0: none)."""
    model, what = models()[name]
    ja, jb, jc = what["sphere_joints"]
    bars = [
        PositionBarrier(what["root"], indices=[0, 1, 2], p_min=np.array([-0.9, -1.1, -1.3]), p_max=np.array([1.2, 0.8, 1.0]), gain=np.array([0.9, 1.1, 0.7, 1.3, 0.8, 1.2])),
        PositionBarrier(what["tip"], indices=[0, 1, 2], p_min=np.array([-1.5, -0.7, -1.2]), p_max=np.array([0.6, 1.4, 0.9]), gain=np.array([1.0, 0.6, 1.4, 0.5, 1.5, 0.75])),
        BodySphericalBarrier(what["branches"], d_min=0.3, gain=1.7),
        BodySphericalBarrier(what["ancestor"], d_min=0.2, gain=0.8),
    ]
    if position_gain_function is not None:  # (a class-K function of the caller's: the host evaluates such a barrier)
        bars[0].gain_function, bars[0].identity_gain_function = position_gain_function, False
    if n_pairs_rows:
        # spheres 0 .. 3: on ja, on jb, on jc, and a second one on jc that touches the first (centres 0.25 apart, radii 0.125)
        s0, s1, s2, s3 = (ja, [0.05, -0.02, 0.03], 0.08), (jb, [-0.04, 0.03, 0.02], 0.06), (jc, [0.0, 0.0, 0.0], 0.125), (jc, [0.25, 0.0, 0.0], 0.125)
        pairs = [(*a, *b) for a, b in ((s0, s2), (s1, s2), (s2, s3), (s1, s2), (s0, s3))]
        bars.append(SelfCollisionBarrier(n_pairs_rows, gain=1.6, d_min=0.05, distance_query=SpherePairs(pairs)))
    return bars


def frames_of(bars):
    out = []
    for bar in bars:
        for f in (() if hasattr(bar, "distance_query") else tuple(bar.frames) if hasattr(bar, "frames") else (bar.frame,)):
            if f not in out:
                out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def tables(name, n_pairs_rows=2):
    """(arrays, rows [6 arrays: frame, axis, sign, bound, gain, frame2], sphere tables or None, (n_rows, d_min, gain) of the
    pairs) -- the host tables of one call."""
    model, _ = models()[name]
    bars = barriers_of(name, n_pairs_rows)
    frames = frames_of(bars)
    sc = bars[-1] if n_pairs_rows else None
    lists, _, _ = barrier_row_tables(bars, lambda f, what: frames.index(f), sc)
    rows = tuple(np.ascontiguousarray(v, dtype=t) for v, t in zip(lists, (np.int32, np.int32, np.float64, np.float64, np.float64, np.int32)))
    sp = sphere_pair_tables(model, sc.distance_query.pairs) if sc is not None else None
    return ModelArrays(model, frames), rows, sp, (n_pairs_rows, 0.05, 1.6)


def configurations(name, B=None, seed=7):
    model = models()[name][0]
    return random_configurations(model, BATCH[name] if B is None else B, np.random.default_rng(seed + ord(name[0])))


# ---- the 60-digit reference ---------------------------------------------------------------------------------------------
def _point_velocity(t, oM, joint, P, nv):
    """World velocity of the point P carried by joint ``joint`` per unit tangent velocity: 3 x nv (mpf), zero off the path."""
    V = [[mp.mpf(0)] * nv for _ in range(3)]
    k = joint
    while k >= 0:
        jt, iv = int(t.jtype[k]), int(t.idx_v[k])
        Rk = [[oM[k][i][j] for j in range(3)] for i in range(3)]
        d = [P[i] - oM[k][i][3] for i in range(3)]
        if jt == ek.FREE_FLYER:
            axes = [[Rk[i][c] for i in range(3)] for c in range(3)]
            cols = axes + [_cross(s, d) for s in axes]
        else:
            a = [mp.mpf(float(c)) for c in t.axis[k]]
            u = [sum(Rk[i][j] * a[j] for j in range(3)) for i in range(3)]
            cols = [_cross(u, d) if jt == ek.REVOLUTE else u]
        for c, l in enumerate(cols):
            for r in range(3):
                V[r][iv + c] = l[r]
        k = int(t.parent[k])
    return V


def _mpf(x):
    return mp.mpf(float(x))


@ek.precise
def exact_rows(t, q, rows, sp, pairs, dt):
    """(G [nr][nv], h [nr], dist [n_pairs_rows], all distances [n_pairs]) as mpf from the exact joint poses by plain mpf products:
    Gd = -J_h / dt and hd = gain alpha(h) of barrier.py:246-254 for the position / spherical rows of the tables ``rows`` and
    the sphere-pair rows of ``sp`` (tables) / ``pairs`` = (n_rows, d_min, gain)."""
    oM = ek.joint_poses(t, q)
    nv = sum(6 if int(x) == ek.FREE_FLYER else 1 for x in t.jtype)
    dt = _mpf(dt)
    G, h = [], []

    def origin(f):
        P = ek.pose_matrix(t.frame_placement[f])
        fj = int(t.frame_joint[f])
        T = P if fj < 0 else ek.mm(oM[fj], P)
        return [T[i][3] for i in range(3)], fj

    frame, axis, sign, bound, gain, frame2 = rows
    for r in range(len(frame)):
        pf, fj = origin(int(frame[r]))
        Vf = _point_velocity(t, oM, fj, pf, nv)
        if int(axis[r]) == 3:
            pg, gj = origin(int(frame2[r]))
            Vg = _point_velocity(t, oM, gj, pg, nv)
            d = [pf[i] - pg[i] for i in range(3)]
            hv = sum(x * x for x in d) - _mpf(bound[r])
            J = [2 * sum(d[i] * (Vf[i][j] - Vg[i][j]) for i in range(3)) for j in range(nv)]
            h.append(_mpf(gain[r]) * hv / (1 + abs(hv)))
        else:
            ax, sg = int(axis[r]), _mpf(sign[r])
            J = [sg * Vf[ax][j] for j in range(nv)]
            h.append(_mpf(gain[r]) * sg * (pf[ax] - _mpf(bound[r])))
        G.append([-x / dt for x in J])
    dist_sel, dist_all = [], []
    if sp is not None:
        sj, sc, sr, _, ps = sp
        nr, d_min, pgain = pairs
        C = []
        for s in range(len(sj)):
            T = oM[int(sj[s])]
            c = [_mpf(x) for x in sc[s]]
            C.append([sum(T[i][l] * c[l] for l in range(3)) + T[i][3] for i in range(3)])
        for a, b in ps:
            rho = mp.sqrt(sum((C[b][i] - C[a][i]) ** 2 for i in range(3)))
            dist_all.append(rho - _mpf(sr[a]) - _mpf(sr[b]))
        order = sorted(range(len(ps)), key=lambda k: (dist_all[k], k))
        for k in order[:nr]:
            a, b = int(ps[k][0]), int(ps[k][1])
            rho = mp.sqrt(sum((C[b][i] - C[a][i]) ** 2 for i in range(3)))
            u = [(C[b][i] - C[a][i]) / rho for i in range(3)]
            w1 = [C[a][i] + _mpf(sr[a]) * u[i] for i in range(3)]
            w2 = [C[b][i] - _mpf(sr[b]) * u[i] for i in range(3)]
            close = all(abs(w1[i] - w2[i]) <= mp.mpf("1e-8") + mp.mpf("1e-5") * abs(w2[i]) for i in range(3))  # np.allclose
            if close:
                J = [mp.mpf(0)] * nv
            else:
                nn = mp.sqrt(sum((w1[i] - w2[i]) ** 2 for i in range(3)))
                n = [(w1[i] - w2[i]) / nn for i in range(3)]
                V1 = _point_velocity(t, oM, int(sj[a]), w1, nv)
                V2 = _point_velocity(t, oM, int(sj[b]), w2, nv)
                J = [sum(n[i] * (V1[i][j] - V2[i][j]) for i in range(3)) for j in range(nv)]
            G.append([-x / dt for x in J])
            h.append(_mpf(pgain) * (dist_all[k] - _mpf(d_min)))
            dist_sel.append(dist_all[k])
    return G, h, dist_sel, dist_all


def _fn(arr, rows, sp, nr):
    def fn(pl, ax, qb, fp, bound, gain, centre, radius, scal):
        t = ek.tables(arr, placement=pl, axis=ax, frame_placement=fp)
        r = (rows[0], rows[1], rows[2], bound, gain, rows[5])
        s = None if sp is None else (sp[0], centre, radius, sp[3], sp[4])
        return exact_rows(t, qb, r, s, (nr, scal[1], scal[2]), scal[0])[:3]
    return fn


@functools.lru_cache(maxsize=None)
def reference(name, n_pairs_rows=2):
    """q and, per instance, ((G, S_G), (h, S_h), (dist, S_d)) with every exact array split into (hi, lo): S is how far the exact
    result moves when every double it is computed from -- placements, axes, q, frame placements, bounds, gains, sphere centres
    and radii, dt, d_min -- moves by one ulp.  Asserts the conditions on the selection (module docstring)."""
    arr, rows, sp, (nr, d_min, pgain) = tables(name, n_pairs_rows)
    q = configurations(name)
    fn = _fn(arr, rows, sp, nr)
    t = ek.tables(arr)
    out, straddles = [], 0
    for b in range(q.shape[0]):
        if sp is not None:
            with mp.workdps(ek.DPS):
                d = exact_rows(t, q[b], rows, sp, (nr, d_min, pgain), DT)[3]
                order = sorted(range(len(d)), key=lambda k: (d[k], k))
                if nr < len(order):
                    a, c = order[nr - 1], order[nr]
                    dup = {a, c} == {1, 3}
                    assert dup or d[c] - d[a] >= GAP, (name, b, float(d[c] - d[a]))
                    straddles += dup
                assert d[1] == d[3]
        scal = np.array([DT, d_min, pgain])
        centre, radius = (sp[1], sp[2]) if sp is not None else (np.zeros((1, 3)), np.zeros(1))
        inputs = [arr.placement, arr.axis, q[b], arr.frame_placement, rows[3], rows[4], centre, radius, scal]
        base = fn(*inputs)
        S = ek.spread(fn, inputs, draws=1, seed=b, base=base)
        out.append(tuple((_split(base[i]), S[i]) for i in range(3)))
    if sp is not None and nr < len(sp[4]):
        assert straddles > 0, f"model {name}: the duplicate never straddles the cut"
    return q, out


def worst(name, G, h, dist=None, n_pairs_rows=2):
    """Worst ratios (G, h, dist) over the batch of ``name``: G [B, nr, nv], h [B, nr], dist [B, n_pairs_rows] or None."""
    q, ref = reference(name, n_pairs_rows)
    B = q.shape[0]
    rg = max(ratio(G[b], *ref[b][0]) for b in range(B))
    rh = max(ratio(h[b], *ref[b][1]) for b in range(B))
    rd = None if dist is None or not n_pairs_rows else max(ratio(dist[b], *ref[b][2]) for b in range(B))
    return rg, rh, rd


def n_rows_of(name, n_pairs_rows=2):
    return len(tables(name, n_pairs_rows)[1][0]) + n_pairs_rows


# ---- measured ratios: PINK_BARRIER_ROWS_RATIOS=<file> (profiles/barrier_rows_exact.json) ---------------------------------------
_RECORDER = RatioRecorder("PINK_BARRIER_ROWS_RATIOS", "profiles/barrier_rows_exact.json", ("G", "h", "dist"), merge=True)
RATIOS, note_ratios, write_ratios = _RECORDER.noted, _RECORDER.note, _RECORDER.write


# ---- the emulator behind BatchSolver.barrier_rows ----------------------------------------------------------------------------
def with_barrier_rows(api):
    """``barrier_rows`` (pinkhip_barrier_rows_device's twin on host memory); a GPU solver has the method already."""
    if hasattr(api, "barrier_rows"):
        return api
    lib, check = _emu(api, pinkhip_emu_barrier_rows=[VP, LL, VP, ctypes.c_double, ctypes.POINTER(BarrierRowsArgs), ctypes.POINTER(SpherePairsArgs),
                                                     VP, LL, VP, LL, CI, VP])

    def barrier_rows(model, B, q, dt, rows, pairs, Gd, sG, hd, sH, row0, dist_out=None):
        check(lib.pinkhip_emu_barrier_rows(model, B, q, float(dt), None if rows is None else ctypes.byref(rows),
                                           None if pairs is None else ctypes.byref(pairs), Gd, sG, hd, sH, int(row0), dist_out))

    api.barrier_rows = barrier_rows
    return api
