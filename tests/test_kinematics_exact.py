"""The device kinematics -- forward kinematics, body Jacobians, log6 / Jlog6 rows, q (+) dq -- against
oracle/exact_kinematics.py (60-digit arithmetic from the definitions), on the CPU wave emulator and on the GPU, at the
edges where such code goes wrong: prismatic joints, branches of unequal depth, angles of several turns, arguments of
sin / cos next to multiples of pi/2, quaternions with w < 0 and of norm 3.7, relative rotations at the series /
closed-form / near-pi switches of log3 and at theta = pi itself, twists at the switches of integrate_joint.

Tolerances are counted in units of u = S + eps max|reference|: S (``exact_kinematics.spread``) is how far the exact
result moves when every double it is computed from moves by one ulp -- what NO fp64 code can be blamed for.  The
limit of a family is K = max(8, 4 x the worst ratio of the HOST NumPy path on the same cases), the host path
(pink_amd.lie, Configuration) being measured, not tested, here; profiles/kinematics_exact.json holds the measured
ratios of the host path, the emulator and the GPU.  The 2 ulp of sin / cos and the exact zeros of the Jacobians are
absolute.

PINK_KINEMATICS_EXACT_RATIOS=<file>: the worst ratios of this run are written there as JSON."""
import functools
import json
import os

import mpmath as mp
import numpy as np
import pytest

from oracle import exact_kinematics as ek
from pink_amd import Configuration, FrameTask
from pink_amd.configuration import Model
from pink_amd.lie import SE3
from pink_amd.rollout import ModelArrays, pose12
from pink_amd.runtime import set_default_solver
from tests.test_rollout import _edge_models

EPS = 2.0 ** -52

# K = max(8, 4 x worst host ratio), per family; the host ratios as measured (profiles/kinematics_exact.json):
K_POSES = 8.0       # host 0.437
K_JACOBIANS = 8.0   # host 0.966
K_E = 4 * 15.3      # host 15.3: theta = pi - 1.01e-2, the closed form k = theta / (2 s) one step before log3 switches to
K_J = 4 * 13.0      # host 13.0  the symmetric part (it divides round-off of R - R^T by sin theta = 1e-2); 2.3 / 1.3 elsewhere
K_INTEGRATE = 8.0   # host 1.03

RATIOS = {}


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    s = request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver")
    set_default_solver(s)
    yield s
    set_default_solver(None)


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PINK_KINEMATICS_EXACT_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump({k: {fam: float("%.3g" % v) for fam, v in sorted(d.items())} for k, d in sorted(RATIOS.items())}, f, indent=1)
            f.write("\n")


def _backend(api):
    return "emu" if "Emu" in type(api).__name__ else "gpu"


def _note(backend, family, ratio):
    d = RATIOS.setdefault(backend, {})
    d[family] = max(d.get(family, 0.0), float(ratio))
    print(f"{backend:5s} {family:10s} worst ratio {ratio:.3g}")


# ---- models -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all_models():
    from pink_amd.lie import exp3

    one = Model()
    one.add_joint("joint_1", "revolute", -1, SE3(), [0.0, 0.0, 1.0])
    rng = np.random.default_rng(20)
    rpr = Model()
    p = -1
    for i, kind in enumerate(("revolute", "prismatic", "revolute")):
        p = rpr.add_joint(f"joint_{i + 1}", kind, p, SE3(exp3(0.7 * rng.normal(size=3)), 0.3 * rng.normal(size=3)), rng.normal(size=3))
    rpr.add_frame("tool0", p, SE3(exp3([0.3, 0.2, -0.4]), [0.1, -0.05, 0.2]))
    models = {"one_z": (one, ["joint_1"]), "rpr": (rpr, ["tool0"])}
    models.update(_edge_models())
    return models


MODEL_NAMES = ["one_z", "rpr", "tree15", "arm12p", "big30p"]


def _arrays(name):
    model, frames = _all_models()[name]
    return model, frames, ModelArrays(model, frames)


def _configurations(name, B, seed, turns=20.0):
    """Revolute angles over several turns, prismatic coordinates in +-0.5, free-flyer quaternions with w < 0, the last
    one scaled by 3.7 (quat_to_rot normalises)."""
    model, _ = _all_models()[name]
    rng = np.random.default_rng(seed)
    q = np.zeros((B, model.nq))
    for j in model.joints:
        if j.kind == "free_flyer":
            q[:, j.idx_q:j.idx_q + 3] = rng.normal(size=(B, 3))
            qu = rng.normal(size=(B, 4))
            qu[:, 3] = -np.abs(qu[:, 3]) - 0.1
            qu /= np.linalg.norm(qu, axis=1, keepdims=True)
            qu[-1] *= 3.7
            q[:, j.idx_q + 3:j.idx_q + 7] = qu
        elif j.kind == "prismatic":
            q[:, j.idx_q] = rng.uniform(-0.5, 0.5, size=B)
        else:
            q[:, j.idx_q] = rng.uniform(-turns, turns, size=B)
    return q


# ---- comparing doubles with mpf ----------------------------------------------------------------------------------------
def _split(ref):
    """(hi, lo) doubles of a nested list of mpf: dev - hi is exact for a dev next to it, lo the rest."""
    fl = ek.flat(ref)
    hi = np.array([float(x) for x in fl])
    with mp.workdps(ek.DPS):
        lo = np.array([float(x - mp.mpf(h)) for x, h in zip(fl, hi)])
    return hi, lo


def _ratio(dev, ref, S):
    hi, lo = ref
    u = S + EPS * np.abs(hi).max()
    return float(np.abs((np.asarray(dev, dtype=np.float64).ravel() - hi) - lo).max() / u)


def _tables_fn(arr, fn):
    """fn(tables, ...) as a function of (placement, axis, frame_placement, ...) for ``spread``."""
    return lambda pl, ax, fp, *rest: fn(ek.tables(arr, placement=pl, axis=ax, frame_placement=fp, nf=len(arr.frames)), *rest)


# ---- references, computed once per model --------------------------------------------------------------------------------
FK_B = {"one_z": 3, "rpr": 5, "tree15": 3, "arm12p": 3, "big30p": 3}


@functools.lru_cache(maxsize=None)
def _fk_reference(name):
    """Per instance: (poses (hi, lo), S_poses, Jacobians (hi, lo), S_jacobians) + the exact results themselves."""
    model, frames, arr = _arrays(name)
    q = _configurations(name, FK_B[name], seed=100 + len(name))
    out = []

    def both(t, qb):
        T, J = ek.kinematics(t, qb)
        return [ek.pose12(x) for x in T], J

    fn = _tables_fn(arr, both)
    for b in range(q.shape[0]):
        base = fn(arr.placement, arr.axis, arr.frame_placement, q[b])
        S = ek.spread(fn, [arr.placement, arr.axis, arr.frame_placement, q[b]], draws=2, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return q, out


def _device_fk(api, arr, q):
    B, nf, nv, nq = q.shape[0], len(arr.frames), arr.model.nv, arr.model.nq
    dm = api.model_create(arr.desc)
    d_q, d_T, d_J = api.alloc(8 * B * nq), api.alloc(8 * B * nf * 12), api.alloc(8 * B * nf * 6 * nv)
    api.put(d_q, q)
    api.fk(dm, B, d_q, d_T, d_J)
    api.sync()
    T, J = np.zeros((B, nf, 12)), np.zeros((B, nf, 6, nv))
    api.get(T, d_T), api.get(J, d_J)
    for p in (d_q, d_T, d_J):
        api.release(p)
    api.model_destroy(dm)
    return T, J


# ---- 0. the oracle's own exponential and logarithm against mpmath's ------------------------------------------------------
def test_oracle_expm_and_log6_agree_with_mpmath():
    xi = np.array([0.1, 0.2, 0.3, 0.3, -2.0, 2.2])
    with mp.workdps(ek.DPS):
        E = ek.exp6(xi)
        Em = mp.expm(mp.matrix(ek.hat6([mp.mpf(float(x)) for x in xi])))
        assert max(abs(E[i][j] - Em[i, j]) for i in range(4) for j in range(4)) < mp.mpf(10) ** -50
        # the logarithm inverts the exponential (its definition), also next to pi where mp.logm leaves the principal sheet
        for th in (2.0, np.pi - 1e-3, np.pi - 1e-12):
            x = np.r_[0.1, -0.2, 0.3, np.array([0.6, -0.48, 0.64]) * th]
            L = ek.log6(ek.exp6(x))
            assert max(abs(a - mp.mpf(float(b))) for a, b in zip(L, x)) < mp.mpf(10) ** -35
        T = np.array([[float(x) for x in row] for row in E])  # rounded: no longer exactly in SE(3)
        a, b = ek.log6(T), ek.log6_logm(T)
        assert max(abs(x - y) for x, y in zip(a, b)) < 1e-15
        # Jlog6 against central differences of mp.logm (oracle/se3_oracle.py)
        from oracle.se3_oracle import jlog6_mp

        J = np.array([[float(x) for x in row] for row in ek.jlog6(T)])
        assert np.abs(J - jlog6_mp(T)).max() < 1e-14


# ---- 1. fast_sincos -----------------------------------------------------------------------------------------------------
# the doubles below 1e5 that lie closest to a multiple of pi/2 (found by rounding k pi/2, k = 1 .. 63661, to doubles
# in 60-digit arithmetic and sorting by the distance): 6.2e-19 ... 2e-16 away
_NEAR_MULTIPLES = [45.553093477052, 91.106186954104, 182.212373908208, 364.424747816416, 728.849495632832, 1457.698991265664,
                   2915.397982531328, 5830.795965062656, 11661.591930125313, 46066.74387591393, 23323.183860250625, 92133.48775182786]


def _sincos_inputs():
    t = [0.0, 5e-324, 1e-300, 2.2250738585072014e-308, 1e-20, 1e-9]
    for k in range(1, 9):
        x = float(k * mp.pi / 4)
        for n in range(-3, 4):
            y = x
            for _ in range(abs(n)):
                y = np.nextafter(y, np.inf if n > 0 else -np.inf)
            t.append(float(y))
    t += _NEAR_MULTIPLES
    t += list(np.logspace(-6, np.log10(99999.0), 160))
    t = np.array(t)
    return np.concatenate([t, -t[1:]])


@functools.lru_cache(maxsize=None)
def _sincos_reference():
    t = _sincos_inputs()
    with mp.workdps(ek.DPS):
        return t, _split([mp.sin(mp.mpf(float(x))) for x in t]), _split([mp.cos(mp.mpf(float(x))) for x in t])


def _ulps(dev, ref):
    hi, lo = ref
    err = np.abs((dev - hi) - lo)
    return np.where(hi == 0.0, np.where(dev == 0.0, 0.0, np.inf), err / np.spacing(np.abs(hi)))


def test_sincos_of_the_joint_angle_within_2_ulp(api):
    """``one_z``: T[0, 0] and T[1, 0] of the frame are bit for bit the cos and sin that rot_axis received.  2 ulp =
    fdlibm's kernels (< 1 ulp) + the half ulp of the reduced argument, whose derivative is at most 1."""
    _, _, arr = _arrays("one_z")
    t, sref, cref = _sincos_reference()
    assert np.abs(t).max() < 1e5 and len(t) % 64 != 0
    T, _ = _device_fk(api, arr, t[:, None].copy())
    us, uc = _ulps(T[:, 0, 3], sref), _ulps(T[:, 0, 0], cref)
    i = int(np.argmax(np.maximum(us, uc)))
    print(f"{_backend(api)}: sin {us.max():.3f} ulp, cos {uc.max():.3f} ulp, worst at t = {t[i]!r}")
    _note(_backend(api), "sincos_ulp", max(us.max(), uc.max()))
    assert us.max() <= 2.0 and uc.max() <= 2.0, (t[i], us[i], uc[i])
    assert (T[:, 0, 9:] == 0.0).all()


# ---- 2. / 3. poses and body Jacobians -------------------------------------------------------------------------------------
def _host_fk(model, frames, q):
    T = np.zeros((q.shape[0], len(frames), 12))
    J = np.zeros((q.shape[0], len(frames), 6, model.nv))
    for b in range(q.shape[0]):
        cfg = Configuration(model, q[b])
        for f, name in enumerate(frames):
            T[b, f], J[b, f] = pose12(cfg.get_transform_frame_to_world(name)), cfg.get_frame_jacobian(name)
    return T, J


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_fk_poses_and_body_jacobians(api, name):
    model, frames, arr = _arrays(name)
    q, ref = _fk_reference(name)
    T, J = _device_fk(api, arr, q)
    rows = {"host": _host_fk(model, frames, q)} if _backend(api) == "emu" else {}
    rows[_backend(api)] = (T, J)  # (last: the assertions below are on it)
    for who, (Tw, Jw) in rows.items():
        rp = max(_ratio(Tw[b], ref[b][0], ref[b][1]) for b in range(q.shape[0]))
        rj = max(_ratio(Jw[b], ref[b][2], ref[b][3]) for b in range(q.shape[0]))
        _note(who, "poses", rp)
        _note(who, "jacobians", rj)
    assert rp <= K_POSES and rj <= K_JACOBIANS  # (the device's: it is the last entry of rows)
    # exact structure: a prismatic column has no angular part; a joint that is not an ancestor of the frame has no column
    for f, fname in enumerate(frames):
        on_path, j = set(), int(arr.frame_joint[f])
        while j >= 0:
            on_path.add(j)
            j = int(arr.parent[j])
        for jn, jt in enumerate(model.joints):
            cols = slice(jt.idx_v, jt.idx_v + jt.nv)
            if jn not in on_path:
                assert (J[:, f, :, cols] == 0.0).all(), (fname, jt.name)
            else:
                assert np.abs(J[:, f, :, cols]).max() > 0.0
                if jt.kind == "prismatic":
                    assert (J[:, f, 3:, cols] == 0.0).all(), (fname, jt.name)


# ---- 4. the fused kernel's task rows ---------------------------------------------------------------------------------------
_REGION_ANGLES = [0.2, 2.0, np.pi - 1e-3, 1e-4, np.pi - 0.3]  # series, closed form, near pi, series, closed form


@functools.lru_cache(maxsize=None)
def _fused_reference(name):
    from pink_amd.lie import exp6

    model, frames, arr = _arrays(name)
    q, fk = _fk_reference(name)
    B, nf = q.shape[0], len(frames)
    rng = np.random.default_rng(300 + len(name))
    Tt = np.zeros((B, nf, 12))
    for b in range(B):
        cfg = Configuration(model, q[b])
        for f, fname in enumerate(frames):
            ax = rng.normal(size=3)
            th = _REGION_ANGLES[(b + f) % len(_REGION_ANGLES)]
            Tt[b, f] = pose12(cfg.get_transform_frame_to_world(fname) * exp6(np.r_[0.2 * rng.normal(size=3), ax / np.linalg.norm(ax) * th]))

    def rows(t, qb, Ttb):
        T, J = ek.kinematics(t, qb)
        e, Jt = [], []
        for f in range(nf):
            X = ek.pose_matrix(Ttb[f])
            e.append(ek.log6(ek.mm(ek.inverse(T[f]), X)))
            Jl = ek.jlog6(ek.mm(ek.inverse(X), T[f]))
            Jt.append([[-x for x in row] for row in ek.mm(Jl, J[f])])
        return e, Jt

    fn = _tables_fn(arr, rows)
    out = []
    for b in range(B):
        base = fn(arr.placement, arr.axis, arr.frame_placement, q[b], Tt[b])
        S = ek.spread(fn, [arr.placement, arr.axis, arr.frame_placement, q[b], Tt[b]], draws=1, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return q, Tt, out


@pytest.mark.parametrize("name", ["rpr", "tree15", "arm12p", "big30p"])
def test_fused_frame_task_rows(api, name):
    """pinkhip_fk_frame_tasks_device: e = log6(T_f^-1 T_t) and the rows -Jlog6(T_t^-1 T_f) J_body of every frame,
    with relative rotations in the series, the closed-form and the near-pi region of log3."""
    model, frames, arr = _arrays(name)
    q, Tt, ref = _fused_reference(name)
    B, nf, nv, nq = q.shape[0], len(frames), model.nv, model.nq
    dm = api.model_create(arr.desc)
    d_q, d_Tt, d_e, d_J = api.alloc(8 * B * nq), api.alloc(8 * B * nf * 12), api.alloc(8 * B * 6 * nf), api.alloc(8 * B * 6 * nf * nv)
    api.put(d_q, q), api.put(d_Tt, Tt)
    api.fk_frame_tasks(dm, B, d_q, d_Tt, None, d_e, 6 * nf, d_J, 6 * nf * nv)
    api.sync()
    e, J = np.zeros((B, nf, 6)), np.zeros((B, nf, 6, nv))
    api.get(e, d_e), api.get(J, d_J)
    for p in (d_q, d_Tt, d_e, d_J):
        api.release(p)
    api.model_destroy(dm)
    rows = {}
    if _backend(api) == "emu":
        eh, Jh = np.zeros_like(e), np.zeros_like(J)
        for b in range(B):
            cfg = Configuration(model, q[b])
            for f, fname in enumerate(frames):
                t = FrameTask(fname, 1.0, 1.0)
                t.set_target(SE3(Tt[b, f, :9].reshape(3, 3), Tt[b, f, 9:]))
                eh[b, f], Jh[b, f] = t.compute_error(cfg), t.compute_jacobian(cfg)
        rows["host"] = (eh, Jh)
    rows[_backend(api)] = (e, J)  # (last: the assertions below are on it)
    for who, (ew, Jw) in rows.items():
        re_ = max(_ratio(ew[b], ref[b][0], ref[b][1]) for b in range(B))
        rj = max(_ratio(Jw[b], ref[b][2], ref[b][3]) for b in range(B))
        _note(who, "e", re_)
        _note(who, "J", rj)
    assert re_ <= K_E and rj <= K_J


# ---- 5. the stand-alone frame-task kernel at the switches of log3 / Jlog6 ------------------------------------------------------
_PI = float(mp.pi)
_THETAS = {  # (one test case per entry: the 60-digit reference of six to eight poses takes a few seconds)
    "series": [0.0, 1e-9, 0.9e-8, 1.1e-8, 1e-6, 1e-3, 0.1, 0.5 - 1e-12],
    "closed": [0.5 + 1e-12, 1.0, 2.0, 3.0],
    "below_the_switch": [_PI - 1.01e-2],
    "near_pi_0.99e-2": [_PI - 0.99e-2],
    "near_pi_1e-4": [_PI - 1e-4],
    "near_pi_1e-8": [_PI - 1e-8],
    "near_pi_1e-12": [_PI - 1e-12],
}
_g = np.array([0.48, -0.6, 0.64])
# x-, y-, z-dominant, generic, one component exactly 0, and the negation of the generic one (both values of sg)
_AXES_PI = [np.array([0.9, 0.3, -0.2]), np.array([0.25, -0.9, 0.3]), np.array([-0.3, 0.2, 0.9]), _g, np.array([0.0, 0.6, -0.8]), -_g]


@functools.lru_cache(maxsize=None)
def _frame_task_reference(region):
    """Relative poses exp6(xi) in 60 digits, rounded to doubles; the reference is the log of the ROUNDED pose.
    T_frame = identity, T_target = X, J_body = I: e = log6(X), J_out = -Jlog6(X^-1)."""
    rng = np.random.default_rng(len(region))
    X = []
    for th in _THETAS[region]:
        for a in (_AXES_PI if th > 3.1 else [_g, -_g][:1 if th < 0.5 else 2]):
            a = a / np.linalg.norm(a)
            with mp.workdps(ek.DPS):
                E = ek.exp6(np.r_[0.3 * rng.normal(size=3), a * th])
            X.append([float(x) for x in ek.pose12(E)])
    X = np.array(X)

    def rows(x):
        M = ek.pose_matrix(x)
        Minv = ek.inverse(M)
        xi = ek.log6(M)
        return xi, [[-v for v in row] for row in ek.jlog6(Minv, xi=[-v for v in xi])]

    out = []
    for b in range(X.shape[0]):
        base = rows(X[b])
        S = ek.spread(rows, [X[b]], draws=2, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return X, out


@pytest.mark.parametrize("region", list(_THETAS))
def test_frame_task_kernel_at_the_switches_of_log3(api, region):
    from pink_amd.lie import Jlog6, log6

    X, ref = _frame_task_reference(region)
    B = X.shape[0]
    Tf = np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)], (B, 1))
    e, J = api.frame_task_terms(Tf, X, np.tile(np.eye(6), (B, 1, 1)))
    rows = {}
    if _backend(api) == "emu":
        M = [SE3(x[:9].reshape(3, 3), x[9:]) for x in X]
        rows["host"] = (np.array([log6(m) for m in M]), np.array([-Jlog6(m.inverse()) for m in M]))
    rows[_backend(api)] = (e, J)  # (last: the assertions below are on it)
    for who, (ew, Jw) in rows.items():
        re_ = [_ratio(ew[b], ref[b][0], ref[b][1]) for b in range(B)]
        rj = [_ratio(Jw[b], ref[b][2], ref[b][3]) for b in range(B)]
        _note(who, "e", max(re_))
        _note(who, "J", max(rj))
    assert max(re_) <= K_E, (int(np.argmax(re_)), max(re_))
    assert max(rj) <= K_J, (int(np.argmax(rj)), max(rj))


def test_frame_task_kernel_at_pi(api):
    """R = 2 a a^T - I rounded: as close to theta = pi as doubles get.  The sign of w is not determined there, so
    exp3(w_device) is compared with R; the Jacobian is not checked."""
    from pink_amd.lie import log6

    X = []
    for a in _AXES_PI[:5]:
        a = a / np.linalg.norm(a)
        X.append(np.r_[(2.0 * np.outer(a, a) - np.eye(3)).ravel(), 0.1, -0.2, 0.3])
    X = np.array(X)
    B = X.shape[0]
    Tf = np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)], (B, 1))
    e, _ = api.frame_task_terms(Tf, X, np.tile(np.eye(6), (B, 1, 1)))
    rows = {"host": np.array([log6(SE3(x[:9].reshape(3, 3), x[9:])) for x in X])} if _backend(api) == "emu" else {}
    rows[_backend(api)] = e  # (last: the assertion below is on it)
    for who, ew in rows.items():
        worst = 0.0
        for b in range(B):
            assert abs(np.linalg.norm(ew[b, 3:]) - np.pi) < 1e-7
            # S of the identity map R -> R: every entry moves by its own ulp
            worst = max(worst, _ratio(X[b, :9], _split(ek.exp3(ew[b, 3:])), float(np.spacing(np.abs(X[b, :9])).max())))
        _note(who, "e", worst)
    assert worst <= K_E


# ---- 6. q (+) dq ----------------------------------------------------------------------------------------------------------
_TWIST_NORMS = [0.0, 1e-9, 0.9e-8, 1.1e-8, 1e-4, 0.1 - 1e-12, 0.1 + 1e-12, 1.0, _PI, 4.0]


@functools.lru_cache(maxsize=None)
def _integrate_reference(name):
    model, frames, arr = _arrays(name)
    B = len(_TWIST_NORMS)
    q = _configurations(name, B, seed=500 + len(name), turns=3.0)
    rng = np.random.default_rng(600 + len(name))
    v = 0.3 * rng.normal(size=(B, model.nv))
    for b, n in enumerate(_TWIST_NORMS):
        w = rng.normal(size=3)
        v[b, 3:6] = w / np.linalg.norm(w) * n
        v[b, :3] = rng.normal(size=3)
    root = arr.idx_q[0] == 0 and int(arr.jtype[0]) == 2
    assert root  # the free-flyer is joint 0: its transform is compared; the scalar joints' q + v as numbers
    ff = ek.tables(arr, parent=arr.parent[:1], jtype=arr.jtype[:1], idx_q=arr.idx_q[:1], idx_v=arr.idx_v[:1])

    def fn(qb, vb):
        with mp.workdps(ek.DPS):
            return ek.pose12(ek.integrate(ff, qb, vb)[0]), [mp.mpf(float(a)) + mp.mpf(float(c)) for a, c in zip(qb[7:], vb[6:])]

    out = []
    for b in range(B):
        base = fn(q[b], v[b])
        S = ek.spread(fn, [q[b], v[b]], draws=4, seed=b, base=base)
        out.append((_split(base[0]), S[0], _split(base[1]), S[1]))
    return q, v, out


@pytest.mark.parametrize("name", ["tree15", "big30p"])
def test_integrate_at_the_switches_of_the_free_flyer(api, name):
    """pinkhip_integrate_device: angular parts of norm 0 ... 4 around the th < 1e-8 and th < 0.1 switches of
    integrate_joint.  Quaternions are defined up to sign: the joint transforms are compared."""
    model, frames, arr = _arrays(name)
    q, v, ref = _integrate_reference(name)
    B = q.shape[0]
    dm = api.model_create(arr.desc)
    d_q, d_v = api.alloc(8 * B * model.nq), api.alloc(8 * B * model.nv)
    api.put(d_q, q), api.put(d_v, v)
    api.integrate(dm, B, d_q, d_v)
    api.sync()
    q2 = np.zeros_like(q)
    api.get(q2, d_q)
    api.release(d_q), api.release(d_v)
    api.model_destroy(dm)
    rows = {"host": np.array([model.integrate(q[b], v[b]) for b in range(B)])} if _backend(api) == "emu" else {}
    rows[_backend(api)] = q2  # (last: the assertion below is on it)
    for who, qw in rows.items():
        worst = 0.0
        for b in range(B):
            hi, lo = ref[b][0]
            with mp.workdps(ek.DPS):
                M = ek.pose12(ek.joint_matrix(2, None, qw[b, :7]))  # the exact transform of the device's (p, quaternion)
                err = max(abs((x - mp.mpf(h)) - mp.mpf(l)) for x, h, l in zip(M, hi, lo))
            worst = max(worst, float(err) / (ref[b][1] + EPS * np.abs(hi).max()), _ratio(qw[b, 7:], ref[b][2], ref[b][3]))
        _note(who, "integrate", worst)
    assert worst <= K_INTEGRATE
    assert np.abs(np.linalg.norm(q2[:, 3:7], axis=1) - 1.0).max() <= 4 * EPS
