"""The kinematics half in 60-digit arithmetic (TEST INFRASTRUCTURE ONLY).

What ``oracle/exact_qp.py`` is to the solvers: a restatement from the DEFINITIONS -- products of 4 x 4 homogeneous
matrices, matrix exponentials of twist matrices as power series, logarithms as the inverse of that exponential,
Jacobians as central differences with a step of 1e-25 -- evaluated with mpmath, so that the error of the reference
(< 1e-40) is nothing next to the round-off of the fp64 code under test.  None of the closed forms of the kernels
(Rodrigues, the alpha / beta coefficients of log6 / Jlog6, the quaternion product of ``integrate_joint``) appears here.

The model is passed as the plain tables of ``pink_amd.rollout.ModelArrays`` (any object with ``parent``, ``jtype``,
``idx_q``, ``idx_v``, ``placement``, ``axis``, ``frame_joint``, ``frame_placement``), as for
``oracle/kinematics_oracle.py``.  Twists are ``[linear; angular]``, Jacobians are body (LOCAL) Jacobians.

Matrices are nested lists of ``mpf`` (mpmath's own matrix class costs the same per product and more per element
access).  ``expm`` is the Taylor series with scaling and squaring; ``tests/test_kinematics_exact.py`` holds it to
``mp.expm``.  ``log6`` solves ``expm(hat(xi)) = T`` by a Newton iteration whose residual is the Mercator series of a
matrix next to the identity: the fixed point is defined by the exponential alone (the fp64 starting value and
preconditioner only decide how fast it is reached); the same test holds it to ``mp.logm``, which is ten times slower.
"""

from __future__ import annotations

from types import SimpleNamespace

import mpmath as mp
import numpy as np

DPS = 60
H_FD = mp.mpf(10) ** -25  # central differences: truncation ~1e-50, round-off 1e-60 / 1e-25

REVOLUTE, PRISMATIC, FREE_FLYER = 0, 1, 2


def precise(fn):
    """Run ``fn`` with ``DPS`` digits."""

    def wrapped(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)

    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


# ---- small dense matrices ---------------------------------------------------------------------------------------------
def eye(n):
    return [[mp.mpf(1 if i == j else 0) for j in range(n)] for i in range(n)]


def mm(A, B):
    n, m, p = len(A), len(B), len(B[0])
    if m == 4:  # (written out: this is where the time goes)
        b0, b1, b2, b3 = B
        return [[a[0] * b0[j] + a[1] * b1[j] + a[2] * b2[j] + a[3] * b3[j] for j in range(p)] for a in A]
    if m == 3:
        b0, b1, b2 = B
        return [[a[0] * b0[j] + a[1] * b1[j] + a[2] * b2[j] for j in range(p)] for a in A]
    return [[sum((A[i][k] * B[k][j] for k in range(1, m)), A[i][0] * B[0][j]) for j in range(p)] for i in range(n)]


def mat(a):
    """Nested list of mpf from anything array-like (doubles convert exactly)."""
    return [[mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in row] for row in np.asarray(a, dtype=object)]


def pose_matrix(T12):
    """4 x 4 matrix of a 12-double pose (rotation row-major, then translation)."""
    T12 = [mp.mpf(float(x)) for x in T12]
    return [T12[0:3] + [T12[9]], T12[3:6] + [T12[10]], T12[6:9] + [T12[11]], [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]]


def pose12(T):
    """The 12 entries (rotation row-major, translation) of a 4 x 4 matrix, as mpf."""
    return [T[i][j] for i in range(3) for j in range(3)] + [T[0][3], T[1][3], T[2][3]]


def inverse(A):
    n = len(A)
    M = mp.inverse(mp.matrix(A))
    return [[M[i, j] for j in range(n)] for i in range(n)]


def hat3(w):
    z = mp.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def hat6(xi):
    """Twist matrix of ``[v; w]``."""
    z = mp.mpf(0)
    v, w = xi[:3], xi[3:]
    return [[z, -w[2], w[1], v[0]], [w[2], z, -w[0], v[1]], [-w[1], w[0], z, v[2]], [z, z, z, z]]


def expm(A):
    """Matrix exponential from its power series: scaled by 2^-s to a norm below 1/16, summed until the terms drop
    below 10^-(digits + 5), squared s times."""
    n = len(A)
    nrm = max(sum(abs(x) for x in row) for row in A)
    s = 0 if nrm == 0 else max(0, int(mp.ceil(mp.log(nrm, 2))) + 4)
    sc = mp.mpf(2) ** -s
    As = [[x * sc for x in row] for row in A]
    tol = mp.mpf(10) ** -(mp.mp.dps + 5)
    E, term, k = eye(n), eye(n), 1
    while True:
        term = [[x / k for x in row] for row in mm(term, As)]
        E = [[E[i][j] + term[i][j] for j in range(n)] for i in range(n)]
        if max(abs(x) for row in term for x in row) < tol:
            break
        k += 1
    for _ in range(s):
        E = mm(E, E)
    return E


def log_near_identity(D):
    """log(D) = E - E^2 / 2 + E^3 / 3 - ... with E = D - I, for |E| < 1e-3 (Mercator series)."""
    n = len(D)
    E = [[D[i][j] - (1 if i == j else 0) for j in range(n)] for i in range(n)]
    nrm = max(sum(abs(x) for x in row) for row in E)
    if nrm > mp.mpf("1e-3"):
        raise ValueError("log_near_identity: |D - I| = %s" % mp.nstr(nrm, 5))
    tol = mp.mpf(10) ** -(mp.mp.dps + 5)
    L, P, k = [row[:] for row in E], E, 1
    while nrm ** (k + 1) > tol * max(nrm, tol):  # terms relative to the leading one
        k += 1
        P = mm(P, E)
        sg = -1 if k % 2 == 0 else 1
        L = [[L[i][j] + sg * P[i][j] / k for j in range(n)] for i in range(n)]
    return L


def vee6(L):
    """``[v; w]`` of a 4 x 4 matrix: the translation column and the skew part of the rotation block."""
    return [L[0][3], L[1][3], L[2][3], (L[2][1] - L[1][2]) / 2, (L[0][2] - L[2][0]) / 2, (L[1][0] - L[0][1]) / 2]


@precise
def exp6(xi):
    return expm(hat6([mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in xi]))


@precise
def exp3(w):
    return expm(hat3([mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in w]))


def _right_jacobian_series(xi, terms=60):
    """fp64 sum of (-1)^k ad^k / (k + 1)!: only the preconditioner of the Newton iteration in ``log6``."""
    v, w = xi[:3], xi[3:]
    hw = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    hv = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    ad = np.block([[hw, hv], [np.zeros((3, 3)), hw]])
    J, P = np.eye(6), np.eye(6)
    for k in range(1, terms):
        P = -P @ ad / (k + 1)
        J = J + P
    return J


@precise
def log6(T, start=None):
    """The twist ``[v; w]``, ``|w| <= pi``, with ``expm(hat(xi)) = T``.  ``T``: 4 x 4 (nested list of mpf or array).
    For a ``T`` that is not exactly in SE(3) (a pose rounded to doubles) the residual that cannot be removed by any
    twist is left where it is; what is solved is vee(log(expm(-hat(xi)) T)) = 0."""
    T = mat(T)
    if start is None:
        import warnings

        from scipy.linalg import logm

        with warnings.catch_warnings():  # ("logm result may be inaccurate" next to pi: it is only where the iteration starts)
            warnings.simplefilter("ignore")
            L0 = np.real(logm(np.array([[float(x) for x in row] for row in T])))
        start = np.array([float(x) for x in vee6(L0.tolist())])
    xi = [mp.mpf(float(x)) for x in start]
    # each step multiplies the error by ~1e-15 (the accuracy of the fp64 preconditioner): the step taken on a residual
    # below 1e-25 leaves less than 1e-39
    tol = mp.mpf(10) ** -25
    flipped = False
    for it in range(40):
        D = mm(expm(hat6([-x for x in xi])), T)
        E = [[D[i][j] - (1 if i == j else 0) for j in range(4)] for i in range(4)]
        nrm = max(sum(abs(x) for x in row) for row in E)
        if nrm > mp.mpf("1e-3"):  # a poor start (fp64 logm next to pi): one plain step on the linear term
            r = vee6(E)
        else:
            r = vee6(log_near_identity(D))
        M = np.linalg.inv(_right_jacobian_series(np.array([float(x) for x in xi])))
        step = [mp.fsum(mp.mpf(float(M[i, k])) * r[k] for k in range(6)) for i in range(6)]
        xi = [xi[i] + step[i] for i in range(6)]
        if max(abs(x) for x in r) < tol:
            th = mp.sqrt(xi[3] ** 2 + xi[4] ** 2 + xi[5] ** 2)
            if th <= mp.pi or flipped:
                return xi
            # converged on the other sheet (angle 2 pi - theta about the opposite axis): move to the principal one
            flipped = True
            w2 = [x * (1 - 2 * mp.pi / th) for x in xi[3:]]
            xi = xi[:3] + w2
    raise ArithmeticError("log6: no convergence")


@precise
def log6_logm(T):
    """The same through ``mp.logm`` (inverse scaling and squaring): the cross-check of ``log6``."""
    L = mp.logm(mp.matrix(mat(T)))
    return [mp.re(x) for x in vee6([[L[i, j] for j in range(4)] for i in range(4)])]


@precise
def right_jacobian_exp6(xi):
    """``Jr`` with ``expm(hat(xi + d)) = expm(hat(xi)) expm(hat(Jr d))`` to first order, by central differences."""
    xi = [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in xi]
    Einv = expm(hat6([-x for x in xi]))
    J = [[None] * 6 for _ in range(6)]
    for k in range(6):
        col = []
        for sg in (1, -1):
            x2 = xi[:]
            x2[k] = x2[k] + sg * H_FD
            col.append(vee6(log_near_identity(mm(Einv, expm(hat6(x2))))))
        for r in range(6):
            J[r][k] = (col[0][r] - col[1][r]) / (2 * H_FD)
    return J


@precise
def jlog6(T, xi=None):
    """d log6(T expm(hat(d))) / d d at 0 (the right Jacobian of the logarithm): log6(T exp(d)) = xi + Jlog d and
    exp(xi + e) = T exp(Jr e) make it the inverse of ``right_jacobian_exp6(log6(T))``; the differences are taken
    next to the identity, so no step can straddle the cut of the logarithm at an angle of pi."""
    xi = log6(T) if xi is None else xi
    return inverse(right_jacobian_exp6(xi))


# ---- models -----------------------------------------------------------------------------------------------------------
def tables(arr, **replace):
    """A light copy of the model tables with some of them replaced (``spread`` perturbs placements and axes)."""
    d = {k: getattr(arr, k) for k in ("parent", "jtype", "idx_q", "idx_v", "placement", "axis", "frame_joint", "frame_placement")}
    d["nf"] = len(arr.frames) if hasattr(arr, "frames") else arr.nf
    d.update(replace)
    return SimpleNamespace(**d)


def _nf(arr):
    return arr.nf if hasattr(arr, "nf") else len(arr.frames)


def quat_matrix(qv):
    """Rotation of the quaternion (x, y, z, w) / |.| through the exponential of its rotation vector."""
    x, y, z, w = [mp.mpf(float(c)) if not isinstance(c, mp.mpf) else c for c in qv]
    n = mp.sqrt(x * x + y * y + z * z)
    if n == 0:
        return eye(3)
    ang = 2 * mp.atan2(n, w)
    return expm(hat3([x / n * ang, y / n * ang, z / n * ang]))


def joint_matrix(jtype, axis, qj):
    """Motion of one joint: expm of its twist matrix (revolute, prismatic), or (rotation of the quaternion,
    translation) for the free-flyer, whose configuration is a pose already."""
    if jtype == FREE_FLYER:
        R = quat_matrix(qj[3:7])
        p = [mp.mpf(float(c)) if not isinstance(c, mp.mpf) else c for c in qj[:3]]
        return [R[0] + [p[0]], R[1] + [p[1]], R[2] + [p[2]], [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]]
    a = [mp.mpf(float(c)) for c in axis]
    q0 = mp.mpf(float(qj[0])) if not isinstance(qj[0], mp.mpf) else qj[0]
    if jtype == REVOLUTE:
        return expm(hat6([0, 0, 0] + [c * q0 for c in a]))
    return expm(hat6([c * q0 for c in a] + [0, 0, 0]))


def _generators(jtype, axis):
    """Twist matrices of the joint's tangent directions (in the joint's own frame)."""
    if jtype == FREE_FLYER:
        return [hat6([mp.mpf(1 if i == k else 0) for i in range(6)]) for k in range(6)]
    a = [mp.mpf(float(c)) for c in axis]
    z = [mp.mpf(0)] * 3
    return [hat6(z + a if jtype == REVOLUTE else a + z)]


def _chain(arr, q):
    nj = len(arr.parent)
    A, oM = [], []
    for j in range(nj):
        jt = int(arr.jtype[j])
        iq = int(arr.idx_q[j])
        X = joint_matrix(jt, arr.axis[j], q[iq:iq + (7 if jt == FREE_FLYER else 1)])
        A.append(mm(pose_matrix(arr.placement[j]), X))
        p = int(arr.parent[j])
        oM.append(A[j] if p < 0 else mm(oM[p], A[j]))
    return A, oM


@precise
def joint_poses(arr, q):
    return _chain(arr, q)[1]


@precise
def kinematics(arr, q, jacobians=True):
    """World poses of the frames, ``[nf]`` 4 x 4, and their body Jacobians ``[nf][6][nv]`` (or ``None``): column j
    is (log6(T^-1 T(q (+) h e_j)) - log6(T^-1 T(q (+) -h e_j))) / 2h with h = 1e-25; the step moves joint j by
    expm(+-h G) on the right of its motion, G the twist matrix of the tangent direction, and every pose behind it
    is recomposed.  A column whose joint is not on the frame's path to the world is zero because nothing moves."""
    A, oM = _chain(arr, q)
    nf = _nf(arr)
    nv = sum(6 if int(t) == FREE_FLYER else 1 for t in arr.jtype)
    Ts, Js = [], []
    for f in range(nf):
        Fp, jf = pose_matrix(arr.frame_placement[f]), int(arr.frame_joint[f])
        T = Fp if jf < 0 else mm(oM[jf], Fp)
        Ts.append(T)
        if not jacobians:
            continue
        J = [[mp.mpf(0)] * nv for _ in range(6)]
        Tinv = inverse(T)
        S, j = Fp, jf  # S = (pose of joint j in the world)^-1 T, built from the frame towards the root
        while j >= 0:
            iv = int(arr.idx_v[j])
            for k, G in enumerate(_generators(int(arr.jtype[j]), arr.axis[j])):
                logs = []
                for sg in (1, -1):
                    step = expm([[x * (sg * H_FD) for x in row] for row in G])
                    logs.append(vee6(log_near_identity(mm(Tinv, mm(mm(oM[j], step), S)))))
                for r in range(6):
                    J[r][iv + k] = (logs[0][r] - logs[1][r]) / (2 * H_FD)
            S = mm(A[j], S)
            j = int(arr.parent[j])
        Js.append(J)
    return Ts, (Js if jacobians else None)


@precise
def integrate(arr, q, v):
    """``q (+) v`` as joint motions ``[nj]`` 4 x 4: the free-flyer's pose times expm of the twist matrix of its six
    tangent entries, the scalar joints at q + v."""
    out = []
    for j in range(len(arr.parent)):
        jt, iq, iv = int(arr.jtype[j]), int(arr.idx_q[j]), int(arr.idx_v[j])
        if jt == FREE_FLYER:
            out.append(mm(joint_matrix(jt, None, q[iq:iq + 7]), expm(hat6([mp.mpf(float(x)) for x in v[iv:iv + 6]]))))
        else:
            out.append(joint_matrix(jt, arr.axis[j], [mp.mpf(float(q[iq])) + mp.mpf(float(v[iv]))]))
    return out


# ---- conditioning -----------------------------------------------------------------------------------------------------
def ulp_moved(a, rng):
    """Every non-zero entry moved to a neighbouring double, up or down at random (zeros are structure: they stay)."""
    a = np.asarray(a, dtype=np.float64)
    up = rng.integers(0, 2, size=a.shape).astype(bool)
    moved = np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))
    return np.where(a == 0.0, a, moved)


def flat(x):
    """Flatten nested lists / arrays of mpf or floats."""
    if isinstance(x, (list, tuple)):
        out = []
        for y in x:
            out += flat(y)
        return out
    if isinstance(x, np.ndarray):
        return flat(x.tolist())
    return [x]


def spread(fn, inputs, draws=8, seed=0, base=None):
    """The unit of the tolerances: how far the exact result moves when the doubles it is computed from each move by
    one ulp.  ``fn(*inputs)`` returns (nested lists of) mpf or a tuple of them; the answer is the largest change
    of any entry over ``draws`` random +-1 ulp copies of ``inputs`` -- one number per member of the tuple.
    ``base``: ``fn(*inputs)`` if the caller has it already."""
    rng = np.random.default_rng(seed)
    base = fn(*inputs) if base is None else base
    single = not isinstance(base, tuple)
    b = [flat(base)] if single else [flat(x) for x in base]
    S = [mp.mpf(0)] * len(b)
    with mp.workdps(DPS):
        for _ in range(draws):
            out = fn(*[ulp_moved(a, rng) for a in inputs])
            o = [flat(out)] if single else [flat(x) for x in out]
            for i in range(len(b)):
                S[i] = max([S[i]] + [abs(x - y) for x, y in zip(o[i], b[i])])
    S = [float(s) for s in S]
    return S[0] if single else S
