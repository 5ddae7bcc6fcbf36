"""H, c of one instance of a packed IKBatch in exact arithmetic -- the anchor of the stack-only kernels.

Restated from the definition only (pink/tasks/task.py:145-167, pink/solve_ik.py:54-67, pink/barriers/barrier.py:193-200);
nothing here knows of tiles, passes or chunks:

    H = damping I + sum_t (J_t^T W_t^2 J_t + mu_t I) + sum_barriers r / (||Gd_rows||_F^2 dt^2) I
    c = sum_t gain_t J_t^T W_t^2 e_t + c_extra,          mu_t = lm_t sum_k (gain_t w_k e_k)^2

over the dense tasks (rows of ``batch.J``) and the diagonal tasks (J_t = eye(nv)[col0:col0 + k], never stored).  Every
double is a dyadic rational, so the sums of products are formed in Python integers over a common power-of-two
denominator; the barrier regulariser divides and is carried as a ``fractions.Fraction``.  The arrays read are the ones
the kernel reads: ``batch.J / e / cost / gain / lm_damping / Gd / c_extra`` of instance ``b``.

Next to every entry stands its ABSOLUTE-TERM SUM S: the same sum with every product replaced by its absolute value.
Any fp64 evaluation of a sum of n such products -- in any order, with or without FMA, each product with a few roundings
of its own -- is within (n + 8) 2^-52 S of the exact value (``ExactStack.violations``); an entry with S = 0 is exactly 0.

About 0.3 s per instance at nv = 64, Kd = 160.
"""
from dataclasses import dataclass
from fractions import Fraction
from typing import List

import numpy as np

TASK_DIAGONAL = 1
ULP = Fraction(1, 2 ** 52)


def _ints(x):
    """Doubles -> (object array of Python ints n, power-of-two D) with x == n / D exactly."""
    x = np.asarray(x, dtype=np.float64)
    ratios = [float(v).as_integer_ratio() for v in x.ravel()]
    D = max((d for _, d in ratios), default=1)
    out = np.empty(len(ratios), dtype=object)
    out[:] = [n * (D // d) for n, d in ratios]
    return out.reshape(x.shape), D


@dataclass
class ExactStack:
    """Exact ``H [nv][nv]``, ``c [nv]`` (Fractions), their absolute-term sums ``SH``, ``Sc`` and the number of terms
    ``nH [nv][nv]``, ``nc [nv]`` each entry is a sum of: Kd dense-row products, plus the terms that touch it -- a
    diagonal task's w^2 or gain w^2 e, mu_t of each task with LM damping, the damping, each barrier's regulariser,
    c_extra."""

    nv: int
    H: List[List[Fraction]]
    SH: List[List[Fraction]]
    nH: List[List[int]]
    c: List[Fraction]
    Sc: List[Fraction]
    nc: List[int]

    def ratios(self, H, c):
        """``|value - exact| / (2^-52 S)`` per entry of a computed ``H [nv, nv]``, ``c [nv]`` (floats; inf where S = 0 and
        the value is not 0) and whether the entry is beyond ``(n + 8) 2^-52 S`` (decided in exact arithmetic)."""
        nv = self.nv
        rH, bH = np.zeros((nv, nv)), np.zeros((nv, nv), bool)
        rc, bc = np.zeros(nv), np.zeros(nv, bool)
        for i in range(nv):
            rc[i], bc[i] = _ratio(c[i], self.c[i], self.Sc[i], self.nc[i])
            for j in range(nv):
                rH[i, j], bH[i, j] = _ratio(H[i, j], self.H[i][j], self.SH[i][j], self.nH[i][j])
        return rH, bH, rc, bc


def _ratio(value, exact, S, n):
    value = float(value)
    if not np.isfinite(value):
        return np.inf, True
    err = abs(Fraction(value) - exact)
    bad = err > (n + 8) * ULP * S
    if S == 0:
        return (0.0 if err == 0 else np.inf), bad
    return float(err / (ULP * S)), bad


def exact_stack(batch, b):
    """``ExactStack`` of instance ``b`` of the packed ``batch``."""
    nv, Kd, K = batch.nv, batch.Kd, batch.K
    rows = [int(r) for r in batch.task_rows]
    cost = np.asarray(batch.cost)
    w = cost[b] if cost.ndim == 2 else cost
    gain, lm = np.zeros(K), np.zeros(K)
    for t in range(batch.T):
        gain[rows[t]:rows[t + 1]] = batch.gain[t]
        lm[rows[t]:rows[t + 1]] = batch.lm_damping[t]
    JI, DJ = _ints(batch.J[b])
    wI, Dw = _ints(w)
    eI, De = _ints(batch.e[b])
    gI, Dg = _ints(gain)
    lI, Dl = _ints(lm)
    w2 = wI * wI  # / Dw^2
    gw2e = gI * w2 * eI  # / (Dg Dw^2 De): gain w^2 e per row
    mu_rows = lI * gI * gI * w2 * eI * eI  # / (Dl Dg^2 Dw^2 De^2): lm (gain w e)^2 per row, all >= 0
    DH, Dc, Dmu = Dw * Dw * DJ * DJ, Dg * Dw * Dw * De * DJ, Dl * Dg * Dg * Dw * Dw * De * De

    H = [[Fraction(0)] * nv for _ in range(nv)]
    SH = [[Fraction(0)] * nv for _ in range(nv)]
    nH = [[Kd] * nv for _ in range(nv)]
    c, Sc, nc = [Fraction(0)] * nv, [Fraction(0)] * nv, [Kd] * nv
    if Kd:
        Jd, JA = JI[:Kd], abs(JI[:Kd])
        A, AA = w2[:Kd, None] * Jd, w2[:Kd, None] * JA  # exact rows once: W^2 J and its absolute values
        for i in range(nv):  # upper triangle, mirrored
            hi, si = A[:, i].dot(Jd[:, i:]), AA[:, i].dot(JA[:, i:])
            for j in range(i, nv):
                H[i][j] = H[j][i] = Fraction(int(hi[j - i]), DH)
                SH[i][j] = SH[j][i] = Fraction(int(si[j - i]), DH)
        ci, sci = gw2e[:Kd].dot(Jd), abs(gw2e[:Kd]).dot(JA)
        c = [Fraction(int(v), Dc) for v in ci]
        Sc = [Fraction(int(v), Dc) for v in sci]

    # what every diagonal entry receives: damping, the LM terms of all tasks (one per row), the barrier regularisers
    diag, n_diag = Fraction(float(batch.damping)), 1 if batch.damping != 0.0 else 0
    for t in range(batch.T):  # mu_t I: one term per task with a non-zero mu_t
        mu_t = int(mu_rows[rows[t]:rows[t + 1]].sum()) if rows[t + 1] > rows[t] else 0
        diag += Fraction(mu_t, Dmu)
        n_diag += 1 if mu_t else 0
    brows = [int(r) for r in batch.barrier_rows]
    for t, r in enumerate(np.asarray(batch.barrier_safe_gain, dtype=np.float64)):
        if r > 1e-6:  # barrier.py:193
            GI, DG = _ints(batch.Gd[b, brows[t]:brows[t + 1]])
            norm2 = Fraction(int((GI * GI).sum()), DG * DG)  # ||J_h||_F^2 = ||Gd_rows||_F^2 dt^2
            diag += Fraction(float(r)) / (norm2 * Fraction(float(batch.dt)) ** 2)
            n_diag += 1
    for i in range(nv):
        H[i][i] += diag
        SH[i][i] += diag  # (every one of these terms is >= 0)
        nH[i][i] += n_diag
    # diagonal tasks: J = eye[col0:col0 + k]
    for t in range(batch.T):
        if int(batch.task_kind[t]) != TASK_DIAGONAL:
            continue
        c0 = int(batch.task_col0[t])
        for r in range(rows[t], rows[t + 1]):
            i = c0 + r - rows[t]
            H[i][i] += Fraction(int(w2[r]), Dw * Dw)
            SH[i][i] += Fraction(int(w2[r]), Dw * Dw)
            nH[i][i] += 1
            c[i] += Fraction(int(gw2e[r]), Dg * Dw * Dw * De)
            Sc[i] += Fraction(abs(int(gw2e[r])), Dg * Dw * Dw * De)
            nc[i] += 1
    if batch.c_extra is not None:
        for i in range(nv):
            x = Fraction(float(batch.c_extra[b, i]))
            c[i] += x
            Sc[i] += abs(x)
            nc[i] += 1
    return ExactStack(nv, H, SH, nH, c, Sc, nc)
