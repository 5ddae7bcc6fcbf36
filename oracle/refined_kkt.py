"""Batched high-precision minimiser of the IK QP (TEST INFRASTRUCTURE ONLY: tests/).

The same computation as ``oracle/exact_qp.py`` -- ``P, q`` formed from the task rows as ``_objective_mp`` forms them, the
KKT system of an active set solved, rows exchanged until primal feasibility and the multiplier signs certify the point --
at thousands of instances a second instead of one:

* ``P, q`` in ``np.longdouble`` (64-bit significand on x86-64) from the fp64 task rows, not from the fp64 ``H``;
* the KKT system of every instance's active set solved by fp64 LU, then iteratively refined on residuals formed in
  ``longdouble`` until the correction is below ``1e-15 max(1, |x|)``, or has stopped shrinking at the noise floor of the
  longdouble residual (at most ``MAX_REFINE`` steps).  The forward error is then ~``cond * 2^-64 |x|`` instead of
  ``cond * 2^-53 |x|``: measured 3e-15 at kappa 1e5, 2e-13 at 5e6, 2e-11 at 2e9, 1e-9 at 2e10 (the last correction,
  ``info["floor"]`` relative to ``max(1, |x|)``, is that estimate per instance);
* the active set starts from the union of the rows the candidate points meet (the C oracle's and the kernel's), the
  pinned pairs (``lb = ub``) as one equality, duplicated rows once (the tighter);
* exchanges (the most negative multiplier leaves, else the most violated row enters) run, one per instance and round,
  until the ``longdouble`` certificate holds.  An instance that does not settle within ``MAX_EXCHANGES`` -- or whose
  refinement does not converge -- is handed to ``exact_minimiser`` (50 digits) and counted in ``info["fallback"]``.

Instances of one call share ``nv``, the task layout and the number of rows of ``G``.
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

LD = np.longdouble
MAX_REFINE = 8
MAX_EXCHANGES = 12
CERT_TOL = 1e-17  # relative slack / multiplier tolerance of the certificate (longdouble round-off is ~5e-20)


def objective_ld(J, e, cost, gain, lm, rows, damping, diag_extra=None, c_extra=None):
    """``P [B, nv, nv]``, ``q [B, nv]`` in longdouble: ``W = diag(cost)``, ``shift = damping + diag_extra + sum_t lm_t ||W_t a_t e_t||^2``,
    ``P = sum (WJ)^T (WJ) + shift I``, ``q = -sum (W a e)^T (WJ) + c_extra`` (exact_qp._objective_mp)."""
    J = np.asarray(J, float)
    B, _, nv = J.shape
    cost = np.broadcast_to(np.asarray(cost, float), J.shape[:2]).astype(LD)
    WJ = cost[..., None] * J.astype(LD)
    P = np.zeros((B, nv, nv), LD)
    q = np.zeros((B, nv), LD)
    shift = np.full(B, LD(float(damping)), LD)
    if diag_extra is not None:
        shift += np.broadcast_to(np.asarray(diag_extra, float), (B,)).astype(LD)
    for t in range(len(rows) - 1):
        r0, r1 = int(rows[t]), int(rows[t + 1])
        if r1 == r0:
            continue
        We = -LD(float(gain[t])) * cost[:, r0:r1] * np.asarray(e, float)[:, r0:r1].astype(LD)
        shift += LD(float(lm[t])) * (We * We).sum(axis=1)
        A = WJ[:, r0:r1]
        P += np.einsum("bki,bkj->bij", A, A)
        q -= np.einsum("bk,bki->bi", We, A)
    P[:, np.arange(nv), np.arange(nv)] += shift[:, None]
    if c_extra is not None:
        q += np.broadcast_to(np.asarray(c_extra, float), (B, nv)).astype(LD)
    return P, q


def _row_structure(G, h, meq):
    """Per instance: rows kept (finite bound), ``eq`` (equalities and the first row of each pinned pair), ``cand`` (rows that
    may enter: of each set of identical normals the tightest, never the partner of a pinned pair)."""
    B, r, _ = G.shape
    keep = np.isfinite(h) & (np.abs(h) < 1e29)
    eq = np.zeros((B, r), bool)
    eq[:, :meq] = keep[:, :meq]
    cand = keep.copy()
    cand[:, :meq] = False
    for b in range(B):
        idx = [i for i in range(meq, r) if keep[b, i]]
        if not idx:
            continue
        key = {}
        for i in idx:
            k = (G[b, i] + 0.0).tobytes()
            j = key.get(k)
            if j is None or h[b, i] < h[b, j]:
                if j is not None:
                    cand[b, j] = False
                key[k] = i
            else:
                cand[b, i] = False
        for k, i in list(key.items()):
            if not cand[b, i]:
                continue
            j = key.get((-G[b, i] + 0.0).tobytes())
            if j is not None and j != i and cand[b, j] and h[b, j] == -h[b, i]:
                eq[b, i] = True  # g x <= h next to -g x <= -h: one equality, multiplier of either sign
                cand[b, i] = cand[b, j] = False
    return keep, eq, cand


def _solve_kkt(P, q, G, h, act, floor_tol):
    """x, multipliers of the rows in ``act`` ([B, r] bool) for the equality-constrained QPs; ``ok`` False where the
    refinement did not converge.  Inactive rows are carried as identity rows (multiplier 0), so every instance has the
    same KKT size."""
    B, nv, _ = P.shape
    r = G.shape[1]
    cols = np.nonzero(act.any(axis=0))[0]  # (rows never active in the batch: left out)
    a = act[:, cols]
    Gc = G[:, cols].astype(LD)
    m = len(cols)
    n = nv + m
    K = np.zeros((B, n, n), LD)
    K[:, :nv, :nv] = P
    Ga = np.where(a[..., None], Gc, LD(0))
    K[:, nv:, :nv] = Ga
    K[:, :nv, nv:] = np.swapaxes(Ga, 1, 2)
    K[:, nv + np.arange(m), nv + np.arange(m)] = np.where(a, LD(0), LD(1))
    rhs = np.zeros((B, n), LD)
    rhs[:, :nv] = -q
    rhs[:, nv:] = np.where(a, np.nan_to_num(h[:, cols]).astype(LD), LD(0))
    K64 = K.astype(float)
    z = np.zeros((B, n), LD)
    ok = np.zeros(B, bool)
    prev = np.full(B, np.inf)
    dn = np.full(B, np.inf)
    with np.errstate(all="ignore"):
        res = rhs.copy()
        for it in range(MAX_REFINE):
            try:
                d = np.linalg.solve(K64, res.astype(float)[..., None])[..., 0]
            except np.linalg.LinAlgError:
                d = np.full((B, n), np.nan)
                for b in range(B):
                    try:
                        d[b] = np.linalg.solve(K64[b], res[b].astype(float))
                    except np.linalg.LinAlgError:
                        pass
            z = z + d.astype(LD)
            xs = np.maximum(1.0, np.abs(z[:, :nv].astype(float)).max(axis=1))
            dn = np.where(np.isfinite(d).all(axis=1), np.abs(d[:, :nv]).max(axis=1), np.inf)
            # converged: the correction is below 1e-15 |x|; or it has stopped shrinking at the noise floor of the longdouble
            # residual (~ cond * 2^-64 |x|), accepted where that floor is below floor_tol
            # (at the last step: whatever it has come to, if that is below floor_tol -- noise need not shrink monotonically)
            ok = (dn <= 1e-15 * xs) | (((dn > 0.5 * prev) | (it == MAX_REFINE - 1)) & (dn <= floor_tol * xs))
            if ok.all():
                break
            prev = dn
            res = rhs - np.einsum("bij,bj->bi", K, z)
    floor = dn / xs
    lam = np.zeros((B, r), LD)
    lam[:, cols] = np.where(a, z[:, nv:], LD(0))
    return z[:, :nv], lam, ok, floor


def batch_minimiser(J, e, cost, gain: Sequence[float], lm: Sequence[float], rows: Sequence[int], damping: float, G, h,
                    guesses: Sequence[np.ndarray], meq: int = 0, diag_extra=None, c_extra=None,
                    fallback: bool = True, floor_tol=1e-9) -> Tuple[np.ndarray, dict]:
    """Minimisers ``[B, nv]`` (fp64) of ``1/2 x'Px + q'x  s.t.  Gx <= h`` (the first ``meq`` rows equalities) for a batch
    with ``J [B, m, nv]``, ``e [B, m]``, ``G [B, r, nv]``, ``h [B, r]`` (rows with ``|h| >= 1e29`` or not finite are missing
    bounds), started from the rows that any of ``guesses`` (``[B, nv]`` points) meets.  ``info``: ``fallback`` (instances
    settled by ``exact_minimiser``), ``exchanges`` (per instance), ``active`` ([B, r] bool), ``residual`` (longdouble
    KKT residual per instance, relative), ``floor`` (size of the last refinement correction relative to ``max(1, |x|)``:
    the reference's own accuracy; NaN where ``exact_minimiser`` settled the instance).  ``floor_tol`` (scalar or per
    instance): the largest such floor accepted -- by default a tenth of the contract's 1e-8; beyond it the instance goes to
    ``exact_minimiser``."""
    J = np.asarray(J, float)
    G = np.ascontiguousarray(np.asarray(G, float))
    h = np.asarray(h, float)
    B, _, nv = J.shape
    r = G.shape[1]
    P, q = objective_ld(J, e, cost, gain, lm, rows, damping, diag_extra, c_extra)
    keep, eq, cand = _row_structure(G, h, meq)
    hl = np.where(keep, h, 0.0).astype(LD)
    Gl = G.astype(LD)
    hscale = 1.0 + np.abs(np.where(keep, h, 0.0))
    act = eq.copy()
    for xg in guesses:
        s = h - np.einsum("brj,bj->br", G, np.asarray(xg, float))
        act |= cand & (np.abs(s) <= 1e-8 * hscale)
    x = np.zeros((B, nv), LD)
    lam = np.zeros((B, r), LD)
    floor = np.zeros(B)
    ftol = np.broadcast_to(np.asarray(floor_tol, float), (B,))
    done = np.zeros(B, bool)
    bad = np.zeros(B, bool)
    exch = np.zeros(B, int)
    todo = np.arange(B)
    for _ in range(MAX_EXCHANGES + 1):
        if not len(todo):
            break
        xt, lt, ok, fl = _solve_kkt(P[todo], q[todo], G[todo], h[todo], act[todo], ftol[todo])
        x[todo], lam[todo], floor[todo] = xt, lt, fl
        slack = hl[todo] - np.einsum("brj,bj->br", Gl[todo], xt)
        gs = np.abs(G[todo]).sum(axis=2)
        tol = CERT_TOL * (hscale[todo] + gs * np.abs(xt.astype(float)).max(axis=1)[:, None])
        lscale = 1.0 + np.abs(q[todo].astype(float)).max(axis=1) + np.abs(P[todo].astype(float)).max(axis=(1, 2)) * np.abs(xt.astype(float)).max(axis=1)
        neg = act[todo] & ~eq[todo] & (lt < -CERT_TOL * lscale[:, None])
        viol = cand[todo] & ~act[todo] & (slack < -tol)
        settled = ok & ~neg.any(axis=1) & ~viol.any(axis=1)
        done[todo[settled]] = True
        bad[todo[~ok]] = True
        go = ok & ~settled
        for i in np.nonzero(go)[0]:
            b = todo[i]
            exch[b] += 1
            if neg[i].any():
                act[b, int(np.argmin(np.where(neg[i], lt[i], LD(0))))] = False
            else:
                enter = int(np.argmin(np.where(viol[i], slack[i] / tol[i], LD(0))))
                # the same normal with another bound cannot be active at once (duplicates are filtered in cand)
                act[b, enter] = True
        todo = todo[go]
    left = np.nonzero(~done)[0]
    if len(left) and fallback:
        from oracle.exact_qp import exact_minimiser

        for b in left:
            xe, _ = exact_minimiser(J[b], e[b], np.broadcast_to(np.asarray(cost, float), J.shape[:2])[b], gain, lm, rows, damping, G[b],
                                    np.where(keep[b], h[b], 1e30), np.asarray(guesses[0], float)[b], meq=meq,
                                    diag_extra=None if diag_extra is None else float(np.broadcast_to(diag_extra, (B,))[b]),
                                    c_extra=None if c_extra is None else np.broadcast_to(c_extra, (B, nv))[b])
            x[b] = xe
    grad = np.einsum("bij,bj->bi", P, x) + q + np.einsum("br,brj->bj", np.where(act, lam, LD(0)), Gl)
    res = (np.abs(grad).max(axis=1).astype(float) / (1.0 + np.abs(q.astype(float)).max(axis=1)))
    res[left] = np.nan
    return x.astype(float), {"fallback": int(len(left)), "fallback_idx": left, "exchanges": exch, "active": act, "residual": res,
                             "refine_failed": int(bad.sum()),
                             "floor": np.where(done, floor, np.nan)}


def conditioning_estimate(H: np.ndarray, free: Optional[np.ndarray] = None) -> np.ndarray:
    """``max_i H_ii (H^-1)_ii`` per instance (the kernel's routing estimate), over the whole ``H`` or over the coordinates
    ``free`` ([B, nv] bool) marks (``H_FF``)."""
    H = np.asarray(H, float)
    if free is None:
        Hi = np.linalg.inv(H)
        return (np.diagonal(H, axis1=1, axis2=2) * np.diagonal(Hi, axis1=1, axis2=2)).max(axis=1)
    out = np.ones(len(H))
    for b in range(len(H)):
        f = np.nonzero(free[b])[0]
        if len(f):
            Hf = H[b][np.ix_(f, f)]
            out[b] = float((np.diag(Hf) * np.diag(np.linalg.inv(Hf))).max())
    return out
