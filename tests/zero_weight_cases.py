"""The batches of tests/test_zero_weight_rows.py and of the generator of its fixture (tests/golden/make_zero_weight_rows.py):
one place, so that the recorded outputs and the test run the same inputs.

The stack + solve kernels do not multiply a task row whose weight is exactly zero in every instance of the wave
(pink_amd/csrc/ik_stack_rows.h: PINKHIP_STACK_SKIP_ZERO_ROWS), provided the row is finite.  A case is

    (shape, Kd, pattern)

  shape    which instantiation and how many instances: nv = 30 and nv = 29 on <30, 0, 32>, its warm twin at nv = 30, and
           nv = 33 with six free leading coordinates on <34, 0, 32> (two front columns are eliminated: the NX = 2 arm of the
           stacking); B = 3 -- the surplus group of the last wave redoes instance 2 -- and B = 4;
  Kd       9 task rows (a chunk of eight and a chunk of one) or 24 (three chunks), one dense task, no Levenberg-Marquardt
           term; a posture task over all coordinates (a diagonal task: its rows are never stored and never skipped) keeps H
           positive definite whatever the pattern takes away;
  pattern  which rows carry weight zero, PATTERNS below.

The stack is Pink's: H = sum_k w_k^2 J_k^T J_k + posture, c = sum_k w_k^2 e_k J_k + posture."""
import numpy as np

from oracle import c_oracle

# name -> (nv, declared free leading coordinates, warm kernel)
KERNELS = {"nv30": (30, 0, False), "nv29": (29, 0, False), "nv30_warm": (30, 0, True), "nv33_lead6": (33, 6, False)}
# what the host plan must answer for them (NV, MD, W): tests/test_zero_weight_rows.py asks it
INSTANTIATION = {"nv30": (30, 0, 32), "nv29": (30, 0, 32), "nv30_warm": (30, 0, 32), "nv33_lead6": (34, 0, 32)}
BATCHES = (3, 4)
KDS = (9, 24)
SHAPES = [f"{k}_B{B}" for k in KERNELS for B in BATCHES]


def _zero_rows(pattern, Kd, B):
    """{instance: rows with weight zero} and the value of the zero (+0.0 or -0.0)"""
    every = lambda rows: {b: list(rows) for b in range(B)}  # noqa: E731
    if pattern == "none":
        return every([]), 0.0
    if pattern == "chunk_first":  # the first row of the first and of the second chunk
        return every([0, 8]), 0.0
    if pattern == "chunk_last":  # the last row of the first chunk and of the last one
        return every([7, Kd - 1]), 0.0
    if pattern == "whole_chunk":  # Kd = 9: the chunk of eight; Kd = 24: the middle one
        return every(range(0, 8) if Kd == 9 else range(8, 16)), 0.0
    if pattern == "all":
        return every(range(Kd)), 0.0
    if pattern == "negative_zero":
        return every([1, 8]), -0.0
    if pattern == "per_instance":
        # instances 0 and 1 share a wave and so do 2 and 3 (or 2 and its own copy at B = 3): row 2 is zero in the odd
        # instances only, row 5 in the even ones only, row 8 in all of them
        return {b: ([2, 8] if b % 2 else [5, 8]) for b in range(B)}, 0.0
    # the non-finite ones: row 3 has weight zero everywhere (and row 8, finite, next to it)
    return every([3, 8]), 0.0


FINITE_PATTERNS = ("none", "chunk_first", "chunk_last", "whole_chunk", "all", "negative_zero", "per_instance")
# a zero-weight row that holds inf / NaN in a column the lanes hold; inf in column 0 (a front column of <34, 0, 32>:
# requested by the lane of the row, handed round with the weights); a zero-weight row whose task error is NaN
NONFINITE_PATTERNS = ("row_inf", "row_nan", "row_inf_col0", "error_nan")
PATTERNS = FINITE_PATTERNS + NONFINITE_PATTERNS
CASES = [(s, Kd, p) for s in SHAPES for Kd in KDS for p in PATTERNS]
_BUILT = {}


def case_id(case):
    return f"{case[0]}_Kd{case[1]}_{case[2]}"


def _terms(shape, Kd):
    """The dense task and the posture task of a shape, all weights non-zero: plain NumPy on a seeded generator."""
    kernel, B = shape.rsplit("_B", 1)
    nv, lead, _ = KERNELS[kernel]
    B = int(B)
    rng = np.random.default_rng(7000 + 100 * nv + 10 * Kd + B)
    J = rng.normal(0, 0.5, size=(B, Kd, nv))
    e = 0.1 * rng.normal(size=(B, Kd))
    w = rng.uniform(0.5, 2.0, size=Kd)
    ep = 0.05 * rng.normal(size=(B, nv))
    lb, ub = np.full((B, nv), -np.inf), np.full((B, nv), np.inf)
    lb[:, lead:] = -rng.uniform(0.002, 0.05, size=(B, nv - lead))
    ub[:, lead:] = rng.uniform(0.002, 0.05, size=(B, nv - lead))
    return nv, lead, B, J, e, w, ep, lb, ub


def _pack(nv, J, e, cost, ep, lb, ub):
    """-> (packed batch, pink-form dict for the C oracle) of one dense task with `cost` ([Kd] or [B, Kd]) + the posture task"""
    from pink_amd.batch import DenseTaskTerm, DiagonalTaskTerm, pack_terms

    B, Kd = e.shape
    tasks = ([DenseTaskTerm(J=J, e=e, cost=cost)] if Kd else []) + [DiagonalTaskTerm(col0=0, e=ep, cost=0.3)]
    batch = pack_terms(nv, tasks, 5e-3, 1e-12, boxes=[(lb, ub)], batch_size=B)
    eye = np.broadcast_to(np.eye(nv), (B, nv, nv))
    wp = np.full(nv, 0.3)
    cost_all = np.concatenate([cost, np.broadcast_to(wp, (B, nv))], axis=1) if np.ndim(cost) == 2 else np.concatenate([cost, wp])
    hb = np.concatenate([ub, -lb], axis=1)
    pf = dict(J=np.ascontiguousarray(np.concatenate([J, eye], axis=1)), e=np.concatenate([e, ep], axis=1), cost=cost_all,
              gain=np.ones(2), lm=np.zeros(2), rows=np.array([0, Kd, Kd + nv], np.int32), damping=1e-12,
              G=np.ascontiguousarray(np.concatenate([eye, -eye], axis=1)), h=np.where(np.isfinite(hb), hb, 1e30))
    return batch, pf


def build(case):
    """-> dict(batch, pink, lead, warm, zero: {instance: rows}) of a case, cached"""
    if case in _BUILT:
        return _BUILT[case]
    shape, Kd, pattern = case
    nv, lead, B, J, e, w, ep, lb, ub = _terms(shape, Kd)
    zero, z = _zero_rows(pattern, Kd, B)
    J, e = J.copy(), e.copy()
    same = all(zero[b] == zero[0] for b in range(B))
    cost = w.copy() if same else np.broadcast_to(w, (B, Kd)).copy()
    for b, rows in zero.items():
        for k in rows:
            if same:
                cost[k] = z
            else:
                cost[b, k] = z
    if pattern == "row_inf":
        J[0, 3, lead + 5] = np.inf
    elif pattern == "row_nan":
        J[1, 3, lead + 2] = np.nan
    elif pattern == "row_inf_col0":
        J[0, 3, 0] = -np.inf
    elif pattern == "error_nan":
        e[0, 3] = np.nan
    batch, pf = _pack(nv, J, e, cost, ep, lb, ub)
    _BUILT[case] = dict(batch=batch, pink=pf, lead=lead, warm=KERNELS[shape.rsplit("_B", 1)[0]][2], zero=zero)
    return _BUILT[case]


def deleted(case):
    """The batches of a finite case with the zero-weight rows taken out (Kd smaller): [(instances, batch, exact)].  One
    batch of all instances where the rows are the same in every instance, one batch per instance where they are not.
    `exact`: the two results must agree bit for bit.  They must wherever a lane's accumulators receive the same non-zero
    terms in the same order -- every accumulator of the stacking except the entries of H and c among the eliminated front
    columns of <34, 0, 32>: those are summed per lane over the rows whose weights the lane holds (row k of a chunk: lane k)
    and over the lanes afterwards, so a deletion that moves a surviving row to another lane reassociates that sum.  There
    `exact` is False unless every surviving row keeps its place in its chunk."""
    key = ("deleted", case)
    if key in _BUILT:
        return _BUILT[key]
    shape, Kd, pattern = case
    assert pattern in FINITE_PATTERNS
    nv, lead, B, J, e, w, ep, lb, ub = _terms(shape, Kd)
    zero, _ = _zero_rows(pattern, Kd, B)
    same = all(zero[b] == zero[0] for b in range(B))
    out = []
    for idx in ([list(range(B))] if same else [[b] for b in range(B)]):
        keep = [k for k in range(Kd) if k not in set(zero[idx[0]])]
        exact = nv <= 32 or all(k % 8 == n % 8 for n, k in enumerate(keep))
        out.append((idx, _pack(nv, J[idx][:, keep], e[idx][:, keep], w[keep], ep[idx], lb[idx], ub[idx])[0], exact))
    _BUILT[key] = out
    return out


def oracle(case):
    key = ("ref", case)
    if key not in _BUILT:
        _BUILT[key] = c_oracle.solve_ik_batch(**build(case)["pink"])
    return _BUILT[key]


def execute(solver, warm_api, case, batch=None):
    """One run -> dict of arrays (dq, status, iters, path): the cold kernel, or the warm twin without a hint."""
    from pink_amd._lib import PackedArgs
    from tests.test_warm_start import warm_solve

    c = build(case)
    batch = c["batch"] if batch is None else batch
    if c["lead"]:
        assert PackedArgs(batch).desc.n_free_lead == c["lead"]
    if not c["warm"]:
        r = solver.solve(batch)
        return dict(dq=r.dq, status=r.status, iters=r.iters, path=r.path)
    o = warm_solve(warm_api, batch)
    assert o.code == 0
    return dict(dq=o.dq, status=o.status, iters=o.iters, path=o.path)
