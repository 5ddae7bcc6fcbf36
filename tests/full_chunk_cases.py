"""The batches of tests/test_full_chunk_requests.py and of the generator of its fixture
(tests/golden/make_full_chunk_requests.py): one place, so that the recorded outputs and the test run the same inputs.

The stack + solve kernels request a FULL chunk of eight task rows -- Kd - r0 >= 8 -- from one scalar row pointer inside one
region of the coordinate lanes, and a partial chunk row by row (pink_amd/csrc/ik_stack_rows.h: PINKHIP_STACK_FULL_CHUNKS).
The same loads from the same addresses: no bit of any result may change.  A case is

    (shape, Kd, pattern)

  shape    which instantiation and how many instances, KERNELS below: <30, 0, 32> at nv = 30 and at nv = 26 (the lanes
           li >= nv must read 0.0), its warm twin, <34, 0, 32> at nv = 33 and 34 (two front columns are eliminated: their
           requests, and 31 resp. all 32 coordinate lanes), <40, 0, 64> (two chunks requested ahead).  B = 1, 3, 5 on <30, 0, 32> -- with an odd B the surplus
           group of the last wave redoes the last instance and writes nothing -- and B = 3 on the others;
  Kd       3 (a partial chunk only), 8 (exactly one full chunk), 9 (full + one row), 16, 17, 24 (the headline's three);
  pattern  "vector": the weights are one vector for all instances; "batched": per instance (cost_batched);
           "zero_row": vector weights with a zero-weight row inside a full chunk (where PINKHIP_STACK_SKIP_ZERO_ROWS and the
           full-chunk requests meet); "zero_row_nan": ... and a NaN in that row, which must still make its NaN.

The stack is that of tests/zero_weight_cases.py: one dense task, a posture task over all coordinates, no
Levenberg-Marquardt term."""
import numpy as np

from tests.zero_weight_cases import _pack

# name -> (nv, declared free leading coordinates, warm kernel)
KERNELS = {"nv30": (30, 0, False), "nv26": (26, 0, False), "nv30_warm": (30, 0, True), "nv33_lead6": (33, 6, False),
           "nv34_lead6": (34, 6, False), "nv40": (40, 0, False)}
# what the host plan must answer for them (NV, MD, W): tests/test_full_chunk_requests.py asks it
INSTANTIATION = {"nv30": (30, 0, 32), "nv26": (30, 0, 32), "nv30_warm": (30, 0, 32), "nv33_lead6": (34, 0, 32),
                 "nv34_lead6": (34, 0, 32), "nv40": (40, 0, 64)}
KDS = (3, 8, 9, 16, 17, 24)
SHAPES = [f"nv30_B{B}" for B in (1, 3, 5)] + [f"{k}_B3" for k in KERNELS if k != "nv30"]
ZERO_ROW = 10  # (of Kd = 24: the third row of the second chunk)
SPECIAL = [(s, 24, p) for s in ("nv30_B3", "nv33_lead6_B3") for p in ("zero_row", "zero_row_nan")]
CASES = [(s, Kd, p) for s in SHAPES for Kd in KDS for p in ("vector", "batched")] + SPECIAL
_BUILT = {}


def case_id(case):
    return f"{case[0]}_Kd{case[1]}_{case[2]}"


def build(case):
    """-> dict(batch, lead, warm) of a case, cached: plain NumPy on a seeded generator"""
    if case in _BUILT:
        return _BUILT[case]
    shape, Kd, pattern = case
    kernel, B = shape.rsplit("_B", 1)
    nv, lead, warm = KERNELS[kernel]
    B = int(B)
    rng = np.random.default_rng(9000 + 100 * nv + 10 * Kd + B)
    J = rng.normal(0, 0.5, size=(B, Kd, nv))
    e = 0.1 * rng.normal(size=(B, Kd))
    ep = 0.05 * rng.normal(size=(B, nv))
    lb, ub = np.full((B, nv), -np.inf), np.full((B, nv), np.inf)
    lb[:, lead:] = -rng.uniform(0.002, 0.05, size=(B, nv - lead))
    ub[:, lead:] = rng.uniform(0.002, 0.05, size=(B, nv - lead))
    cost = rng.uniform(0.5, 2.0, size=(B, Kd) if pattern == "batched" else Kd)
    if pattern in ("zero_row", "zero_row_nan"):
        cost[ZERO_ROW] = 0.0
    if pattern == "zero_row_nan":
        J[B - 1, ZERO_ROW, lead + 2] = np.nan
    batch, _ = _pack(nv, J, e, cost, ep, lb, ub)
    _BUILT[case] = dict(batch=batch, lead=lead, warm=warm)
    return _BUILT[case]


def execute(solver, warm_api, case):
    """One run -> dict of arrays (dq, status, iters, path): the cold kernel, or the warm twin without a hint."""
    from pink_amd._lib import PackedArgs
    from tests.test_warm_start import warm_solve

    c = build(case)
    if c["lead"]:
        assert PackedArgs(c["batch"]).desc.n_free_lead == c["lead"]
    if not c["warm"]:
        r = solver.solve(c["batch"])
        return dict(dq=r.dq, status=r.status, iters=r.iters, path=r.path)
    o = warm_solve(warm_api, c["batch"])
    assert o.code == 0
    return dict(dq=o.dq, status=o.status, iters=o.iters, path=o.path)
