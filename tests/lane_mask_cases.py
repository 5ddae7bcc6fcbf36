"""The batches of tests/test_lane_masks.py and of the generator of its fixture (tests/golden/make_lane_masks.py): one
place, so that the recorded outputs and the test run the same inputs.

Every batch is B = 7 (odd: the last wave holds a surplus group that redoes the last instance and writes nothing), and
neighbours inside one wavefront are in different control states of the tableau loop:

  instance 1   no finite bound at all: nothing to guess, zero exchanges, straight to its closing trip;
  instance 2   a box that the diagonal guess violates in every bounded coordinate: the start fixes them all, no initial
               sweep runs for its group while its neighbours sweep;
  instance 3   an empty box in one coordinate (lb > ub): "constraints are inconsistent", next to groups that converge;
  instance 5   weakly regularised: its task rows scaled by 1e4 over a posture cost of 0.1, so that max H_ii (H^-1)_ii is
               beyond PINKHIP_SWEEP_ROUTE_COND and the group is routed to the Goldfarb-Idnani code (it starts the loop
               with `refined` set and never runs) next to groups that are certified on the tableau;
  the others   as drawn (tight random boxes, some coordinates free, some one-sided).

One more batch, ``nv30_negdiag``: sixty task rows, no posture term and no damping, which leaves every H positive definite
except instance 4's, whose task rows are zero in coordinate 3: H_33 = 0 exactly, a non-positive diagonal entry (costs enter
squared, so a negative one cannot be stated) -- "not positive definite" before the first sweep, next to groups that run.
Instance 1 has no bounds there either.

Each shape is run with the default iteration cap and once more with ``max_iter = 3`` from the descriptor: instance 1
converges without an exchange while its neighbours run into the cap in the same wave.  The warm twin of <30, 0, 32> runs
without a hint (NULL) and with one (the active set of the cold result, instance 0's bytes replaced by garbage)."""
import numpy as np

from oracle import c_oracle

from tests.cases import random_case

B = 7
SMALL_CAP = 3
# name -> (nv, md, declared free leading coordinates)
SHAPES = {
    "nv30": (30, 0, 0),       # <30, 0, 32>
    "nv29": (29, 0, 0),       # <30, 0, 32>, one pad lane
    "nv32": (32, 0, 0),       # <32, 0, 32>
    "nv16": (16, 0, 0),       # <16, 0, 16>: four groups per wave
    "nv13": (13, 0, 0),       # <16, 0, 16>, odd row pitch
    "nv34_lead6": (34, 0, 6),  # <34, 0, 32>: front coordinates eliminated
    "nv50": (50, 0, 0),       # <50, 0, 64>
    "nv30_md2": (30, 2, 0),   # <30, 2, 32>: dense rows in the tableau
    "nv30_md6": (30, 6, 0),   # <30, 6, 32>: virtual dense rows (ik_sweepx.h)
    "nv30_negdiag": (30, 0, 0),  # <30, 0, 32>, one instance with a non-positive diagonal entry
}
ROUTED_SCALE = 1e4
_BUILT = {}


def build(name):
    """(packed batch, pink-form dict for the oracle, declared lead) of one shape."""
    if name in _BUILT:
        return _BUILT[name]
    nv, md, lead = SHAPES[name]
    if name == "nv30_negdiag":
        _BUILT[name] = _negdiag(nv)
        return _BUILT[name]
    batch, pf = random_case(nv, B, 100 + nv + md, md=md, root=lead)
    lb, ub = batch.lb, batch.ub
    lb[1], ub[1] = -np.inf, np.inf
    Kd = batch.J.shape[1]
    batch.J[5] *= ROUTED_SCALE
    pf["J"][5, :Kd] *= ROUTED_SCALE
    Hc = c_oracle.solve_ik_batch(**dict(pf, G=None, h=None), want_Hc=True, solve=False)
    xd = -Hc["c"][2] / np.diagonal(Hc["H"][2])
    idx = np.arange(lead, nv)
    below = idx % 2 == 0
    ub[2, idx] = np.where(below, xd[idx] - 0.01, xd[idx] + 0.06)
    lb[2, idx] = np.where(below, xd[idx] - 0.06, xd[idx] + 0.01)
    k = lead + 3
    lb[3, k], ub[3, k] = 0.02, -0.02  # empty
    hb = np.concatenate([ub, -lb], axis=1)
    pf["h"][:, :2 * nv] = np.where(np.isfinite(hb), hb, 1e30)
    _BUILT[name] = (batch, pf, lead)
    return _BUILT[name]


def _negdiag(nv):
    from pink_amd.batch import DenseTaskTerm, pack_terms

    rng = np.random.default_rng(977)
    K = 60
    J = rng.normal(0, 0.5, size=(B, K, nv))
    J[4, :, 3] = 0.0
    e = 0.1 * rng.normal(size=(B, K))
    lb, ub = -0.02 * np.ones((B, nv)), 0.03 * np.ones((B, nv))
    lb[1], ub[1] = -np.inf, np.inf
    batch = pack_terms(nv, [DenseTaskTerm(J=J, e=e, cost=1.0)], 5e-3, 0.0, boxes=[(lb, ub)], batch_size=B)
    eye = np.broadcast_to(np.eye(nv), (B, nv, nv))
    hb = np.concatenate([ub, -lb], axis=1)
    pf = dict(J=np.ascontiguousarray(J), e=e, cost=np.ones(K), gain=np.array([1.0]), lm=np.array([0.0]), rows=np.array([0, K], np.int32), damping=0.0,
              G=np.ascontiguousarray(np.concatenate([eye, -eye], axis=1)), h=np.where(np.isfinite(hb), hb, 1e30))
    return batch, pf, 0


def oracle(name):
    key = ("ref", name)
    if key not in _BUILT:
        _BUILT[key] = c_oracle.solve_ik_batch(**build(name)[1])
    return _BUILT[key]


def runs():
    """(run name, shape, max_iter, warm mode) of everything that is recorded: warm mode None = the cold kernel."""
    out = []
    for name in SHAPES:
        out.append((name, name, 0, None))
        out.append((f"{name}_cap{SMALL_CAP}", name, SMALL_CAP, None))
    out.append(("nv30_warm_nohint", "nv30", 0, "nohint"))
    out.append(("nv30_warm_hint", "nv30", 0, "hint"))
    out.append((f"nv30_warm_hint_cap{SMALL_CAP}", "nv30", SMALL_CAP, "hint"))
    return out


def execute(solver, warm_api, shape, max_iter, warm):
    """One run -> dict of arrays (dq, status, iters, path, and active for the warm kernels)."""
    from pink_amd._lib import PackedArgs
    from tests.test_warm_start import warm_solve

    batch, _, lead = build(shape)
    if lead:
        assert PackedArgs(batch).desc.n_free_lead == lead
    if warm is None:
        r = solver.solve(batch, max_iter=max_iter)
        return dict(dq=r.dq, status=r.status, iters=r.iters, path=r.path)
    hint = None
    if warm == "hint":
        cold = warm_solve(warm_api, batch)
        hint = cold.active.copy()
        hint[0] = (np.arange(batch.nv) * 37 + 5) % 256  # garbage bytes: never trusted
    o = warm_solve(warm_api, batch, active_in=hint, max_iter=max_iter)
    assert o.code == 0
    return dict(dq=o.dq, status=o.status, iters=o.iters, path=o.path, active=o.active)
