"""The batches of tests/test_trip_paths.py and of the generator of its fixture (tests/golden/make_trip_paths.py): one place,
so that the recorded outputs and the test run the same inputs.

The box-only tableau loop runs its ordinary trips `while some group of the wave exchanges` and its closing trips in a loop
of their own behind them (pink_amd/csrc/ik_sweep.h: PINKHIP_SWEEP_SPLIT_CLOSING).  Every instantiation whose loop that changes is run at the smallest batch that leaves surplus groups in the last wave (they redo the last instance and write nothing), with neighbours that
leave the first loop at different trips and for different reasons:

  role "none"       no finite bound at all: nothing to exchange, the group waits from the first trip on;
  role "many"       one vector added to every task column: H is far from its diagonal, the diagonal guess is wrong in many
                    coordinates and the group keeps the wave in the first loop after its neighbours have left it (exchanges
                    on the emulator: 6 at nv16, 12 at nv30, 9 at nv34_lead6, 24 and 22 at nv50);
  role "routed"     two task columns that agree to 3e-5: max H_ii (H^-1)_ii is beyond PINKHIP_SWEEP_ROUTE_COND, the group is
                    routed to the Goldfarb-Idnani code and starts the loops with `refined` set.  The box of the two contains
                    the diagonal guess (both start free: the estimate sees the pair), and the instance's task errors and box
                    are a hundredth of the others', so that cond(H) eps |dq| stays below the suite's tolerance;
  role "wrongsign"  an INDEFINITE H: a second task of one row, J = 0 and e = 1 in this instance alone (0 in the others), with
                    a negative Levenberg-Marquardt factor shifts this instance's diagonal down by the eigenvalue a third of
                    the way up the spectrum of J^T J -- every diagonal entry stays positive.  Seed found on the emulator
                    (make_trip_paths.py --search): H is positive definite on the free set the diagonal guess leaves, and
                    an exchange inside the loop meets a pivot of the wrong sign (the first one at nv16, nv30 and nv50_b, the
                    second at nv34_lead6: what the search's debug emulator reports; the ordinary one cannot tell it from a
                    non-positive pivot of the initial sweeps, which is why the search insists on it) -- the verdict inside
                    the loop ("not positive definite on this set"), which ends the group's exchanges and hands it to the
                    Goldfarb-Idnani code, whose Cholesky factorisation says the same as the oracle's;
  the others        as drawn.

Sixty task rows, no posture term and no damping (H = J^T W J, positive definite except where a role says otherwise).  Every
run is repeated with ``max_iter = 3`` from the descriptor: the "none" instance converges while its neighbours run into the
cap in the same wave.  The uncapped runs are made once more on an emulator built with PINKHIP_SWEEP_PPM_MURTY_AFTER(nv) = 2:
every group that exchanges more than twice goes on with Murty's least-index rule.  The warm twins of <16, 0, 16> and
<30, 0, 32> run with a hint (the active set of their own cold call, instance 0's bytes replaced by garbage)."""
import numpy as np

from oracle import c_oracle

SMALL_CAP = 3
K_ROWS = 60
# name -> (nv, declared free leading coordinates, B, roles by instance, seed)
SHAPES = {
    "nv16": (16, 0, 9, {0: "many", 1: "none", 2: "wrongsign", 3: "routed"}, 29),        # <16, 0, 16>: four groups, column by indicator product
    "nv30": (30, 0, 5, {0: "many", 1: "none", 2: "wrongsign", 3: "routed"}, 0),       # <30, 0, 32>: the headline instantiation
    "nv34_lead6": (34, 6, 5, {0: "many", 1: "none", 2: "wrongsign", 3: "routed"}, 335),  # <34, 0, 32>: front elimination
    "nv50_a": (50, 0, 3, {0: "many", 1: "none", 2: "routed"}, 0),                      # <50, 0, 64>: one group per wave
    "nv50_b": (50, 0, 3, {0: "wrongsign", 1: "none", 2: "many"}, 54),
}
WARM_SHAPES = ("nv16", "nv30")
_BUILT = {}


def make(name, seed=None):
    """(packed batch, pink-form dict for the oracle, declared lead, roles) of one shape, not cached."""
    from pink_amd.batch import DenseTaskTerm, pack_terms

    nv, lead, B, roles, seed0 = SHAPES[name]
    rng = np.random.default_rng(4000 + nv + 1000 * (seed0 if seed is None else seed))
    J = rng.normal(0, 0.5, size=(B, K_ROWS, nv))
    e = 0.1 * rng.normal(size=(B, K_ROWS))
    lb, ub = np.full((B, nv), -np.inf), np.full((B, nv), np.inf)
    lb[:, lead:] = -rng.uniform(0.002, 0.05, size=(B, nv - lead))
    ub[:, lead:] = rng.uniform(0.002, 0.05, size=(B, nv - lead))
    common = rng.normal(size=K_ROWS)
    e2, shift = np.zeros((B, 1)), 0.0
    i, j = lead + 1, lead + 4
    for b, role in roles.items():
        if role == "none":
            lb[b], ub[b] = -np.inf, np.inf
        elif role == "many":
            J[b] += 2.0 * common[:, None]
        elif role == "routed":
            J[b, :, j] = J[b, :, i] + 3e-5 * rng.normal(size=K_ROWS)
            e[b] *= 0.01
            lb[b] *= 0.01
            ub[b] *= 0.01
        elif role == "wrongsign":
            e2[b] = 1.0
            shift = float(np.linalg.eigvalsh(J[b].T @ J[b])[nv // 3])
    J2 = np.zeros((B, 1, nv))
    pf = dict(J=np.ascontiguousarray(np.concatenate([J, J2], axis=1)), e=np.concatenate([e, e2], axis=1), cost=np.ones(K_ROWS + 1), gain=np.array([1.0, 1.0]),
              lm=np.array([0.0, -shift]), rows=np.array([0, K_ROWS, K_ROWS + 1], np.int32), damping=0.0)
    Hc = c_oracle.solve_ik_batch(**dict(pf, G=None, h=None), want_Hc=True, solve=False)
    for b, role in roles.items():
        if role == "routed":
            xd = -Hc["c"][b, [i, j]] / Hc["H"][b, [i, j], [i, j]]  # the diagonal guess of the two coordinates
            lb[b, [i, j]], ub[b, [i, j]] = xd - 3e-4, xd + 3e-4  # (inside: both start free, the estimate sees the pair)
    tasks = [DenseTaskTerm(J=J, e=e, cost=1.0), DenseTaskTerm(J=J2, e=e2, cost=1.0, lm_damping=-shift)]
    batch = pack_terms(nv, tasks, 5e-3, 0.0, boxes=[(lb, ub)], batch_size=B)
    eye = np.broadcast_to(np.eye(nv), (B, nv, nv))
    hb = np.concatenate([ub, -lb], axis=1)
    pf.update(G=np.ascontiguousarray(np.concatenate([eye, -eye], axis=1)), h=np.where(np.isfinite(hb), hb, 1e30))
    return batch, pf, lead, roles


def build(name):
    if name not in _BUILT:
        _BUILT[name] = make(name)
    return _BUILT[name]


def oracle(name):
    key = ("ref", name)
    if key not in _BUILT:
        _BUILT[key] = c_oracle.solve_ik_batch(**build(name)[1])
    return _BUILT[key]


def runs():
    """(run name, shape, max_iter, warm) of everything that is recorded: warm False = the cold kernel."""
    out = []
    for name in SHAPES:
        out.append((name, name, 0, False))
        out.append((f"{name}_cap{SMALL_CAP}", name, SMALL_CAP, False))
    for name in WARM_SHAPES:
        out.append((f"{name}_warm", name, 0, True))
        out.append((f"{name}_warm_cap{SMALL_CAP}", name, SMALL_CAP, True))
    return out


def runs_murty():
    """... of what is recorded once more from an emulator whose principal pivoting switches to Murty's least-index rule after
    two trips (__graft_entry__.EMU_VARIANTS["murty"]): the uncapped runs."""
    return [r for r in runs() if r[2] == 0]


def execute(solver, warm_api, shape, max_iter, warm, built=None):
    """One run -> dict of arrays (dq, status, iters, path, and active for the warm kernels)."""
    from pink_amd._lib import PackedArgs
    from tests.test_warm_start import warm_solve

    batch, _, lead, _ = built or build(shape)
    if lead:
        assert PackedArgs(batch).desc.n_free_lead == lead
    if not warm:
        r = solver.solve(batch, max_iter=max_iter)
        return dict(dq=r.dq, status=r.status, iters=r.iters, path=r.path)
    cold = warm_solve(warm_api, batch)
    hint = cold.active.copy()
    hint[0] = (np.arange(batch.nv) * 37 + 5) % 256  # garbage bytes: never trusted
    o = warm_solve(warm_api, batch, active_in=hint, max_iter=max_iter)
    assert o.code == 0
    return dict(dq=o.dq, status=o.status, iters=o.iters, path=o.path, active=o.active)
