"""No instance's result may depend on who shares its wavefront: solo against company, bit for bit.

Every solver family packs 64 / W problems into one wavefront (W = 8, 16, 32: 8, 4 or 2 per wave) and is full of control
flow that looks across those groups: wave_any(...) branches, masked trips of groups that finished early, the hand-over of a
whole wave to the Goldfarb-Idnani code when one group fails its certificate, the sequential hand-over at nv = 33 / 34.  A
leak across a group border changes a neighbour's answer only when the neighbour is extreme, so benign batches do not show
it.  Here each case is a list of *probes* (one per way through the family's code) and of *company* (instances that are
infeasible, NaN, Inf, singular, routed, handed over, out of iterations, ...) for one kernel instantiation -- the smallest
of its table in dispatch.h with more than one group per wave:

1. every probe and every company instance is solved alone, B = 1;
2. a fixed table of arrangements of them is solved, one launch per arrangement;
3. every instance of every arrangement is compared with its solo result, with no tolerance anywhere:
   probe    the bits of dq, status, path, iters, and active_out where the family writes it (whole-step: after each of two
            integrated steps the bits of q, and first_failure);
   company  status and path equal solo, the bits of dq where the solo status is 0.
   (In a launch whose max_iter is too small to finish, an instance that runs out of iterations is company.)

The arrangement table is checked before anything is launched: every probe sits in every slot of a wave (index mod 64 / W),
shares a wave with every kind of company, sits last in a tail group (B mod 64 / W != 0) and appears in the second wave of a
launch; B <= 3 (64 / W) + 1.  The path of every probe and the status of the company that has a stated one are asserted, so
that a case keeps testing what it says it does.

Anchors -- equal bits must not pass by being equally wrong: the solo result of every stack + solve probe is held to the
50-digit minimiser of oracle/exact_qp.py at the bar tests/test_conditioning_bands.py claims for its conditioning
(parity_suite.banded_bar), the solo velocity of every whole-step probe to c_oracle.gi_solve on build_ik's QP at 1e-8, as
tests/test_kernel_table_launch.py does.  No new tolerance.

Emulator under -m "not gpu", the MI355X under -m gpu."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import c_oracle
from pink_amd._lib import PackedArgs
from pink_amd.batch import DenseTaskTerm, DiagonalTaskTerm, IKBatch, pack_terms

from tests import parity_suite as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLEAU, HANDOVER, ROUTED, GI = 0, 1, 2, 3  # include/pinkhip.h PINKHIP_PATH_*
PATH_NAMES = ["tableau", "handover", "routed", "gi"]
PLAN_SWEEP, PLAN_SWEEPX, PLAN_PACKED = 3, 4, 5  # host_plan.h PlanKind
RECORD = {}  # (case, backend) -> what profiles/wave_isolation.json holds of it


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    from tests.test_warm_start import EmuWarm

    if request.param == "emu":
        return "emu", EmuWarm(request.getfixturevalue("emu"))
    return "gpu", request.getfixturevalue("gpu_solver")


# ------------------------------------------------------------------------------------------------------ arrangements


def arrangements(n_probes, n_company, per):
    """Launches (lists of instance ids: probes 0 .. n_probes - 1, then the company) that meet the coverage conditions of
    the module docstring for ``per`` groups per wave.  Waves are made greedily -- the probes with the most slots and company
    kinds still to meet, on slots they have not sat on, next to company they have not met -- then dealt to launches of two
    or three full waves and a tail group that holds one probe alone."""
    P, C = n_probes, n_company
    n_pw = max(1, min(P, per // 2))  # probes per wave; the rest is company
    need_slot = {(p, s) for p in range(P) for s in range(per)}
    need_comp = {(p, c) for p in range(P) for c in range(C)}
    waves = []
    while need_slot or need_comp:
        score = [sum(1 for k in need_slot if k[0] == p) + sum(1 for k in need_comp if k[0] == p) for p in range(P)]
        chosen = sorted(range(P), key=lambda p: (-score[p], p))[:n_pw]
        wave = [None] * per
        for p in chosen:
            free = [s for s in range(per) if wave[s] is None]
            want = [s for s in free if (p, s) in need_slot]
            wave[(want or free)[0]] = p
        for s in range(per):
            if wave[s] is None:
                here = [w - P for w in wave if w is not None and w >= P]
                gain = [(-sum(1 for p in chosen if (p, c) in need_comp), c in here, c) for c in range(C)]
                wave[s] = P + min(gain)[2]
        for s, w in enumerate(wave):
            if w < P:
                need_slot.discard((w, s))
                need_comp.difference_update({(w, c - P) for c in wave if c >= P})
        waves.append(wave)
    n_launch = max(P, -(-len(waves) // 3))
    while len(waves) < 2 * n_launch:  # (every launch has a second wave)
        waves.append(waves[len(waves) % max(1, len(waves) - 1)])
    launches = [waves[i::n_launch] for i in range(n_launch)]
    # every probe once in the second wave: rotate each launch so that a wave with a probe still missing there comes second
    missing = set(range(P))
    for L in launches:
        best = max(range(len(L)), key=lambda i: len(missing & set(L[i])))
        L[1], L[best] = L[best], L[1]
        missing -= set(L[1])
    return [[i for wave in L for i in wave] + [n % P] for n, L in enumerate(launches)]


def check_coverage(launches, n_probes, kinds, per):
    """The conditions of the issue on an arrangement table; ``kinds[i]``: the company kind of instance i (None: a probe)."""
    company = sorted({k for k in kinds if k is not None})
    assert len(launches) <= 13, len(launches)
    for p in range(n_probes):
        slots, met, tail, second = set(), set(), False, False
        for L in launches:
            assert len(L) <= 3 * per + 1
            for pos, i in enumerate(L):
                if i != p:
                    continue
                wave = L[pos - pos % per:pos - pos % per + per]
                slots.add(pos % per)
                met |= {kinds[j] for j in wave if kinds[j] is not None}
                tail |= pos == len(L) - 1 and len(L) % per != 0
                second |= pos // per == 1
        assert slots == set(range(per)), ("a probe misses a slot", p, slots)
        assert met == set(company), ("a probe never shares a wave with", p, set(company) - met)
        assert tail, ("a probe is never last in a tail group", p)
        assert second, ("a probe is never in the second wave", p)


@pytest.mark.parametrize("per", [2, 4, 8])
@pytest.mark.parametrize("n_company", [5, 7, 9])
def test_arrangement_tables_meet_the_coverage_conditions(per, n_company):
    launches = arrangements(4, n_company, per)
    check_coverage(launches, 4, [None] * 4 + [f"c{c}" for c in range(n_company)], per)


# --------------------------------------------------------------------------------------------- stack + solve families

# name -> nv, dense rows, unbounded front coordinates, PINKHIP_SOLVER, warm-start entry, lanes per problem, the plan {kind,
#         NV, MD, W, dense} the library must choose (the warm twins have no plan query: their active_out is what shows them)
SOLVE_CASES = {
    "packed-6-0-8": dict(nv=6, md=0, env="packed", W=8, plan=(PLAN_PACKED, 6, 0, 8, 0)),
    "packed-6-1-8": dict(nv=6, md=1, env="packed", W=8, plan=(PLAN_PACKED, 6, 0, 8, 1)),
    "sweep-8-0-16": dict(nv=8, md=0, W=16, plan=(PLAN_SWEEP, 8, 0, 16, 0)),
    "sweep-12-4-16": dict(nv=12, md=4, W=16, plan=(PLAN_SWEEP, 12, 4, 16, 0)),
    "sweepx-16-8-16": dict(nv=16, md=8, W=16, plan=(PLAN_SWEEPX, 16, 8, 16, 0)),
    "sweep-24-0-32": dict(nv=24, md=0, W=32, plan=(PLAN_SWEEP, 24, 0, 32, 0)),
    "sweepx-30-6-32": dict(nv=30, md=6, W=32, plan=(PLAN_SWEEPX, 30, 6, 32, 0)),
    "sweep-34-0-32": dict(nv=33, md=0, lead=3, W=32, plan=(PLAN_SWEEP, 34, 0, 32, 0)),
    "wsweep-16-0-16": dict(nv=16, md=0, W=16, warm=True),
    "wsweep-30-0-32": dict(nv=30, md=0, W=32, warm=True),
}
PROBES = ["interior", "exchanges", "routed", "handover"]  # (forced Goldfarb-Idnani kernel: interior, tight, routed, weak)
N_CANDIDATES = 80
SHORT_MAX_ITER = 3  # the launch whose max_iter is too small for the probe with many exchanges


def solve_instances(case):
    """(batch of all instances of the case, their names, the company kind of each or None, active_in bytes or None).  One
    draw per instance of two dense tasks of three rows, a posture task, a box and ``md`` dense rows; costs are per
    instance, so that one batch can hold an instance without any task (J = 0, damping alone).
      interior   a box of +-5 and rows far away: the minimiser is inside, no exchange
      exchanges  / handover: weakly regularised draws (``weak_candidate``), chosen by the test among a fixed seeded list
                 as the first that stays on the tableau through many exchanges / that fails its certificate and is handed
                 over with status 0, on the backend under test
      routed     J scaled by 3e3 (conditioning ~1e9 .. 1e10, the top band of tests/test_conditioning_bands.py): the tableau sends it to the Goldfarb-Idnani code by its conditioning estimate
    Forced Goldfarb-Idnani kernel: every probe is on that path, so they vary the step count instead -- interior, tight
    (bounds of 2e-3 .. 1e-2), routed, weak (posture cost 3e-4, a third of the coordinates unbounded)."""
    c = SOLVE_CASES[case]
    nv, md, lead, warm = c["nv"], c["md"], c.get("lead", 0), c.get("warm", False)
    company = ["empty_box", "nan_J", "inf_e", "zero_J", "tiny_box"] + (["inconsistent_rows"] if md else []) + (["active_255"] if warm else [])
    names = PROBES + company
    n = len(names)
    rng = np.random.default_rng(1000 * nv + 10 * md + len(case))
    J = rng.normal(0, 0.5, size=(n, 6, nv))
    e = 0.1 * rng.normal(size=(n, 6))
    cost = rng.uniform(0.2, 3.0, size=(n, 6))
    ep = rng.uniform(-0.5, 0.5, size=(n, nv - lead))
    dcost = np.full((n, nv - lead), 0.1)
    lb, ub = np.full((n, nv), -np.inf), np.full((n, nv), np.inf)
    lb[:, lead:], ub[:, lead:] = -rng.uniform(0.002, 0.05, size=(n, nv - lead)), rng.uniform(0.002, 0.05, size=(n, nv - lead))
    G, h = rng.normal(size=(n, md, nv)), rng.uniform(0.0, 0.05, size=(n, md))
    active = rng.integers(0, 3, size=(n, nv)).astype(np.uint8) if warm else None
    for i, name in enumerate(names):
        if name == "interior":
            lb[i, lead:], ub[i, lead:], h[i] = -5.0, 5.0, 50.0
            if warm:
                active[i] = 0
        elif name == "exchanges" and c.get("env") == "packed":  # ("tight")
            lb[i, lead:], ub[i, lead:] = -rng.uniform(0.002, 0.01, size=nv - lead), rng.uniform(0.002, 0.01, size=nv - lead)
        elif name == "routed":
            J[i] *= 3e3
            if warm:
                active[i] = 0  # (the estimate is taken on the all-free start; from other bytes the same instance is handed over)
        elif name == "handover" and c.get("env") == "packed":  # ("weak")
            dcost[i] = 3e-4
            free = lead + np.nonzero(rng.random(nv - lead) < 0.33)[0]
            lb[i, free], ub[i, free] = -np.inf, np.inf
        elif name == "empty_box":
            lb[i, lead + 2], ub[i, lead + 2] = 1.0, -1.0
        elif name == "nan_J":
            J[i, 1, lead + 1] = np.nan
        elif name == "inf_e":
            e[i, 2] = np.inf
        elif name == "zero_J":
            J[i], cost[i], dcost[i] = 0.0, 0.0, 0.0
        elif name == "tiny_box":
            lb[i, lead:], ub[i, lead:] = -1e-6, 1e-6
        elif name == "inconsistent_rows":  # x_k <= -1 against a box of a few hundredths (and against x_k >= 1 where two rows fit)
            G[i, 0], h[i, 0] = 0.0, -1.0
            G[i, 0, lead + 1] = 1.0
            if md > 1:
                G[i, 1], h[i, 1] = -G[i, 0], -1.0
        elif name == "active_255":
            active[i] = 255
    tasks = [DenseTaskTerm(J=J[:, :3], e=e[:, :3], cost=cost[:, :3], gain=0.7), DenseTaskTerm(J=J[:, 3:], e=e[:, 3:], cost=cost[:, 3:], gain=1.0),
             DiagonalTaskTerm(col0=lead, e=ep, cost=dcost, gain=1.0)]
    batch = pack_terms(nv, tasks, 0.005, 1e-12, boxes=[(lb, ub)], dense_rows=[(G, h)] if md else (), batch_size=n)
    kinds = [None] * len(PROBES) + company
    return batch, names, kinds, active


def weak_candidate(batch, i, seed, lead):
    """Instance i of the batch redrawn as candidate ``seed`` of the weakly regularised probes: a posture cost of 3e-6 .. 1e-3,
    bounds of 2e-3 .. 5e-2, 10 % .. 70 % of the coordinates unbounded."""
    rng = np.random.default_rng(seed)
    nv = batch.nv
    batch.cost[i, 6:] = 10 ** rng.uniform(-5.5, -3)
    batch.lb[i, lead:], batch.ub[i, lead:] = -rng.uniform(0.002, 0.05, size=nv - lead), rng.uniform(0.002, 0.05, size=nv - lead)
    free = lead + np.nonzero(rng.random(nv - lead) < rng.uniform(0.1, 0.7))[0]
    batch.lb[i, free], batch.ub[i, free] = -np.inf, np.inf


def take(batch, idx):
    """The instances ``idx`` of a batch (with repeats, in that order)."""
    idx = np.asarray(idx)
    b = batch
    return IKBatch(b.nv, b.J[idx], b.e[idx], b.cost[idx], b.task_rows, b.task_kind, b.task_col0, b.gain, b.lm_damping, b.lb[idx], b.ub[idx],
                   b.Gd[idx], b.hd[idx], b.barrier_rows, b.barrier_safe_gain, None, b.damping, b.dt, b.n_eq, {})


def launch(where, api, batch, active, max_iter, warm):
    """One call: (dq, status, path, iters, active_out or None)"""
    if not warm:
        out = api.solve(batch, max_iter=max_iter)
        return out.dq, out.status, np.asarray(out.path), out.iters, None
    if where == "gpu":
        out = api.solve(batch, max_iter=max_iter, active_in=np.ascontiguousarray(active), return_active=True)
        return out.dq, out.status, np.asarray(out.path), out.iters, out.active
    from tests.test_warm_start import warm_solve

    o = warm_solve(api, batch, active_in=active, max_iter=max_iter)
    assert o.code == 0, o.code
    return o.dq, o.status, o.path, o.iters, o.active


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare_solve(solo, got, i, is_probe):
    """The fields of instance i's result ``got`` that differ from its solo result (empty: none)"""
    bad = [f for k, f in ((1, "status"), (2, "path")) if int(got[k]) != int(solo[k][0])]
    strict = is_probe and int(solo[1][0]) != 1  # (out of iterations: company, whoever it is)
    if (strict or int(solo[1][0]) == 0) and not np.array_equal(bits(got[0]), bits(solo[0][0])):
        bad.append("dq")
    if strict and int(got[3]) != int(solo[3][0]):
        bad.append("iters")
    if strict and solo[4] is not None and not np.array_equal(got[4], solo[4][0]):
        bad.append("active_out")
    return bad


_ANCHORED = set()


def anchor_solve_probe(case, name, one, dq, status):
    """The solo result of a probe against the 50-digit minimiser, at the bar of the conditioning bands (once per case)."""
    from oracle.exact_qp import exact_minimiser
    from oracle.refined_kkt import conditioning_estimate

    if (case, name) in _ANCHORED:
        return
    pf = ps.ikbatch_form(one)
    ref = c_oracle.solve_ik_batch(**pf, want_Hc=True)
    assert status == 0 and ref["status"][0] == 0, (case, name, status, ref["status"])
    kappa = float(conditioning_estimate(ref["H"])[0])
    xe, _ = exact_minimiser(pf["J"][0], pf["e"][0], pf["cost"][0], pf["gain"], pf["lm"], pf["rows"], pf["damping"], pf["G"][0], pf["h"][0],
                            ref["dq"][0], meq=pf["meq"])
    xmax, err, err_oracle = float(np.abs(xe).max()), float(np.abs(dq - xe).max()), float(np.abs(ref["dq"][0] - xe).max())
    bar = float(ps.banded_bar(kappa, xmax, err_oracle))
    print(f"{case} {name}: kappa {kappa:.2e} |dq - x*| = {err:.2e} (oracle {err_oracle:.2e}, bar {bar:.2e})")
    assert err <= bar, (case, name, kappa, err, err_oracle, bar)
    _ANCHORED.add((case, name))


@pytest.mark.parametrize("case", list(SOLVE_CASES))
def test_stack_and_solve_families(backend, case, monkeypatch):
    where, api = backend
    c = SOLVE_CASES[case]
    warm, per = c.get("warm", False), 64 // c["W"]
    if c.get("env"):
        monkeypatch.setenv("PINKHIP_SOLVER", c["env"])
    else:
        monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
    batch, names, kinds, active = solve_instances(case)
    n, P = len(names), len(PROBES)
    launches = arrangements(P, n - P, per)
    check_coverage(launches, P, kinds, per)
    if "plan" in c:  # the instantiation the case is about, by the plan the library itself runs
        planned = (ctypes.c_int * 6)()
        lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libpinkemu.so"))
        for idx in ([0], launches[0]):
            assert lib.pinkhip_emu_plan_solve(ctypes.byref(PackedArgs(take(batch, idx)).desc), ctypes.byref(planned)) == 0
            assert tuple(planned)[:5] == c["plan"], (case, tuple(planned))
    packed, lead, chosen = c.get("env") == "packed", c.get("lead", 0), {}
    if not packed:  # the two probes the backend itself has to show the way of (solve_instances)
        many = 4
        for i, want in ((1, lambda o: o[1][0] == 0 and o[2][0] == TABLEAU and o[3][0] >= many), (3, lambda o: o[1][0] == 0 and o[2][0] == HANDOVER)):
            for sd in range(N_CANDIDATES):
                weak_candidate(batch, i, sd, lead)
                if want(launch(where, api, take(batch, [i]), None if active is None else active[[i]], 0, warm)):
                    chosen[names[i]] = sd
                    break
            else:
                pytest.fail(f"{where} {case}: none of {N_CANDIDATES} candidates gives the probe '{names[i]}'")
    # 1. alone (and alone under the short max_iter)
    short = next(L for L in launches if 1 in L)  # (the launch that runs again under the short max_iter holds the probe it stops)
    alone = lambda i, mi: launch(where, api, take(batch, [i]), None if active is None else active[[i]], mi, warm)
    solo = {0: [alone(i, 0) for i in range(n)], SHORT_MAX_ITER: {i: alone(i, SHORT_MAX_ITER) for i in sorted(set(short))}}
    paths = {names[i]: int(solo[0][i][2][0]) for i in range(n)}
    statuses = {names[i]: int(solo[0][i][1][0]) for i in range(n)}
    print(f"\n{where} {case}: solo status / path " + ", ".join(f"{k} {statuses[k]}/{PATH_NAMES[paths[k]]}" for k in names))
    # the ways through the code the case stands for
    if packed:
        assert all(paths[k] == GI for k in names), paths
        steps = [int(solo[0][i][3][0]) for i in range(P)]
        assert len(set(steps)) >= 3 and min(steps) <= 1 and max(steps) >= 4, steps  # (the probes vary the step count)
    else:
        assert paths["interior"] == TABLEAU and int(solo[0][0][3][0]) <= 1, (paths, solo[0][0][3])
        assert paths["exchanges"] == TABLEAU and int(solo[0][1][3][0]) >= many, (paths, solo[0][1][3])
        assert paths["routed"] == ROUTED and paths["handover"] == HANDOVER, paths
    assert all(statuses[k] == 0 for k in PROBES), statuses
    assert statuses["empty_box"] == 2 and statuses.get("inconsistent_rows", 2) == 2, statuses
    assert int(solo[SHORT_MAX_ITER][1][1][0]) == 1, "the short launch does not stop the probe with many exchanges"
    for i in range(P):
        anchor_solve_probe(case, names[i], take(batch, [i]), solo[0][i][0][0], statuses[names[i]])
    # 2. in company, 3. compared
    compared = differed = 0
    diffs = []
    plan = [(L, 0) for L in launches] + [(short, SHORT_MAX_ITER)]
    for L, mi in plan:
        out = launch(where, api, take(batch, L), None if active is None else active[L], mi, warm)
        for pos, i in enumerate(L):
            got = [f[pos] if f is not None else None for f in out]
            bad = compare_solve(solo[mi][i], got, i, i < P)
            compared += 1
            if bad:
                differed += 1
                diffs.append(f"{names[i]} at {pos} of {[names[j] for j in L]} (max_iter {mi}): {bad}")
    RECORD[(case, where)] = dict(arrangements=len(plan), placements=compared, differed=differed, groups_per_wave=per,
                                 paths=sorted({PATH_NAMES[p] for p in paths.values()}), chosen_candidates=chosen, solo={k: [statuses[k], PATH_NAMES[paths[k]]] for k in names})
    _dump_record()
    assert not diffs, f"{where} {case}: {differed} of {compared} placements differ from solo\n" + "\n".join(diffs[:20])


def _dump_record():
    out = os.environ.get("PINKHIP_WAVE_ISOLATION_RECORD")
    if out:
        for where in {w for _, w in RECORD}:
            with open(f"{out}.cases.{where}.json", "w") as f:
                json.dump({k: v for (k, w), v in sorted(RECORD.items()) if w == where}, f, indent=1)


# ----------------------------------------------------------------------------------------------- whole-step families

# name -> the robot, the barriers, warm start, lanes per robot, dense rows the rollout must report
ROLLOUT_CASES = {
    "rollout-12-0-16": dict(robot="arm12", bars=None, W=16, md=0),
    "rdense-12-4-16": dict(robot="arm12", bars="rdense", W=16, md=1),
    "wrollout-16-0-16": dict(robot="arm12", bars=None, warm=True, W=16, md=0),
    # (the SelfCollisionBarrier's safe-displacement term regularises every coordinate: this stack is never routed)
    "rpairs-12-4-16": dict(robot="arm12", bars="rpairs", W=16, md=2, routes=False),
    # (30 coordinates: the interior probes need the stronger damping to stay within what the fp64 reference resolves)
    "rdense-30-6-32": dict(robot="big30", bars="two", W=32, md=6, lm=1.0),
}
ROLLOUT_PROBES = ["interior", "exchanges", "routed", "handover"]
DT = 5e-3
# A weak posture task and a strong Levenberg-Marquardt term (mu |e|^2 on the diagonal): the conditioning of a robot's QP
# follows its own distance to the target -- 10 um away the estimate is beyond the routing threshold, millimetres away it
# is not -- so that one rollout, whose costs are the same for every robot, holds robots on every path.
POSTURE_COST, LM_DAMPING = 1e-4, 0.1
N_ROLLOUT_CANDIDATES = 40


def _robot(which):
    from pink_amd import build_chain

    if which == "arm12":  # (the arm of tests/test_kernel_table_launch.py: nv = nj = 12, the 16-lane entries)
        return build_chain(12, seed=5), ["tool0", "joint_6"]
    return build_chain(24, free_flyer=True, seed=2), ["tool0", "joint_12"]  # (tests/test_rollout.py _models()[3]: nv = 30)


def _draw_robot(model, frames, rng, reach):
    """(q, targets [nf, 12]) of one robot: joints in +-0.6, the tool's target ``reach`` metres above the tool, the second
    frame's a fifth of that away in a drawn direction"""
    from pink_amd import Configuration
    from pink_amd.configuration import _rot_to_quat
    from pink_amd.lie import exp6
    from pink_amd.rollout import pose12

    q = model.neutral().copy()
    for j in model.joints:
        if j.kind == "free_flyer":
            M = exp6(rng.normal(size=6) * 0.3)
            q[j.idx_q:j.idx_q + 3], q[j.idx_q + 3:j.idx_q + 7] = M.translation, _rot_to_quat(M.rotation)
        else:
            q[j.idx_q] = rng.uniform(-0.6, 0.6)
    cfg = Configuration(model, q)
    targets = np.zeros((len(frames), 12))
    for i, f in enumerate(frames):
        tgt = cfg.get_transform_frame_to_world(f).copy()
        tgt.translation = tgt.translation + (np.array([0.0, 0.0, reach]) if i == 0 else 0.2 * reach * rng.normal(size=3))
        targets[i] = pose12(tgt)
    return q, targets


class Robots:
    """The instances of a whole-step case: probes
    each the first of a fixed seeded list of draws (``reference_resolves`` ones only) that takes its way on the backend
    under test in its first step, status 0 in both:
      interior   targets 3 .. 10 mm away, on the tableau with at most one exchange
      exchanges  the tool's target 8 .. 30 cm above it, on the tableau through four exchanges or more (velocity limits bind)
      routed     targets 0.1 .. 10 um away, sent to the Goldfarb-Idnani code by the conditioning estimate
      handover   targets 0.1 .. 3 mm away, handed over in one of the two steps (none of the list: its first draw, and the
                 record says so -- next to the company every probe still goes through the wave's hand-over)
    and company: a joint beyond its limit (safety_break=False), a NaN joint angle, a NaN target, a target metres away (and,
    warm start, active-set bytes of 255)."""

    def __init__(self, case):
        from tests.test_kernel_table_launch import _barriers
        from pink_amd import Configuration
        from pink_amd.barriers import PositionBarrier

        c = ROLLOUT_CASES[case]
        self.model, self.frames = _robot(c["robot"])
        self.warm = c.get("warm", False)
        self.names = ROLLOUT_PROBES + ["q_outside", "nan_q", "nan_target", "far_target"] + (["active_255"] if self.warm else [])
        self.kinds = [None] * len(ROLLOUT_PROBES) + self.names[len(ROLLOUT_PROBES):]
        self.specs = [(f, 1.0, 0.5 if i == 0 else 0.0, 1.0, c.get("lm", LM_DAMPING)) for i, f in enumerate(self.frames)]
        rng = np.random.default_rng(31 + len(case) + self.model.nv)
        reach = dict(interior=3e-3, routed=1e-5, far_target=5.0)
        draws = [_draw_robot(self.model, self.frames, rng, reach.get(k, 0.08)) for k in self.names]
        self.q0, self.targets = np.array([d[0] for d in draws]), np.array([d[1] for d in draws])
        last = self.model.joints[-1]
        self.q0[self.names.index("q_outside"), last.idx_q] = self.model.upperPositionLimit[last.idx_q] + 0.5
        self.q0[self.names.index("nan_q"), self.model.joints[-2].idx_q] = np.nan
        self.targets[self.names.index("nan_target"), 0, 10] = np.nan
        self.active = None
        if self.warm:
            self.active = np.zeros((len(self.names), self.model.nv), np.uint8)
            self.active[self.names.index("active_255")] = 255
            self.active[1] = rng.integers(0, 3, size=self.model.nv)
        # barriers: one table for every robot, placed by the probes' own start poses (never by an arrangement)
        P = len(ROLLOUT_PROBES)
        p0 = np.array([[Configuration(self.model, q).get_transform_frame_to_world(f).translation for f in self.frames] for q in self.q0[:P]])
        if c["bars"] == "two":  # (tests/test_conditioning_bands.py: three rows each, no safe-displacement term on the diagonal)
            self.bars = [PositionBarrier(self.frames[0], indices=[0, 1, 2], p_max=p0[:, 0].max(axis=0) + 0.01, gain=np.full(3, 50.0)),
                         PositionBarrier(self.frames[1], indices=[0, 1, 2], p_min=p0[:, 1].min(axis=0) - 0.01, gain=np.full(3, 50.0))]
        else:
            self.bars = _barriers(c["bars"], self.model, self.q0[:P]) if c["bars"] else []

    def redraw(self, i, seed, lo, hi):
        rng = np.random.default_rng(seed)
        self.q0[i], self.targets[i] = _draw_robot(self.model, self.frames, rng, 10 ** rng.uniform(np.log10(lo), np.log10(hi)))

    def reference_resolves(self, i):
        """Whether the anchor means something for robot i: the fp64 Goldfarb-Idnani reference is good to about cond eps |v|, and
        the anchor asks 1e-8 of the velocity -- a draw with 10 kappa eps |v| beyond that (the fp64 limit of
        parity_suite.banded_bar, kappa the host estimate of build_ik's P) is passed over.  Looks at the inputs only."""
        from oracle.refined_kkt import conditioning_estimate

        qp = self.host_qp(i)
        x, status, _, _ = c_oracle.gi_solve(qp.P, qp.q, qp.G, qp.h)
        kappa = float(conditioning_estimate(np.asarray(qp.P)[None])[0])
        return status == 0 and 10.0 * kappa * np.finfo(float).eps * float(np.abs(x).max()) / DT <= 1e-8

    def host_qp(self, i):
        """build_ik's QP of robot i at its start (the anchor of tests/test_kernel_table_launch.py)"""
        import pink_amd
        from pink_amd import Configuration, FrameTask, PostureTask
        from pink_amd.lie import SE3

        tl = []
        for k, (f, pc, oc, gain, lm) in enumerate(self.specs):
            t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
            t.set_target(SE3(self.targets[i, k, :9].reshape(3, 3), self.targets[i, k, 9:]))
            tl.append(t)
        p = PostureTask(cost=POSTURE_COST)
        p.set_target(self.q0[i])
        return pink_amd.build_ik(Configuration(self.model, self.q0[i]), tl + [p], DT, barriers=self.bars or None)


def rollout_launch(api, r, idx, max_iter, md):
    """Two integrated steps of the robots ``idx`` in one rollout: per robot dq, status, path, iters of both steps, q after
    each (the first integrated by the second launch itself, the second by the flush), first_failure after each and, warm
    start, the active sets."""
    from pink_amd.rollout import DeviceRollout

    idx = np.asarray(idx)
    B = len(idx)
    ro = DeviceRollout(api, r.model, r.q0[idx], r.specs, DT, posture_cost=POSTURE_COST, fused="kernel", position_barriers=r.bars, warm_start=r.warm,
                       safety_break=False, max_iter=max_iter)
    out = {}
    try:
        ro.set_targets(r.targets[idx])
        if r.warm:
            ro.set_active(np.ascontiguousarray(r.active[idx]))
        for step in (1, 2):
            ro.step()
            api.sync()
            assert ro.fused == "kernel" and ro.md == md and ro.nv == r.model.nv, (ro.fused, ro.md)
            dq, st, it = ro.last_step()
            out[f"dq{step}"], out[f"status{step}"], out[f"iters{step}"], out[f"path{step}"] = dq, st, it, np.asarray(ro.last_path).copy()
            if r.warm:
                out[f"active{step}"] = ro.last_active()
            if step == 2:  # (the second launch has integrated the first step; its own dq is still pending)
                out["q1"], out["fail1"] = np.zeros((B, r.model.nq)), np.zeros(B, np.int32)
                api.get(out["q1"], ro.d_q), api.get(out["fail1"], ro.d_fail)
        out["q2"] = ro.configurations()
        api.sync()
        out["fail2"] = np.zeros(B, np.int32)
        api.get(out["fail2"], ro.d_fail)
    finally:
        ro.free()
    return out


def compare_rollout(solo, got, pos, is_probe):
    s = {k: v[0] for k, v in solo.items()}
    g = {k: v[pos] for k, v in got.items()}
    ok1, ok2 = int(s["status1"]) == 0, int(s["status1"]) == 0 and int(s["status2"]) == 0
    strict = is_probe and 1 not in (int(s["status1"]), int(s["status2"]))  # (out of iterations: company, whoever it is)
    bad = [k for k in ("status1", "status2", "path1", "path2", "fail1", "fail2") if int(g[k]) != int(s[k])]
    for k, when in (("dq1", ok1), ("q1", ok1), ("dq2", ok2), ("q2", ok2)):
        if (strict or when) and not np.array_equal(bits(g[k]), bits(s[k])):
            bad.append(k)
    for k in ("iters1", "iters2", "active1", "active2"):
        if strict and k in s and not np.array_equal(g[k], s[k]):
            bad.append(k)
    return bad


@pytest.mark.parametrize("case", list(ROLLOUT_CASES))
def test_whole_step_families(backend, case, monkeypatch):
    import pink_amd
    from pink_amd.runtime import set_default_solver
    from tests.test_self_collision_device import PairsSpy

    where, api = backend
    monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
    c = ROLLOUT_CASES[case]
    per, md, P = 64 // c["W"], c["md"], len(ROLLOUT_PROBES)
    if where == "emu":  # (the emulator's rollout_step_pairs is not part of the ``emu`` fixture)
        api = PairsSpy(api, api._emu, False)
    r = Robots(case)
    n = len(r.names)
    launches = arrangements(P, n - P, per)
    check_coverage(launches, P, r.kinds, per)
    set_default_solver(api)
    try:
        chosen = {}
        stays = lambda o: o["status1"][0] == 0 and o["status2"][0] == 0
        wants = ((0, 3e-3, 1e-2, lambda o: stays(o) and o["path1"][0] == TABLEAU and o["iters1"][0] <= 1),
                 (1, 0.08, 0.3, lambda o: stays(o) and o["path1"][0] == TABLEAU and o["iters1"][0] >= 4),
                 (2, 1e-7, 1e-5, lambda o: stays(o) and o["path1"][0] == ROUTED),
                 (3, 1e-4, 3e-3, lambda o: stays(o) and HANDOVER in (o["path1"][0], o["path2"][0])))
        for i, lo, hi, want in wants:
            first = None
            for sd in range(7000, 7000 + N_ROLLOUT_CANDIDATES):
                r.redraw(i, sd, lo, hi)
                if not r.reference_resolves(i):
                    continue
                first = sd if first is None else first
                if want(rollout_launch(api, r, [i], 0, md)):
                    chosen[r.names[i]] = sd
                    break
            else:
                assert first is not None, (case, r.names[i], "no candidate the fp64 reference resolves")
                r.redraw(i, first, lo, hi)
        short = next(L for L in launches if 1 in L)
        solo = {0: [rollout_launch(api, r, [i], 0, md) for i in range(n)],
                SHORT_MAX_ITER: {i: rollout_launch(api, r, [i], SHORT_MAX_ITER, md) for i in sorted(set(short))}}
        show = {r.names[i]: (int(solo[0][i]["status1"][0]), int(solo[0][i]["status2"][0]), PATH_NAMES[solo[0][i]["path1"][0]], PATH_NAMES[solo[0][i]["path2"][0]],
                             int(solo[0][i]["iters1"][0])) for i in range(n)}
        print(f"\n{where} {case}: solo (status, status, path, path, iters of step 1) {show}")
        # (a robot that reaches its target in the first step is routed in the second: only the first path is stated)
        assert show["interior"][:3] == (0, 0, "tableau") and show["interior"][4] <= 1, show
        assert show["exchanges"][:3] == (0, 0, "tableau") and show["exchanges"][4] >= 4, show
        assert show["routed"][:3] == (0, 0, "routed") or not c.get("routes", True), show
        assert show["handover"][:2] == (0, 0) and ("handover" not in chosen or "handover" in show["handover"][2:4]), show
        assert show["q_outside"][0] != 0 and show["nan_q"][0] != 0 and show["nan_target"][0] != 0, show
        worst = 0.0
        for i in range(P):  # anchors
            qp = r.host_qp(i)
            x, status, _, _ = c_oracle.gi_solve(qp.P, qp.q, qp.G, qp.h)
            assert status == 0
            err = float(np.abs(solo[0][i]["dq1"][0] - x).max()) / DT
            print(f"{case} {r.names[i]}: max|v - v_oracle| = {err:.3e}")
            worst = max(worst, err)
        assert worst < 1e-8, worst
        compared = differed = 0
        diffs = []
        plan = [(L, 0) for L in launches] + [(short, SHORT_MAX_ITER)]
        for L, mi in plan:
            out = rollout_launch(api, r, L, mi, md)
            for pos, i in enumerate(L):
                bad = compare_rollout(solo[mi][i], out, pos, i < P)
                compared += 1
                if bad:
                    differed += 1
                    diffs.append(f"{r.names[i]} at {pos} of {[r.names[j] for j in L]} (max_iter {mi}): {bad}")
    finally:
        pink_amd.clear_device_cache()
        set_default_solver(None)
    paths = sorted({p for v in show.values() for p in v[2:4]})
    RECORD[(case, where)] = dict(arrangements=len(plan), placements=compared, differed=differed, groups_per_wave=per, paths=paths,
                                 chosen_candidates=chosen, solo={k: list(v) for k, v in show.items()})
    _dump_record()
    assert not diffs, f"{where} {case}: {differed} of {compared} placements differ from solo\n" + "\n".join(diffs[:20])
