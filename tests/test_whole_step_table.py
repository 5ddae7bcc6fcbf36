"""Every instantiation of the whole-step kernels (ik_rollout_kernel, ik_rollout_warm_kernel: the rollout, rdense and wrollout
lines of ``pinkhip_emu_table_text()``) against the exact minimiser of the QP its robot states, on the emulator and on the
MI355X.  The task, barrier, limit and equality rows of these kernels never reach memory: dq (and q after integration) is
where a wrong row, lane mask or LDS offset shows.  Cases: tests/whole_step_cases.py.

Reference: the rows of the host evaluation (pack_configurations(..., gpu_frame_tasks=False)) and x* of
oracle.refined_kkt.batch_minimiser started from the fp64 C oracle's point -- never the kernel, the emulator or the device
route.  The host rows are held to oracle/exact_kinematics.py here for one instance per tree (1e-12).

Bars.  |dq - x*| <= parity_suite.banded_bar(kappa, |x*|, err_oracle, floor): 1e-8 max(1, |x*|) below an estimate of 1e6.
Stacks b and c (kappa 3e9 .. 1e13, where banded_bar is loose along the flat directions) are also held in the range space:
r(dq) = max(max |W J (dq - x*)| over the task rows, violation of every box, dense and equality row by dq) must stay within
max(1e-8 max(1, |x*|), 10 r(dq_oracle)).  Measured for the fp64 C oracle before any kernel ran (profiles/whole_step_table.json,
"oracle"): r(dq_oracle) <= 5.7e-11 on the b cases and <= 7e-16 on the c cases, so the limit is the 1e-8 term everywhere.

The sensitivity test drops every term of every case from the reference QP: x* must move by 100 x the case's bar in at least
half of the instances -- |x* - x*_dropped| >= 100 banded_bar; for stacks b / c, which are held to two bars, by that or by
r(x*_dropped) >= 100 x the range-space limit (a kernel that lost the term would return x*_dropped and miss that bar).

Run times: a case takes well under a second on the MI355X (B = 3 / 5 / 9).  The emulator leaves the nf = 32 variants to the GPU
(_on_emulator: one nf variant per entry and shape stays, nf = 1, plus nf = 17 at W = 16, on rdense<12,4,16> too); its half of
this module takes about two and a half minutes, a third of it the 60-digit checks and the sensitivity test.

PINK_WHOLE_STEP_TABLE=<file>: the worst values per entry and path of this run are merged into that JSON file."""
import ctypes
import json
import os

import numpy as np
import pytest

from pink_amd import Configuration
from pink_amd._lib import Desc, PinkHipError, RolloutStep, Warm
from pink_amd.rollout import ModelArrays

from tests import parity_suite as ps
from tests import whole_step_cases as wc

CASES = wc.cases()
CASE_IDS = [c.id for c in CASES]
EPS = np.finfo(float).eps


class EmuApi:
    """The ``emu`` fixture's object plus rollout_step_warm of BatchSolver's raw interface, on host memory."""

    def __init__(self, emu):
        self._emu = emu
        emu.lib.pinkhip_emu_rollout_step_warm.argtypes = [ctypes.POINTER(Desc), ctypes.c_void_p, ctypes.POINTER(RolloutStep), ctypes.POINTER(Warm)]
        emu.lib.pinkhip_emu_warm_last_error.restype = ctypes.c_char_p

    def __getattr__(self, name):
        return getattr(self._emu, name)

    def rollout_step_warm(self, desc, model, args, warm):
        rc = self._emu.lib.pinkhip_emu_rollout_step_warm(ctypes.byref(desc), model, ctypes.byref(args), ctypes.byref(warm))
        if rc != 0:
            raise PinkHipError(rc, self._emu.lib.pinkhip_emu_warm_last_error().decode())


def _api(request, where):
    if where == "emu":
        return EmuApi(request.getfixturevalue("emu"))
    return request.getfixturevalue("gpu_solver")


def _on_emulator(case):
    """The emulator runs one nf variant per entry and shape -- nf = 1 on the full robot (what the padded and the
    one-joint-per-lane robots carry is their only variant), plus nf = 17 at W = 16 -- and leaves the nf = 32 variants to the
    GPU: they are where the emulator's minutes went (5 .. 10 s each at W = 64)."""
    return case.nf != wc.MAX_FRAMES


def _runs(cases):
    out = []
    for c in cases:
        if _on_emulator(c):
            out.append(pytest.param("emu", c, id=f"emu-{c.id}"))
        out.append(pytest.param("gpu", c, id=f"gpu-{c.id}", marks=pytest.mark.gpu))
    return out


# ------------------------------------------------------------------------------------------------------------- measurements
_MEAS = {}


def _note(where, case, path, **values):
    """Worst value per (backend, entry, path name) of each quantity."""
    key = f"{case.prefix}<{case.entry[0]},{case.entry[1]},{case.entry[2]}>"
    slot = _MEAS.setdefault(where, {}).setdefault(key, {}).setdefault(path, {})
    for k, v in values.items():
        slot[k] = max(slot.get(k, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def _measurements_file():
    yield
    path = os.environ.get("PINK_WHOLE_STEP_TABLE")
    if path and _MEAS:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        for where, entries in _MEAS.items():
            for key, paths in entries.items():
                old.setdefault(where, {}).setdefault(key, {}).update(paths)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
            f.write("\n")


PATH_NAMES = ["tableau", "handover", "routed", "gi"]
STACK_PATHS = {"a": (wc.PATH_TABLEAU,), "b": (wc.PATH_HANDOVER, wc.PATH_ROUTED), "c": (wc.PATH_GI,)}


def _oracle_note(case):
    """The fp64 C oracle's own distance from x* and its range-space quantity, under the path the stack is meant to take."""
    r = wc.range_space_quantity(case.pf, case.ref["dq"], case.x)
    name = {"a": "tableau", "b": "routed", "c": "gi"}.get(case.stack, "tableau")
    _note("oracle", case, name, err=case.err_oracle.max(), range=r.max(), kappa=case.kappa.max())
    return r


# ------------------------------------------------------------------------------------------------------------------ launching
def _step(api, ro, integrate, null_outputs=False, active_in=True):
    """One whole step of ``ro``; ``null_outputs``: T_frames and iters NULL; ``active_in`` False: the warm twin with active_in NULL."""

    def launch(st, lo=0):
        if null_outputs:
            st.T_frames, st.iters = None, None
        if ro.warm_start:
            w = Warm()
            w.active_in, w.active_out = (ro.d_active if active_in else None), ro.d_active
            api.rollout_step_warm(ro.desc, ro.dmodel, st, w)
            return True
        return api.rollout_step(ro.desc, ro.dmodel, st)

    ro._launch_whole_step = launch
    try:
        ro.step(integrate=integrate)
        api.sync()
    finally:
        del ro._launch_whole_step
    assert ro.fused == "kernel", "the whole-step kernel refused the case"


def _results(api, ro):
    dq, st, raw = np.empty((ro.B, ro.nv)), np.empty(ro.B, np.int32), np.empty(ro.B, np.int32)
    api.get(dq, ro.d_dq), api.get(st, ro.d_status), api.get(raw, ro.d_iters)
    return dq, st, raw & 0xFFFFFF, raw >> 24


def _check_point(where, case, dq, path, tag=""):
    """The bars of the module docstring on one returned dq [B, nv]."""
    err = np.abs(dq - case.x).max(axis=1)
    r = wc.range_space_quantity(case.pf, dq, case.x)
    r_oracle = _oracle_note(case)
    ratio = err / np.maximum(np.maximum(case.err_oracle, case.kappa * EPS * case.xmax), 1e-300)
    for b in range(case.B):
        _note(where, case, PATH_NAMES[int(path[b])], err=err[b], range=r[b], kappa=case.kappa[b], ratio=ratio[b])
    print(f"{where} {case.id}{tag}: kappa {case.kappa.max():.2e} |dq - x*| {err.max():.2e} (oracle {case.err_oracle.max():.2e}, bar {case.bar.min():.2e}) "
          f"range {r.max():.2e} (oracle {r_oracle.max():.2e}) paths {sorted(set(int(p) for p in path))}")
    assert (err <= case.bar).all(), (case.id, tag, err, case.bar, path)
    if case.stack in ("b", "c"):
        lim = np.maximum(ps.TOL_EXACT * np.maximum(1.0, case.xmax), 10.0 * r_oracle)
        assert (r <= lim).all(), (case.id, tag, r, lim, path)


# ----------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("where,case", _runs(CASES))
def test_entry_against_the_exact_minimiser(request, where, case):
    api = _api(request, where)
    case.build()
    ro = case.rollout(api)
    try:
        plan = wc.planned_entry(ro)
        assert plan is not None and plan[0] == wc.PLAN_KIND[case.prefix] and plan[1:4] == case.entry, (case.id, plan)
        assert plan[5] == 3  # (two full wavefronts of groups and the tail group)
        _step(api, ro, False, active_in=False)
        dq, st, it, path = _results(api, ro)
        assert (st == 0).all(), (case.id, st)
        want = STACK_PATHS.get(case.stack, (wc.PATH_TABLEAU,))
        assert np.isin(path, want).all(), (case.id, path, want)
        _check_point(where, case, dq, path)
        if case.warm:  # the exact set of the reference, then random bytes: the same minimiser and status, no exchange from the exact set
            assert it.sum() > 0 or (case.active == 0).all()
            cold = dq
            ro.set_active(case.active)
            _step(api, ro, False)
            dq, st, it_exact, path = _results(api, ro)
            assert (st == 0).all() and (path == wc.PATH_TABLEAU).all(), (case.id, st, path)
            _check_point(where, case, dq, path, " exact set")
            assert np.abs(dq - cold).max() <= 2.0 * case.bar.min()
            assert it_exact.sum() == 0, (case.id, it_exact, it)
            assert np.array_equal(ro.last_active(), case.active)
            ro.set_active(np.random.default_rng(case.seed).integers(0, 256, size=case.active.shape, dtype=np.uint8))
            _step(api, ro, False)
            dq, st, _, path = _results(api, ro)
            assert (st == 0).all() and (path == wc.PATH_TABLEAU).all(), (case.id, st, path)
            _check_point(where, case, dq, path, " random bytes")
            assert np.array_equal(ro.last_active(), case.active)
            first = cold.copy()  # T_frames and iters NULL (active_in NULL, as the first launch): bit-identical results
            api.put(ro.d_dq, np.full((ro.B, ro.nv), -7.0)), api.put(ro.d_status, np.full(ro.B, -9, dtype=np.int32))
            _step(api, ro, False, null_outputs=True, active_in=False)
            dq2, st2 = np.empty_like(first), np.empty(ro.B, np.int32)
            api.get(dq2, ro.d_dq), api.get(st2, ro.d_status)
            assert np.array_equal(dq2, first) and (st2 == 0).all(), (case.id, np.abs(dq2 - first).max(), st2)
            assert np.array_equal(ro.last_active(), case.active)
        else:  # T_frames and iters NULL: bit-identical results
            first = dq.copy()
            api.put(ro.d_dq, np.full((ro.B, ro.nv), -7.0)), api.put(ro.d_status, np.full(ro.B, -9, dtype=np.int32))
            _step(api, ro, False, null_outputs=True)
            dq2, st2 = np.empty_like(first), np.empty(ro.B, np.int32)
            api.get(dq2, ro.d_dq), api.get(st2, ro.d_status)
            assert np.array_equal(dq2, first) and (st2 == 0).all(), (case.id, np.abs(dq2 - first).max(), st2)
    finally:
        ro.free()


def _one_per_entry():
    seen, out = set(), []
    for c in CASES:
        if (c.prefix, c.entry) not in seen:
            seen.add((c.prefix, c.entry))
            out.append(c)
    return out


@pytest.mark.parametrize("where,case", _runs(_one_per_entry()))
def test_two_integrated_steps(request, where, case):
    """integrate = 1 for two steps: after each, q is exact_kinematics.integrate(q before, dq returned) and T_frames the host
    poses of the configuration the step solved at, to 1e-12.  The second step starts from what the first one wrote."""
    from oracle import exact_kinematics as ek

    api = _api(request, where)
    case.build()
    ro = case.rollout(api)
    arr = ro.arrays
    try:
        q_prev = case.q0.copy()
        for step in range(2):
            _step(api, ro, True)
            dq, st, _, _ = _results(api, ro)
            assert (st == 0).all(), (case.id, step, st)
            q, T = np.zeros((ro.B, ro.nq)), ro.frame_poses()
            api.get(q, ro.d_q)
            worst_q = worst_T = 0.0
            for b in range(ro.B):
                want = ek.integrate(arr, q_prev[b], dq[b])
                for j in range(len(arr.parent)):
                    jt, iq = int(arr.jtype[j]), int(arr.idx_q[j])
                    got = ek.joint_matrix(jt, arr.axis[j], q[b, iq:iq + (7 if jt == ek.FREE_FLYER else 1)])
                    worst_q = max(worst_q, max(abs(float(got[r][c] - want[j][r][c])) for r in range(3) for c in range(4)))
                cfg = Configuration(case.model, q_prev[b])
                for f, name in enumerate(case.frames):
                    worst_T = max(worst_T, float(np.abs(T[b, f] - wc.pose12(cfg.get_transform_frame_to_world(name))).max()))
            print(f"{where} {case.id} step {step}: |q - q (+) dq| {worst_q:.2e}, |T_frames - host| {worst_T:.2e}")
            assert worst_q <= 1e-12 and worst_T <= 1e-12, (case.id, step, worst_q, worst_T)
            q_prev = q
        assert np.abs(q_prev - case.q0).max() > 1e-4  # (the robots moved)
    finally:
        ro.free()


# ------------------------------------------------------------------------------------------------------------ the cases themselves
def test_every_table_entry_has_a_case():
    """A line of the whole-step tables without a case whose plan is that entry fails here (the plan of each case is asked again
    in test_entry_against_the_exact_minimiser, on both backends)."""
    entries = wc.table_entries()
    reached = {(c.prefix, c.entry) for c in CASES}
    missing = [e for e in entries if (e[0], e[1:]) not in reached]
    print(f"{len(entries)} entries, {len(CASES)} cases; shapes no robot reaches: {wc.UNREACHED}")
    assert not missing, missing
    count = {p: sum(1 for e in entries if e[0] == p) for p in wc.PREFIXES}
    assert count == {"rollout": 10, "rdense": 7, "wrollout": 4}, count
    for c in CASES:  # every case from a plan-only rollout of its own tables
        ro = c.build().rollout(wc._PlanApi())
        try:
            assert wc.planned_entry(ro)[1:4] == c.entry, c.id
        finally:
            ro.free()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_dropped_term_moves_the_reference(case):
    """No kernel: every term of the stack dropped from the reference QP moves x* by 100 x the case's bar in at least half of the
    instances (module docstring).  In stacks a / b / c instance 0 stays inside its box and most others do not."""
    failures = case.build().shortfalls()
    assert not failures, (case.id, failures)


GUARD_FRAMES = 4  # tip_a, tip_b (every joint of the tree lies under one of them), f0, f1: ~1 s of 60-digit arithmetic per frame


def _trees():
    """One case per tree (scalar joints, root): the one with the most frames."""
    best = {}
    for c in CASES:
        k = (c.n_scalar, c.free_flyer)
        if k not in best or c.nf > best[k].nf:
            best[k] = c
    return list(best.values())


@pytest.mark.parametrize("case", _trees(), ids=[f"{c.n_scalar}{'ff' if c.free_flyer else ''}-nf{c.nf}" for c in _trees()])
def test_host_rows_against_exact_kinematics(case):
    """The guard under the reference: e and J of the host evaluation's first FrameTask rows of instance 0 against the 60-digit
    kinematics, e = log6(T_f^-1 T_t) and -Jlog6(T_t^-1 T_f) J_body (as tests/test_kinematics_exact.py states them)."""
    from oracle import exact_kinematics as ek

    case.build()
    arr = ModelArrays(case.model, case.frames[:GUARD_FRAMES])
    Ts, Js = ek.kinematics(arr, case.q0[0])
    rows = case.pf["rows"]
    worst = 0.0
    for f in range(min(case.nf - case.eq, GUARD_FRAMES)):
        X = ek.pose_matrix(case.targets[0, f])
        e = np.array([float(v) for v in ek.log6(ek.mm(ek.inverse(Ts[f]), X))])
        Jl = ek.jlog6(ek.mm(ek.inverse(X), Ts[f]))
        J = -np.array([[float(v) for v in row] for row in ek.mm(Jl, Js[f])])
        r0 = int(rows[f])
        worst = max(worst, float(np.abs(case.pf["e"][0, r0:r0 + 6] - e).max()), float(np.abs(case.pf["J"][0, r0:r0 + 6] - J).max()))
    print(f"{case.id}: host FrameTask rows against the exact kinematics: {worst:.2e}")
    assert worst <= 1e-12, (case.id, worst)
