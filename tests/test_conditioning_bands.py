"""Every solver path against the high-precision minimiser x* of the QP, banded by conditioning.

The contract is |dq - x*| <= 1e-8 max(1, |x*|).  The tableau kernels (ik_sweep.h, ik_sweepx.h) update an explicit inverse
of H, which loses up to cond(H)^2 eps, and accept their point on a KKT certificate; instances whose conditioning estimate
max_i H_ii (H^-1)_ii exceeds PINKHIP_SWEEP_ROUTE_COND go to the Goldfarb-Idnani code instead.  This module measures the
band below that threshold, where nothing else holds the kernels to the contract: problems are drawn per family of shapes
(tests/parity_suite.BANDED_FAMILIES, one per instantiation kind of dispatch.h), binned by the host estimate kappa of the
full stacked H (which bounds the kernel's estimate on any free set from above) into [1e2, 1e4) (control), one band per
decade up to [1e7, 1e8), and [1e8, 1e11), and compared with x* from oracle/refined_kkt.py (longdouble-refined KKT solve of
the active set, certified; its own accuracy ~kappa 2^-64 |x|).

The bar (parity_suite.banded_bar): below kappa 1e6 every feasible instance within 1e-8 max(1, |x*|) on every path,
absolute, not scaled by cond.  From 1e6 on, the largest of that, 10 |dq_oracle - x*| (the rule of test_exact_anchor.py)
and 10 kappa eps |x*|: measured on the MI355X, the fp64 C oracle is itself 2e-8 .. 5e-7 from x* in [1e6, 1e8) and the
Goldfarb-Idnani kernel 1e-8 .. 8e-8, so no fp64 solve meets an absolute 1e-8 on every draw there; the kernels' worst
error per band stays below the oracle's from 1e4 on.  Statuses equal the C oracle's.  Each family runs three legs -- default dispatch and PINKHIP_SOLVER=sweep, which must report a tableau path
(0 / 1 / 2), and PINKHIP_SOLVER=packed, which must report path 3 -- so that no leg quietly tests another kernel.

Sizes: GPU_PER_BAND = 2000 instances per band per family on the MI355X; EMU_PER_BAND = 8 on the emulator (5 families x
6 bands x 8 = 240 instances, three legs each; the module takes about two minutes on 8 CPUs).  Run with -s for the per-band table.
"""
import numpy as np
import pytest

from oracle import c_oracle
from oracle.refined_kkt import batch_minimiser, conditioning_estimate
from tests import parity_suite as ps

GPU_PER_BAND = 2000
EMU_PER_BAND = 8
SEED0 = {"box": 7_100_000, "eliminating": 7_200_000, "dense": 7_300_000, "virtual": 7_400_000, "equality": 7_500_000}
LEGS = (("default", None, (0, 1, 2)), ("sweep", "sweep", (0, 1, 2)), ("packed", "packed", (3,)))
ROUND6_SEEDS = [3063897, 3074349, 3085897, 415035]  # weakly regularised draws of fuzz(ill=True): 2e-5 .. 8e-5 off x* (round 6), 1.3e-6 (round 3)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def solver(request):
    return request.param, request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver")


def _violations_message(family, leg, rec, bad):
    worst = bad[np.argsort(-rec["err"][bad])][:8]
    return [f"{family}/{leg}: seed {int(rec['seed'][i])} instance {int(rec['instance'][i])} kappa {rec['kappa'][i]:.3e} "
            f"(final free set {rec['kappa_final'][i]:.3e}) path {int(rec['path'][i])}: |dq - x*| = {rec['err'][i]:.3e}, "
            f"oracle {rec['err_oracle'][i]:.3e}, |x*| = {rec['xmax'][i]:.2e}" for i in worst]


@pytest.mark.parametrize("family", list(ps.BANDED_FAMILIES))
def test_conditioning_bands(solver, family, monkeypatch):
    where, s = solver
    per_band = GPU_PER_BAND if where == "gpu" else EMU_PER_BAND
    problems, filled = ps.banded_problems(family, per_band, SEED0[family], batch=256 if where == "gpu" else 48,
                                          max_draws=100000 if where == "gpu" else 4000)
    assert (filled == per_band).all(), ("the generator did not fill every band", family, filled)
    reference, lines, failures, routed_top, fallbacks = {}, [], [], 0.0, 0
    for leg, env, paths in LEGS:
        if env is None:
            monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
        else:
            monkeypatch.setenv("PINKHIP_SOLVER", env)
        rec, fb = ps.fuzz_banded(s, family, per_band, SEED0[family], problems=problems, expect_paths=paths, reference=reference)
        fallbacks += fb  # (the reference is computed on the first leg and reused by the others)
        lines += ps.band_table(family, leg, rec)
        bad = ps.banded_violations(rec)
        if len(bad):
            failures += _violations_message(family, leg, rec, bad)
        top = rec["band"] == len(ps.BANDS) - 1
        if leg != "packed" and top.any():
            routed_top = max(routed_top, float(np.isin(rec["path"][top], (1, 2)).mean()))
        assert (rec["status_oracle"] == 0).sum() >= 0.5 * len(rec["status"]), ("too few feasible draws", family, leg)
    print(f"\n{where} {family}: reference handed {fallbacks} instances to exact_minimiser; routed or handed-over share in the "
          f"top band {routed_top:.3f}\n" + "\n".join(lines))
    assert not failures, "\n".join(failures)


def test_routing_is_visible_above_the_threshold(solver, monkeypatch):
    """Beyond the threshold the tableau kernel must route (or hand over) a visible share of the instances: box-only, the
    family whose flat directions are not all held by rows."""
    where, s = solver
    per_band = 200 if where == "gpu" else EMU_PER_BAND
    problems, _ = ps.banded_problems("box", per_band, SEED0["box"], batch=48)
    monkeypatch.setenv("PINKHIP_SOLVER", "sweep")
    rec, _ = ps.fuzz_banded(s, "box", per_band, SEED0["box"], problems=problems)
    top = rec["band"] == len(ps.BANDS) - 1
    low = rec["band"] == 0
    assert np.isin(rec["path"][top], (1, 2)).mean() > 0.0, rec["path"][top]
    assert (rec["path"][low] == 0).all()  # (the control band stays on the tableau)


def test_round6_seeds_against_the_minimiser(solver, monkeypatch):
    """fuzz(ill=True) seeds 3063897, 3074349, 3085897 (certified tableau points 2e-5 .. 8e-5 from x* before the routing
    threshold came down to 1e8) and 415035: with the bar of the bands, under the default dispatch and the sweep kernel."""
    where, s = solver
    for env in (None, "sweep"):
        if env is None:
            monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
        else:
            monkeypatch.setenv("PINKHIP_SOLVER", env)
        recs = []
        assert ps.fuzz(s, ROUND6_SEEDS, ill=True, exact_records=recs) >= 12
        for sd, b, kap, eg, eo, xm, path in recs:
            assert eg <= ps.banded_bar(kap, xm, eo), (env, sd, b, kap, path, eg, eo)


# ---------------------------------------------------------------------------------------------------------- the reference


def test_reference_reproduces_the_published_examples():
    """Goldfarb & Idnani's worked example and the qpsolvers README example (tests/test_exact_anchor.py), started from the
    origin (a wrong active set): the same minimisers as exact_minimiser, to 1e-12."""
    from oracle.exact_qp import exact_minimiser
    from tests.test_published_qp import GI_A, GI_b, GI_d, GI_X, M, QS_A, QS_G, QS_X, QS_b, QS_h

    one = (np.ones(3), [1.0], [0.0], [0, 3])
    x, info = batch_minimiser(np.eye(3)[None], -GI_d[None], *one, 0.0, -GI_A.T[None], -GI_b[None], [np.zeros((1, 3))])
    xe, _ = exact_minimiser(np.eye(3), -GI_d, *one, 0.0, -GI_A.T, -GI_b, np.zeros(3))
    assert np.abs(x[0] - xe).max() < 1e-12 and np.abs(x[0] - GI_X).max() < 5e-8 and info["fallback"] == 0
    G, h = np.vstack([QS_A, QS_G]), np.concatenate([QS_b, QS_h])
    x, info = batch_minimiser(M[None], np.array([[3.0, 2.0, 3.0]]), *one, 0.0, G[None], h[None], [np.zeros((1, 3))], meq=1)
    xe, _ = exact_minimiser(M, np.array([3.0, 2.0, 3.0]), *one, 0.0, G, h, np.zeros(3), meq=1)
    assert np.abs(x[0] - xe).max() < 1e-12 and np.abs(x[0] - QS_X).max() < 5e-9 and info["fallback"] == 0


@pytest.mark.parametrize("family", ["box", "dense", "equality"])
def test_reference_against_exact_arithmetic_per_band(family):
    """Three instances per band of the banded generator, up to kappa 1e11: the longdouble-refined minimiser agrees with
    the 50-digit one (oracle/exact_qp.py) to 1e-12 max(1, |x|) below 1e8 and, above, to its own reported accuracy
    (``floor``, ~kappa 2^-64) -- a hundredth of the bar the bands apply there at most.  No kernel involved."""
    from oracle.exact_qp import exact_minimiser

    problems, filled = ps.banded_problems(family, 3, 9_000_000 + len(family), batch=24)
    assert (filled == 3).all()
    seen = np.zeros(len(ps.BANDS), int)
    for sd, shape, batch, pf, mech, keep, band in problems:
        ref = c_oracle.solve_ik_batch(**pf)
        sel = ref["status"][keep] == 0
        kk, bk = keep[sel], band[sel]
        p = ps._take(pf, kk)
        x, info = batch_minimiser(p["J"], p["e"], p["cost"], p["gain"], p["lm"], p["rows"], p["damping"], p["G"], p["h"], [ref["dq"][kk]], meq=p["meq"])
        for j, i in enumerate(kk):
            xe, _ = exact_minimiser(pf["J"][i], pf["e"][i], pf["cost"][i], pf["gain"], pf["lm"], pf["rows"], pf["damping"], pf["G"][i], pf["h"][i],
                                    ref["dq"][i], meq=pf["meq"])
            scale = max(1.0, float(np.abs(xe).max()))
            d = float(np.abs(x[j] - xe).max())
            fl = info["floor"][j]
            tol = 1e-12 if bk[j] < len(ps.BANDS) - 1 else max(1e-12, 10.0 * (0.0 if np.isnan(fl) else fl))
            assert d <= tol * scale, (family, sd, int(i), int(bk[j]), d, fl)
            assert np.isnan(fl) or fl <= 1e-9  # (a hundredth of the bar the bands apply)
            seen[bk[j]] += 1
    assert (seen >= 1).all(), seen


def test_conditioning_estimate_bounds_the_free_set_estimate():
    """For SPD H, max_i H_ii (H^-1)_ii over the whole H bounds the estimate over any principal submatrix (the free set
    the kernel sees): (H_FF^-1)_ii <= (H^-1)_ii by interlacing of the Schur complement."""
    rng = np.random.default_rng(3)
    for nv in (5, 17, 40):
        J = rng.normal(size=(20, nv + 2, nv))
        H = np.einsum("bki,bkj->bij", J, J) + 1e-6 * np.eye(nv)
        free = rng.random(size=(20, nv)) < 0.6
        assert (conditioning_estimate(H, free) <= conditioning_estimate(H) * (1 + 1e-9)).all()


# ------------------------------------------------------------------------------------------------- the whole-step kernels


ROLLOUT_BAND_TARGETS = [1e3, 3e4, 3e5, 3e6, 3e7, 1e9]  # one target kappa per band (kappa ~ 120 / posture_cost^2 here)


def _rollout_q(model, B, rng):
    from pink_amd.configuration import _rot_to_quat
    from pink_amd.lie import exp6

    q = np.tile(model.neutral(), (B, 1))
    for j in model.joints:
        if j.kind == "free_flyer":
            for b in range(B):
                M = exp6(rng.normal(size=6) * 0.3)
                q[b, j.idx_q:j.idx_q + 3] = M.translation
                q[b, j.idx_q + 3:j.idx_q + 7] = _rot_to_quat(M.rotation)
        else:
            q[:, j.idx_q] = rng.uniform(-0.8, 0.8, size=B)
    return q


@pytest.mark.parametrize("md", [0, 6], ids=["30-0-32", "30-6-32"])
def test_whole_step_kernel_bands(solver, md):
    """ik_rollout_kernel<30, 0, 32> (floating base + 24 joints, two FrameTasks, a PostureTask, the default limits) and
    <30, 6, 32> (the same with two PositionBarriers of three rows each, formed on chip: virtual dense rows): these kernels
    start all-free and route in-kernel (ik_rollout.h), so they get their own evidence.  One step from a fixed q with the
    posture cost lowered so that kappa lands in each band; dq against x* of the stack the host evaluation
    (pack_configurations: pink_amd.batch_eval's rows) forms for the same q, with the bar of the bands.  Sizes: 4 posture
    costs per band x 64 robots on the MI355X, 1 x 3 on the emulator."""
    from pink_amd import Configuration, FrameTask, PostureTask, build_chain
    from pink_amd.barriers import PositionBarrier
    from pink_amd.lie import exp6
    from pink_amd.rollout import DeviceRollout, pose12
    from pink_amd.solve_ik import pack_configurations
    from oracle.refined_kkt import objective_ld

    where, s = solver
    B, per = (64, 4) if where == "gpu" else (3, 1)
    model = build_chain(24, free_flyer=True, seed=2)
    frames = ["tool0", "joint_12"]
    specs = [(f, 1.0, 0.5, 1.0, 0.0) for f in frames]
    dt = 5e-3
    assert model.nv == 30
    rec = {k: [] for k in ("band", "kappa", "path", "err", "err_oracle", "xmax", "floor", "tag")}
    fallbacks = 0
    for bi, target in enumerate(ROLLOUT_BAND_TARGETS):
        for rep in range(per):
            sd = 8_100_000 + 1000 * md + 10 * bi + rep
            rng = np.random.default_rng(sd)
            cost = float(np.sqrt(120.0 / target) * 10 ** rng.uniform(-0.15, 0.15))
            q0 = _rollout_q(model, B, rng)
            cfgs = [Configuration(model, q0[b]) for b in range(B)]
            targets = np.zeros((B, len(frames), 12))
            tasks = []
            for b, cfg in enumerate(cfgs):
                tl = []
                for i, (f, pc, oc, gain, lm) in enumerate(specs):
                    t = FrameTask(f, pc, oc, lm_damping=lm, gain=gain)
                    T = cfg.get_transform_frame_to_world(f) * exp6(0.03 * rng.normal(size=6))
                    t.set_target(T)
                    targets[b, i] = pose12(T)
                    tl.append(t)
                p = PostureTask(cost=cost)
                p.set_target(q0[b])
                tasks.append(tl + [p])
            bars = []
            if md:
                p0 = np.array([[c.get_transform_frame_to_world(f).translation for f in frames] for c in cfgs])
                bars = [PositionBarrier(frames[0], indices=[0, 1, 2], p_max=p0[:, 0].max(axis=0) + rng.uniform(0.0, 2e-3, size=3), gain=np.full(3, 50.0)),
                        PositionBarrier(frames[1], indices=[0, 1, 2], p_min=p0[:, 1].min(axis=0) - rng.uniform(0.0, 2e-3, size=3), gain=np.full(3, 50.0))]
            ro = DeviceRollout(s, model, q0, specs, dt, posture_cost=cost, fused="kernel", position_barriers=bars)
            try:
                ro.set_targets(targets)
                ro.step(integrate=False)
                s.sync()
                dq, st, _ = ro.last_step()
                path = np.asarray(ro.last_path)
                assert ro.fused == "kernel" and ro.md == md and ro.nv == 30
            finally:
                ro.free()
            batch = pack_configurations(cfgs, tasks, dt, barriers=bars or None, gpu_frame_tasks=False)
            assert batch.md == md
            pf = ps.ikbatch_form(batch)
            ref = c_oracle.solve_ik_batch(**pf)
            assert (st == 0).all() and (ref["status"] == 0).all(), (sd, st, ref["status"])
            assert np.isin(path, (0, 1, 2)).all(), (sd, path)
            P, _ = objective_ld(pf["J"], pf["e"], pf["cost"], pf["gain"], pf["lm"], pf["rows"], pf["damping"])
            kap = conditioning_estimate(P.astype(float))
            x, info = batch_minimiser(**{k: v for k, v in pf.items() if k != "meq"}, guesses=[ref["dq"], dq], meq=pf["meq"],
                                      floor_tol=np.where(kap < ps.ABS_BAR_COND, 0.1 * ps.TOL_EXACT, 10 * ps.TOL_EXACT))
            fallbacks += info["fallback"]
            for b in range(B):
                rec["band"].append(int(ps.band_of(kap[b:b + 1])[0])), rec["kappa"].append(float(kap[b])), rec["path"].append(int(path[b]))
                rec["err"].append(float(np.abs(dq[b] - x[b]).max())), rec["err_oracle"].append(float(np.abs(ref["dq"][b] - x[b]).max()))
                rec["xmax"].append(float(np.abs(x[b]).max())), rec["floor"].append(float(np.nan_to_num(info["floor"][b]))), rec["tag"].append((sd, b))
    rec = {k: np.array(v) if k != "tag" else v for k, v in rec.items()}
    seen = np.bincount(rec["band"][rec["band"] >= 0], minlength=len(ps.BANDS))
    lines = []
    names = ["tableau", "handover", "routed", "gi"]
    for i, nm in enumerate(ps.BAND_NAMES):
        m = rec["band"] == i
        sh = " ".join(f"{names[p]} {float((rec['path'][m] == p).mean()) if m.any() else 0.0:.3f}" for p in range(4))
        lines.append(f"rollout-30-{md}-32 {nm:11s} n={int(m.sum()):5d} worst|dq-x*|={rec['err'][m].max(initial=0.0):.2e} "
                     f"oracle={rec['err_oracle'][m].max(initial=0.0):.2e}  {sh}")
    print(f"\n{where} whole-step <30,{md},32>: reference handed {fallbacks} instances to exact_minimiser\n" + "\n".join(lines))
    assert (seen >= 1).all(), ("a band without an instance", seen)
    bar = ps.banded_bar(rec["kappa"], rec["xmax"], rec["err_oracle"], rec["floor"])
    bad = np.nonzero(~(rec["err"] <= bar))[0]
    assert not len(bad), [(rec["tag"][i], float(rec["kappa"][i]), int(rec["path"][i]), float(rec["err"][i]), float(rec["err_oracle"][i])) for i in bad[:8]]


def test_banded_families_reach_their_instantiations(emu, monkeypatch):
    """Each family of the bands reaches the instantiation kind it stands for, by the plan the library itself runs
    (pink_amd/csrc/host_plan.h, asked through the emulator's pinkhip_emu_plan_solve): box-only <NV,0,W> one lane per
    coordinate, eliminating <34,0,32>, dense rows <NV,MD,W> with MD > 0 and not the virtual-row kernel, virtual dense
    rows ik_sweepx.h.  An edit of the tables or of the rule that moves a family to another kernel fails here."""
    import ctypes

    from pink_amd._lib import Desc

    PLAN_SWEEP, PLAN_SWEEPX = 3, 4  # host_plan.h PlanKind
    emu.lib.pinkhip_emu_plan_solve.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(ctypes.c_int * 6)]

    def plan(nv, md, lead, solver):
        """(kind, NV, MD, W) for a batch of full rank with md dense rows under PINKHIP_SOLVER = solver (None: unset)"""
        if solver is None:
            monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
        else:
            monkeypatch.setenv("PINKHIP_SOLVER", solver)
        d = Desc(B=256, nv=nv, md=md, damping=1e-3, dt=0.01, max_iter=100, n_free_lead=lead)
        out = (ctypes.c_int * 6)()
        rc = emu.lib.pinkhip_emu_plan_solve(ctypes.byref(d), ctypes.byref(out))
        assert rc == 0, (rc, emu.lib.pinkhip_emu_last_error().decode())
        return tuple(out[:4])

    def select_sweep(nv, md, lead=0):  # the tableau instantiation with one lane per row that holds the problem, if any
        p = plan(nv, md, lead, "sweep")
        return p[1:] if p[0] == PLAN_SWEEP else None

    def prefer_sweepx(nv, md):  # is the kernel with virtual dense rows the one that runs it?
        return plan(nv, md, 0, None)[0] == PLAN_SWEEPX

    for fam, shapes in ps.BANDED_FAMILIES.items():
        for nv, md, neq, lead in shapes:
            rows = md + neq
            s_ = select_sweep(nv, rows, lead)
            if fam == "box":
                assert rows == 0 and s_ is not None and s_[1] == 0 and s_[0] <= s_[2], (fam, nv, s_)
            elif fam == "eliminating":
                assert rows == 0 and s_ == (34, 0, 32), (fam, nv, lead, s_)
            elif fam == "dense":
                assert rows > 0 and s_ is not None and s_[1] > 0 and not prefer_sweepx(nv, rows), (fam, nv, md, s_)
            elif fam == "virtual":
                assert rows > 0 and prefer_sweepx(nv, rows), (fam, nv, md)
            else:  # equalities: on one of the two tableau kernels
                assert neq > 0 and (prefer_sweepx(nv, rows) or s_ is not None), (fam, nv, md, neq)


# The worst draw of [1e6, 1e7) and [1e7, 1e8) per family on the MI355X (largest |dq - x*| / max(1, |x*|) under the default
# dispatch, batches of 256): (family, seed, instance).  Pinned so that the middle bands keep their hardest instances whatever
# the sample sizes of a run.
PINNED_WORST = [("box", 7100053, 41), ("box", 7100055, 163), ("eliminating", 7200014, 226), ("eliminating", 7200030, 205),
                ("dense", 7300058, 241), ("dense", 7300009, 9), ("virtual", 7400052, 180), ("virtual", 7400001, 62),
                ("equality", 7500032, 27), ("equality", 7500052, 2)]


@pytest.mark.parametrize("family,sd,inst", PINNED_WORST)
def test_worst_middle_band_draws(solver, family, sd, inst, monkeypatch):
    where, s = solver
    _, batch, pf, _ = ps.banded_draw(family, SEED0[family], sd, 256)
    one = batch.slice(inst, inst + 1)
    p1 = ps._take(pf, np.array([inst]))
    ref = c_oracle.solve_ik_batch(**p1, want_Hc=True)
    assert ref["status"][0] == 0
    kap = conditioning_estimate(ref["H"])
    assert 1e6 <= kap[0] < 1e8, kap
    for env, paths in ((None, (0, 1, 2)), ("sweep", (0, 1, 2)), ("packed", (3,))):
        if env is None:
            monkeypatch.delenv("PINKHIP_SOLVER", raising=False)
        else:
            monkeypatch.setenv("PINKHIP_SOLVER", env)
        out = s.solve(one)
        assert out.status[0] == 0 and int(out.path[0]) in paths, (env, out.status, out.path)
        x, info = batch_minimiser(p1["J"], p1["e"], p1["cost"], p1["gain"], p1["lm"], p1["rows"], p1["damping"], p1["G"], p1["h"],
                                  [ref["dq"], out.dq], meq=p1["meq"], floor_tol=10 * ps.TOL_EXACT)
        eg, eo = float(np.abs(out.dq[0] - x[0]).max()), float(np.abs(ref["dq"][0] - x[0]).max())
        xm = float(np.abs(x[0]).max())
        assert eg <= ps.banded_bar(kap[0], xm, eo, np.nan_to_num(info["floor"][0])), (family, sd, inst, env, float(kap[0]), eg, eo)
