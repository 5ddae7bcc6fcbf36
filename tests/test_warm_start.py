"""Warm start of the tableau solvers from a caller-supplied active set (include/pinkhip.h, pinkhip_warm): the entry points
pinkhip_solve_warm_device / pinkhip_rollout_step_warm_device, their emulator twins and the Python surface on top
(BatchSolver.solve(active_in=, return_active=), upload(warm=True), DeviceRollout(warm_start=True)).

The contract under test: the bytes of ``active_in`` are a hint -- whatever they hold, every instance is solved to the
minimiser the C oracle finds (pink/solve_ik.py:206-275 through Goldfarb-Idnani), an exact set costs no exchange, and
``active_out`` is the active set at the returned point (zeros for a failed instance).  Emulator here, MI355X under -m gpu.

Shapes: nv = 12 (four groups per wave, padding lanes 12..15), nv = 30 (two groups per wave: the ballot split), nv = 33 with
declared free leading coordinates (front coordinates eliminated: the index offset; one instance bounds a leading coordinate
and is routed), nv = 50 (one group per wave).  B = 67 on the emulator (odd: the surplus group of the last wave runs),
4 096 on the GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle
from oracle.parity_report import active_sets
from pink_amd import Configuration, build_chain, synthetic
from pink_amd._lib import ABI_SYMBOLS, Desc, PackedArgs, PinkHipError, Problem, Result, RolloutStep, Warm
from pink_amd.batch import DenseTaskTerm, DiagonalTaskTerm, pack_terms
from pink_amd.lie import SE3, exp3
from pink_amd.rollout import DeviceRollout, pose12

from tests.cases import config_case, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["nv12", "nv30", "nv33", "nv50"]
STARTS = ["exact", "zeros", "all_fixed", "random_bytes", "exact_10pct_redrawn"]


class EmuWarm:
    """The ``emu`` fixture's object plus the two warm-start methods of BatchSolver's raw interface, on host memory."""

    def __init__(self, emu):
        self._emu = emu
        lib = emu.lib
        lib.pinkhip_emu_solve_warm_host.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Problem), ctypes.POINTER(Result), ctypes.POINTER(Warm)]
        lib.pinkhip_emu_warm_last_error.restype = ctypes.c_char_p
        lib.pinkhip_emu_rollout_step_warm.argtypes = [ctypes.POINTER(Desc), ctypes.c_void_p, ctypes.POINTER(RolloutStep), ctypes.POINTER(Warm)]

    def __getattr__(self, name):
        return getattr(self._emu, name)

    def _check(self, rc):
        if rc != 0:
            raise PinkHipError(rc, self._emu.lib.pinkhip_emu_warm_last_error().decode())

    def solve_warm_raw(self, desc, problem, result, warm):
        self._check(self._emu.lib.pinkhip_emu_solve_warm_host(ctypes.byref(desc), ctypes.byref(problem), ctypes.byref(result), ctypes.byref(warm)))

    def rollout_step_warm(self, desc, model, args, warm):
        self._check(self._emu.lib.pinkhip_emu_rollout_step_warm(ctypes.byref(desc), model, ctypes.byref(args), ctypes.byref(warm)))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    if request.param == "emu":
        return EmuWarm(request.getfixturevalue("emu"))
    return request.getfixturevalue("gpu_solver")


def _on_gpu(api):
    return not isinstance(api, EmuWarm)


def _B(api):
    return 4096 if _on_gpu(api) else 67


# ------------------------------------------------------------------------------------------------ problems, built once
_CASES = {}


def _case(shape, B):
    """(packed batch, n_free_lead to declare or None, oracle result) of one shape; the oracle runs once per (shape, B)."""
    key = (shape, B)
    if key in _CASES:
        return _CASES[key]
    lead = None
    if shape == "nv12":
        batch, pf = random_case(12, B, 11)
    elif shape == "nv30":
        batch, pf = config_case("draco3", "tight", "dense", B)
    elif shape == "nv50":
        batch, pf = random_case(50, B, 13)
    elif shape == "nv33":
        # a free-flyer whose six root coordinates carry no bound, declared (tests/test_round6_elimination.py) -- except that
        # instance 3 bounds coordinate 1 after all: the kernel sends it to the Goldfarb-Idnani code (PATH_ROUTED)
        name = "freeflyer_nv33"
        synthetic.CONFIGS[name] = dict(synthetic.CONFIGS["draco3_freeflyer"], nv=33, config_id=73)
        terms = synthetic.make_terms(name, B, bounds="tight")
        batch, pf = synthetic.pack(terms), synthetic.pink_form(terms)
        batch.lb[3, 1], batch.ub[3, 1] = -1e-4, 2e-4
        rows = np.zeros((B, 2, 33))
        rows[:, 0, 1], rows[:, 1, 1] = 1.0, -1.0
        h = np.full((B, 2), 1e30)
        h[3] = [2e-4, 1e-4]
        pf["G"] = np.ascontiguousarray(np.concatenate([pf["G"], rows], axis=1))
        pf["h"] = np.ascontiguousarray(np.concatenate([pf["h"], h], axis=1))
        lead = 6
    ref = c_oracle.solve_ik_batch(**pf)
    assert (ref["status"] == 0).all(), "an infeasible draw would hide a failure"
    _CASES[key] = (batch, lead, ref)
    return _CASES[key]


class Out:
    pass


def warm_solve(api, batch, active_in=None, max_iter=0, lead=None, in_place=False, want_out=True):
    """One pinkhip_solve_warm_device call through the raw interface (device memory on the GPU, host memory on the emulator)."""
    a = PackedArgs(batch, max_iter)
    if lead is not None:
        a.desc.n_free_lead = lead
    B, nv = batch.B, batch.nv
    ptrs = {name: api.alloc(max(arr.nbytes, 8)) for name, arr in a.streams()}
    for name, arr in a.streams():
        api.put(ptrs[name], arr)
    p = Problem()
    for name in ("J", "e", "cost", "lb", "ub", "Gd", "hd", "c_extra"):
        setattr(p, name, ptrs.get(name))
    d_dq, d_st, d_it = api.alloc(8 * B * nv), api.alloc(4 * B), api.alloc(4 * B)
    d_in, d_out = api.alloc(B * nv), api.alloc(B * nv)
    sentinel = np.full((B, nv), 77, dtype=np.uint8)
    api.put(d_out, sentinel)
    api.put(d_dq, np.full((B, nv), -7.0))
    api.put(d_st, np.full(B, -9, dtype=np.int32))
    api.put(d_it, np.zeros(B, dtype=np.int32))
    if active_in is not None:
        api.put(d_in, np.ascontiguousarray(active_in))
    r = Result()
    r.dq, r.status, r.iters = d_dq, d_st, d_it
    w = Warm()
    w.active_in = d_in if active_in is not None else None
    w.active_out = (d_in if in_place else d_out) if want_out else None
    o = Out()
    o.code = 0
    try:
        api.solve_warm_raw(a.desc, p, r, w)
    except PinkHipError as exc:
        o.code = exc.code
    api.sync()
    o.dq, o.status, raw, o.active = np.zeros((B, nv)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, nv), np.uint8)
    api.get(o.dq, d_dq), api.get(o.status, d_st), api.get(raw, d_it), api.get(o.active, d_in if in_place else d_out)
    o.iters, o.path = raw & 0xFFFFFF, raw >> 24
    for ptr in list(ptrs.values()) + [d_dq, d_st, d_it, d_in, d_out]:
        api.release(ptr)
    return o


def _starts(batch, exact, seed):
    rng = np.random.default_rng(seed)
    lb, ub = batch.lb, batch.ub
    redrawn = exact.copy()
    pick = rng.random(size=exact.shape) < 0.10
    redrawn[pick] = rng.integers(0, 3, size=int(pick.sum()), dtype=np.uint8)
    return dict(
        exact=exact,
        zeros=np.zeros_like(exact),
        all_fixed=np.where(np.isfinite(lb), 1, np.where(np.isfinite(ub), 2, 0)).astype(np.uint8),
        random_bytes=rng.integers(0, 256, size=exact.shape, dtype=np.uint8),
        exact_10pct_redrawn=redrawn,
    )


_COLD = {}


def _cold(api, shape):
    """The cold call of a shape (active_in = NULL: the kernel's own start), once per backend."""
    key = (shape, _on_gpu(api))
    if key not in _COLD:
        batch, lead, ref = _case(shape, _B(api))
        _COLD[key] = warm_solve(api, batch, None, lead=lead)
    return _COLD[key]


# ------------------------------------------------------------------------------------------------ T1
def test_symbols_in_header_binding_and_library(built):
    header = open(os.path.join(ROOT, "include", "pinkhip.h")).read()
    from pink_amd import _lib

    for name in ("pinkhip_solve_warm_device", "pinkhip_rollout_step_warm_device"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in ABI_SYMBOLS
        assert hasattr(_lib.load_library(), name)
    assert re.search(r"#define PINKHIP_HAS_WARM_START 1\b", header)
    assert _lib.load_library().pinkhip_version() == 112
    assert ctypes.sizeof(Warm) == 16
    emu = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libpinkemu.so"))
    assert hasattr(emu, "pinkhip_emu_solve_warm_host") and hasattr(emu, "pinkhip_emu_rollout_step_warm")


# ------------------------------------------------------------------------------------------------ T2
@pytest.mark.parametrize("shape", SHAPES)
def test_any_start_same_minimiser(api, shape):
    batch, lead, ref = _case(shape, _B(api))
    cold = _cold(api, shape)
    assert cold.code == 0 and np.array_equal(cold.status, ref["status"])
    print(f"{shape} cold: max|dq - dq_oracle| = {np.abs(cold.dq - ref['dq']).max():.3e}")
    assert np.abs(cold.dq - ref["dq"]).max() <= 1e-10
    if shape == "nv33":
        assert cold.path[3] == 2 and (np.delete(cold.path, 3) == 0).all()  # routed by its bounded leading coordinate
    for k, (name, start) in enumerate(_starts(batch, cold.active, 100).items()):
        out = warm_solve(api, batch, start, lead=lead)
        err = np.abs(out.dq - ref["dq"]).max()
        print(f"{shape} {name}: max|dq - dq_oracle| = {err:.3e}, exchanges {out.iters.sum()} (cold {cold.iters.sum()})")
        assert out.code == 0 and np.array_equal(out.status, ref["status"]), name
        assert err <= 1e-10, (name, err)


@pytest.mark.gpu
def test_batch_solver_keywords(gpu_solver):
    """BatchSolver.solve(active_in=, return_active=) and upload(warm=True) / solve_device / download (the emulator has no
    BatchSolver: its half of this surface is the raw interface every other test here goes through)."""
    api = gpu_solver
    batch, lead, ref = _case("nv30", _B(api))
    first = api.solve(batch, return_active=True)
    assert first.active is not None and first.active.dtype == np.uint8 and first.active.shape == (batch.B, batch.nv)
    again = api.solve(batch, active_in=first.active)
    assert np.abs(again.dq - ref["dq"]).max() <= 1e-10 and np.array_equal(again.active, first.active)
    assert again.iters[again.path == 0].sum() <= 0.01 * first.iters[first.path == 0].sum()
    assert api.solve(batch).active is None
    with pytest.raises(ValueError):
        api.solve(batch, active_in=first.active[:, :-1])
    with pytest.raises(ValueError):
        api.solve(batch, active_in=first.active.astype(np.int32))
    dev = api.upload(batch, warm=True)
    api.solve_device(dev)
    r1 = api.download(dev)
    api.solve_device(dev)  # (from the set the first pass left in d_active)
    r2 = api.download(dev)
    dev.free()
    assert np.array_equal(r1.active, first.active) and np.array_equal(r2.active, first.active)
    assert np.abs(r2.dq - ref["dq"]).max() <= 1e-10 and r2.iters[r2.path == 0].sum() <= 0.01 * r1.iters[r1.path == 0].sum()
    with pytest.raises(PinkHipError) as exc:
        api.solve(random_case(12, 8, 5, md=2)[0], return_active=True)
    assert exc.value.code == -5


# ------------------------------------------------------------------------------------------------ T3
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_set_costs_no_exchange(api, shape):
    batch, lead, ref = _case(shape, _B(api))
    cold = _cold(api, shape)
    out = warm_solve(api, batch, cold.active, lead=lead)
    tab = (cold.path == 0) & (out.path == 0)
    cold_total, warm_total = int(cold.iters[tab].sum()), int(out.iters[tab].sum())
    print(f"{shape}: exchanges cold {cold_total}, from the exact set {warm_total}, instances with any {int((out.iters[tab] > 0).sum())}")
    assert tab.sum() >= batch.B - 1 and cold_total > 0
    assert warm_total <= 0.01 * cold_total


# ------------------------------------------------------------------------------------------------ T4
def _oracle_set(dq, lb, ub):
    at_lb, at_ub, _ = active_sets(dq, lb, ub)
    return np.where(at_lb, 1, np.where(at_ub, 2, 0)).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_active_out_is_the_active_set(api, shape):
    batch, lead, ref = _case(shape, _B(api))
    cold = _cold(api, shape)
    want = _oracle_set(ref["dq"], batch.lb, batch.ub)
    same = (cold.active == want).all(axis=1)
    print(f"{shape}: active_out equals the oracle's set in {same.mean():.5f} of {batch.B} instances")
    assert same.mean() >= 0.999
    assert cold.active.max() <= 2 and cold.active.any()
    if shape == "nv33":  # the routed instance: the working set of the Goldfarb-Idnani code that solved it
        assert cold.path[3] == 2 and same[3] and cold.active[3, 1] == want[3, 1]


def _weak_case(B):
    """Stacks that only `damping`-sized terms make positive definite (tests/test_round4.py: a posture task of negligible
    cost under six task rows on twelve coordinates): cond(H) beyond the tableau's routing threshold -- the instances leave
    the tableau (PATH_ROUTED / PATH_HANDOVER)."""
    rng = np.random.default_rng(4)
    nv = 12
    J = rng.normal(0, 0.5, size=(B, 6, nv))
    e = 0.1 * rng.normal(size=(B, 6))
    ep = 0.1 * rng.normal(size=(B, nv))
    lb, ub = -0.05 * np.ones((B, nv)), 0.05 * np.ones((B, nv))
    batch = pack_terms(nv, [DenseTaskTerm(J=J, e=e, cost=1.0), DiagonalTaskTerm(col0=0, e=ep, cost=1e-5)], 5e-3, 1e-12, boxes=[(lb, ub)], batch_size=B)
    eye = np.broadcast_to(np.eye(nv), (B, nv, nv))
    pf = dict(J=np.ascontiguousarray(np.concatenate([J, eye], axis=1)), e=np.concatenate([e, ep], axis=1), cost=np.r_[np.ones(6), np.full(nv, 1e-5)],
              gain=np.array([1.0, 1.0]), lm=np.array([0.0, 0.0]), rows=np.array([0, 6, 6 + nv], np.int32), damping=1e-12,
              G=np.ascontiguousarray(np.concatenate([eye, -eye], axis=1)), h=np.full((B, 2 * nv), 0.05))
    return batch, pf


def test_active_out_of_instances_that_left_the_tableau(api):
    B = _B(api)
    key = ("weak", B)
    if key not in _CASES:
        batch, pf = _weak_case(B)
        _CASES[key] = (batch, None, c_oracle.solve_ik_batch(**pf))
    batch, _, ref = _CASES[key]
    assert (ref["status"] == 0).all()
    out = warm_solve(api, batch, None)
    off = out.path != 0
    print(f"weak stack: paths {np.bincount(out.path, minlength=4)[:4]}")
    assert out.code == 0 and (out.status == 0).all() and np.isin(out.path, (0, 1, 2)).all()
    assert off.sum() >= B // 4, "the batch was meant to leave the tableau"
    want = _oracle_set(ref["dq"], batch.lb, batch.ub)
    same = (out.active == want).all(axis=1)
    print(f"weak stack: active_out equals the oracle's set in {same[off].mean():.5f} of the {off.sum()} instances off the tableau, "
          f"{same[~off].mean() if (~off).any() else 1.0:.5f} of the others")
    assert same[off].mean() >= 0.999
    assert (~off).sum() == 0 or same[~off].mean() >= 0.999
    # ... and seeds the next call like any other set
    again = warm_solve(api, batch, out.active)
    assert again.code == 0 and (again.status == 0).all()
    assert np.abs(again.dq - out.dq).max() <= 1e-8  # (weakly determined minimisers: the project's contract, test_round4.py)


# ------------------------------------------------------------------------------------------------ T5
def test_failures_do_not_seed(api):
    batch, lead, ref = _case("nv30", _B(api))
    cold = _cold(api, "nv30")
    capped = warm_solve(api, batch, None, max_iter=1)
    failed = capped.status != 0
    assert capped.code == 0 and failed.any() and (capped.status[failed] == 1).all()
    assert not capped.active[failed].any()
    assert np.array_equal(capped.active[~failed], cold.active[~failed])
    import dataclasses

    empty = dataclasses.replace(batch, lb=batch.lb.copy(), ub=batch.ub.copy())
    empty.lb[5, 9], empty.ub[5, 9] = 0.01, -0.01
    out = warm_solve(api, empty, cold.active)
    assert out.code == 0 and out.status[5] == 2 and (np.delete(out.status, 5) == 0).all()
    assert not out.active[5].any()
    assert np.array_equal(np.delete(out.active, 5, axis=0), np.delete(cold.active, 5, axis=0))


# ------------------------------------------------------------------------------------------------ T6
def _deficient(B):
    rng = np.random.default_rng(6)
    nv = 12
    box = [(-0.05 * np.ones((B, nv)), 0.05 * np.ones((B, nv)))]
    return pack_terms(nv, [DenseTaskTerm(J=rng.normal(0, 0.5, size=(B, 6, nv)), e=0.1 * rng.normal(size=(B, 6)), cost=1.0)], 5e-3, 1e-12, boxes=box, batch_size=B)


def _assert_refused(out):
    assert out.code == -5
    assert (out.dq == -7.0).all() and (out.status == -9).all() and (out.active == 77).all()


def test_refusals_touch_nothing(api):
    B = 9
    _assert_refused(warm_solve(api, random_case(12, B, 5, md=2)[0], np.zeros((B, 12), np.uint8)))
    _assert_refused(warm_solve(api, _deficient(B), np.zeros((B, 12), np.uint8)))


def _child_packed(backend):
    """Runs in a fresh process with PINKHIP_SOLVER=packed: prints the code of the warm call and whether it left its buffers."""
    if backend == "emu":
        from tests.conftest import EmuSolver

        s = EmuWarm(EmuSolver(ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libpinkemu.so"))))
    else:
        from pink_amd.batch_solver import BatchSolver

        s = BatchSolver(0)
    out = warm_solve(s, random_case(12, 9, 5)[0], np.zeros((9, 12), np.uint8))
    print("CHILD", out.code, int((out.dq == -7.0).all() and (out.status == -9).all() and (out.active == 77).all()))


def test_forced_packed_solver_is_refused(api, built):
    backend = "gpu" if _on_gpu(api) else "emu"
    code = f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_warm_start as t; t._child_packed({backend!r})"
    env = dict(os.environ, PINKHIP_SOLVER="packed")
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "CHILD -5 1" in run.stdout, run.stdout


# ------------------------------------------------------------------------------------------------ T7
@pytest.mark.parametrize("shape", ["nv12", "nv33"])
def test_in_place_equals_two_arrays(api, shape):
    batch, lead, ref = _case(shape, _B(api))
    start = _starts(batch, _cold(api, shape).active, 7)["exact_10pct_redrawn"]
    two = warm_solve(api, batch, start, lead=lead)
    one = warm_solve(api, batch, start, lead=lead, in_place=True)
    assert one.code == 0 and two.code == 0
    assert np.array_equal(one.dq, two.dq) and np.array_equal(one.status, two.status)
    assert np.array_equal(one.iters, two.iters) and np.array_equal(one.path, two.path) and np.array_equal(one.active, two.active)


# ------------------------------------------------------------------------------------------------ T8 - T10
def _loop_models():
    arm12 = build_chain(12, seed=5)
    humanoid = build_chain(9, free_flyer=True, seed=3)
    humanoid.add_frame("mid", 4, SE3(np.eye(3), [0.05, 0.0, 0.1]))
    big = build_chain(24, free_flyer=True, seed=2)
    return [(arm12, ["tool0", "joint_6"]), (humanoid, ["tool0", "mid"]), (big, ["tool0", "joint_12"])]


MOVE = 0.3  # metres: far enough that velocity / configuration bounds stay active for several steps


def _loop(api, which, warm, steps=8, garbage_after=None):
    from tests.test_rollout import _random_q

    model, frames = _loop_models()[which]
    rng = np.random.default_rng(80 + which)
    B = 5
    q0 = _random_q(model, B, rng) * 0.6 + 0.4 * np.tile(model.neutral(), (B, 1))
    if model.nq != model.nv:
        q0[:, 3:7] /= np.linalg.norm(q0[:, 3:7], axis=1, keepdims=True)
    specs = [(f, 1.0, 0.5, 0.9, 1e-3) for f in frames]
    targets = np.zeros((B, len(frames), 12))
    for b in range(B):
        cfg = Configuration(model, q0[b])
        for i, f in enumerate(frames):
            d = rng.normal(size=3)
            targets[b, i] = pose12(cfg.get_transform_frame_to_world(f) * SE3(exp3(0.3 * rng.normal(size=3)), MOVE * d / np.linalg.norm(d)))
    ro = DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=5e-2, fused="kernel", warm_start=warm)
    ro.set_targets(targets)
    hist = []
    for k in range(steps):
        ro.step()
        api.sync()
        dq, st, it = ro.last_step()
        hist.append((dq.copy(), st.copy(), it.copy(), ro.configurations().copy()))
        if warm and garbage_after is not None and k + 1 == garbage_after:
            ro.set_active(np.random.default_rng(3).integers(0, 256, size=(B, model.nv), dtype=np.uint8))
    assert ro.fused == "kernel"
    extra = None
    if warm:
        act = ro.last_active()
        assert act.shape == (B, model.nv) and act.max() <= 2
        ro.reset(q0)
        extra = (act, ro.last_active())
    ro.free()
    return hist, extra


_LOOPS = {}


def _cold_loop(api, which):
    key = (which, _on_gpu(api))
    if key not in _LOOPS:
        _LOOPS[key] = _loop(api, which, False)[0]
    return _LOOPS[key]


def _assert_same_trajectory(cold, warm):
    for (dq_a, st_a, _, q_a), (dq_b, st_b, _, q_b) in zip(cold, warm):
        assert np.array_equal(st_a, st_b) and (st_a == 0).all()
        assert np.abs(dq_a - dq_b).max() < 1e-11 and np.abs(q_a - q_b).max() < 1e-11


@pytest.mark.parametrize("which", [0, 1, 2])
def test_closed_loop_warm_equals_cold_with_fewer_exchanges(api, which):
    cold = _cold_loop(api, which)
    warm, (act, after_reset) = _loop(api, which, True)
    _assert_same_trajectory(cold, warm)
    cold_it = np.array([h[2] for h in cold[1:]])
    warm_it = np.array([h[2] for h in warm[1:]])
    print(f"model {which}: exchanges over steps 2..8 cold {cold_it.sum()} (mean {cold_it.mean():.2f}), warm {warm_it.sum()}, "
          f"ratio {warm_it.sum() / max(cold_it.sum(), 1):.3f}")
    assert cold_it.mean() >= 3.0, "a loop without active bounds shows nothing: enlarge the move"
    assert warm_it.sum() < cold_it.sum()
    assert act.any() and not after_reset.any()


def test_garbage_state_mid_loop(api):
    cold = _cold_loop(api, 1)
    warm, (act, after_reset) = _loop(api, 1, True, garbage_after=3)
    _assert_same_trajectory(cold, warm)
    assert not after_reset.any()


def test_construction_errors(api):
    from pink_amd.barriers import PositionBarrier

    model, frames = _loop_models()[0]
    q0 = np.tile(model.neutral(), (2, 1))
    specs = [(f, 1.0, 0.5, 0.9, 1e-3) for f in frames]
    with pytest.raises(ValueError, match="warm_start"):
        DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=5e-2, fused=True, warm_start=True)
    bar = PositionBarrier("tool0", indices=[2], p_max=np.array([5.0]), gain=np.array([50.0]), safe_displacement_gain=1.0)
    with pytest.raises(ValueError, match="warm_start"):
        DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=5e-2, fused="kernel", position_barriers=[bar], warm_start=True)
    ro = DeviceRollout(api, model, q0, specs, 5e-3, posture_cost=5e-2, fused="kernel")
    with pytest.raises(ValueError):
        ro.last_active()
    ro.free()


# ------------------------------------------------------------------------------------------------ T11
def test_warm_objects_keep_the_tableau_in_registers(built):
    """The rule of tests/test_abi.py::test_tableau_rows_stay_in_registers over the warm-start objects: a private segment
    beyond four bytes per spilled register stays under 128 bytes (a tableau tuple in scratch memory shows as hundreds)."""
    import glob

    build = os.path.join(ROOT, "pink_amd", "csrc", "build")
    objs = sorted(glob.glob(os.path.join(build, "wsweep_*.o")) + glob.glob(os.path.join(build, "wrollout_*.o")))
    assert len(objs) == 9
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_meta.py")] + objs, capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-objdump / llvm-readelf not available: " + out.stderr[-200:])
    print(out.stdout)
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ik_") and "_warm_kernel" in ln]
    assert len(rows) == 9, out.stdout[-2000:]
    excess = lambda f: int(f[-2]) - 4 * int(f[-4])  # noqa: E731  (columns: ... vspill sspill scratch lds)
    worst = max(rows, key=excess)
    assert excess(worst) < 128, " ".join(worst)
