"""The stack-only kernels (ik_stack_mfma_kernel<1..4>, ik_stack_staged_kernel<3, 4>, ik_stack_small_kernel<1, 4>:
``build_ik``'s P, q) against oracle/exact_stack.py -- the definition in exact rational arithmetic -- on the CPU wave
emulator and on the GPU, at every edge of their loops: more than 32 and more than 128 dense rows at nv > 8 (J requested
again per 32-row pass and per row of tiles, the second 128-row coefficient table), the staged / direct decision at
nv > 32 (even and odd Kd nv, Kd around 32, a J stream that starts 8 bytes off a 16-byte boundary), both packings of the
nv <= 8 kernel with their tail waves, Kd = 0, the barrier regulariser and c_extra.

THE BAR IS DERIVED, NOT MEASURED.  An entry is a sum of n = Kd + n_diag terms: Kd dense-row products, plus on the
diagonal / in c the n_diag terms that touch it (a diagonal task's w^2 or gain w^2 e, mu_t of each task with LM damping,
the damping, each barrier's regulariser, c_extra).  Summed in any order, with or without FMA, each product with at most
three extra roundings of its own (w w, . J, . gain), such a sum is within (n / 2 + 2) 2^-52 S <= (n + 8) 2^-52 S of the
exact value, S being the same sum over the absolute values of the products (``ExactStack.ratios`` decides it in exact
arithmetic).  mu_t counts as ONE term although it is a sum over its task's rows: all its terms are positive, its own
summation error (rows_t / 2 + 3) 2^-52 mu_t stays under the bar wherever the LM rows are fewer than 2 (Kd + n_diag) + 10
(every shape here but Kd = 0 at nv = 30 and 50, where the worst case of round-off would need 20 units against a bar of
11 or 12 and what is observed is 1.4).  No absolute floor, no max|H|: where S is zero the entry must be exactly zero.

Inputs that make it bite: row costs log-uniform over 1e-2 .. 1e2 (per instance for odd B), gains in 0.3 .. 1, LM
damping on two of three dense tasks and on one diagonal task, a diagonal task from column nv // 3 on (across the tile
boundaries at 16 and 32), damping 1e-9.

PINK_STACK_EXACT_RATIOS=<file>: the worst ratios |error| / (2^-52 S) of this run, per backend and kernel family, are
written there as JSON (profiles/stack_exact.json holds the ones measured)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from oracle.exact_stack import exact_stack
from pink_amd._lib import PackedArgs
from pink_amd.batch import BarrierTerm, DenseTaskTerm, DiagonalTaskTerm, pack_terms

RATIOS = {}
GUARD = 64  # doubles of sentinel in front of and behind H_out / c_out
SENTINEL = -1.2345e300


# ---- backends ---------------------------------------------------------------------------------------------------------
class _Emu:
    name = "emu"

    def __init__(self, solver):
        self.s = solver

    def four_tiles(self, B):
        return B % 2 == 1  # (emu/emu_kernels.cpp: the emulator picks the four-tile packing by B % 2)

    def stack(self, batch):
        return self.s.stack(batch)

    def stack_raw(self, batch, j_offset=0, guard=0):
        """``stack`` on buffers of the test's own: the J stream starts ``8 j_offset`` bytes behind a 16-byte boundary,
        H_out / c_out lie ``guard`` doubles inside larger arrays (returned whole)."""
        a = PackedArgs(batch)
        p = a.host_problem()
        jbuf = np.zeros(a.J.size + 4)
        s0 = (j_offset - jbuf.ctypes.data // 8) % 2 + 2  # (jbuf + 8 s0) % 16 == 8 j_offset
        jbuf[s0:s0 + a.J.size] = a.J.ravel()
        p.J = jbuf.ctypes.data + 8 * s0
        assert p.J % 16 == 8 * j_offset
        nH, nc = batch.B * batch.nv * batch.nv, batch.B * batch.nv
        Hbuf, cbuf = _guarded(nH, guard), _guarded(nc, guard)
        rc = self.s.lib.pinkhip_emu_stack_host(ctypes.byref(a.desc), ctypes.byref(p), Hbuf.ctypes.data + 8 * guard, cbuf.ctypes.data + 8 * guard)
        assert rc == 0, self.s.lib.pinkhip_emu_last_error().decode()
        return Hbuf, cbuf


class _Gpu:
    name = "gpu"

    def __init__(self, solver):
        self.s = solver

    def four_tiles(self, B):
        return B >= 65536  # (pinkhip.hip: launch)

    def stack(self, batch):
        return self.s.stack(batch)

    def stack_raw(self, batch, j_offset=0, guard=0):
        s = self.s
        dev = s.upload(batch)
        nH, nc = batch.B * batch.nv * batch.nv, batch.B * batch.nv
        Hbuf, cbuf = _guarded(nH, guard), _guarded(nc, guard)
        dJ, dH, dc = s.alloc(dev.args.J.nbytes + 16), s.alloc(Hbuf.nbytes), s.alloc(cbuf.nbytes)
        try:
            assert dJ % 16 == 0
            if dev.args.J.size:
                s.put(dJ + 8 * j_offset, dev.args.J)
            dev.problem.J = dJ + 8 * j_offset
            s.put(dH, Hbuf)
            s.put(dc, cbuf)
            dev.d_H, dev.d_c = dH + 8 * guard, dc + 8 * guard
            s.stack_device(dev)
            s.sync()
            s.get(Hbuf, dH)
            s.get(cbuf, dc)
        finally:
            dev.d_H = dev.d_c = None  # (addresses inside dH / dc: released below, not by dev.free())
            dev.free()
            for ptr in (dJ, dH, dc):
                s.release(ptr)
        return Hbuf, cbuf


def _guarded(n, guard):
    buf = np.full(n + 2 * guard, np.nan)  # interior: NaN until written
    buf[:guard] = buf[guard + n:] = SENTINEL
    return buf


def _interior(batch, Hbuf, cbuf, guard):
    B, nv = batch.B, batch.nv
    return Hbuf[guard:guard + B * nv * nv].reshape(B, nv, nv), cbuf[guard:guard + B * nv].reshape(B, nv)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return _Emu(request.getfixturevalue("emu")) if request.param == "emu" else _Gpu(request.getfixturevalue("gpu_solver"))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("PINK_STACK_EXACT_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump({k: {fam: {q: float("%.3g" % v) for q, v in sorted(d.items())} for fam, d in sorted(fams.items())} for k, fams in sorted(RATIOS.items())},
                      f, indent=1)
            f.write("\n")


# ---- inputs -----------------------------------------------------------------------------------------------------------
def make_batch(nv, Kd, B, seed, barrier=False, batched=None):
    """Up to three dense tasks of Kd rows in all (LM damping 0.2 / 0 / 0.05), a diagonal task from column nv // 3 to the
    end (LM damping 0.1) and one over the first half; costs per instance for odd B (``batched``: override)."""
    rng = np.random.default_rng(seed)
    batched = (B % 2 == 1) if batched is None else batched
    cost = lambda k: 10.0 ** rng.uniform(-2.0, 2.0, size=(B, k) if batched else k)  # noqa: E731
    gain = lambda: float(rng.uniform(0.3, 1.0))  # noqa: E731
    tasks = []
    nt = min(3, Kd)
    for t in range(nt):
        k = Kd * (t + 1) // nt - Kd * t // nt
        tasks.append(DenseTaskTerm(J=rng.normal(0, 0.5, size=(B, k, nv)), e=0.1 * rng.normal(size=(B, k)), cost=cost(k), gain=gain(),
                                   lm_damping=(0.2, 0.0, 0.05)[t]))
    col0, k2 = nv // 3, max(1, nv // 2)
    tasks.append(DiagonalTaskTerm(col0=col0, e=rng.uniform(-0.5, 0.5, size=(B, nv - col0)), cost=cost(nv - col0), gain=gain(), lm_damping=0.1))
    tasks.append(DiagonalTaskTerm(col0=0, e=rng.uniform(-0.5, 0.5, size=(B, k2)), cost=cost(k2), gain=gain()))
    barriers = []
    if barrier:  # one barrier of two rows with a safe displacement: the regulariser on the diagonal of H, c_extra in c
        barriers.append(BarrierTerm(J_h=rng.normal(0, 0.3, size=(B, 2, nv)), h=rng.uniform(0.0, 0.05, size=(B, 2)), gain=100.0,
                                    safe_displacement_gain=2.5, safe_displacement=0.01 * rng.normal(size=(B, nv))))
    batch = pack_terms(nv, tasks, 0.01, 1e-9, barriers=barriers, batch_size=B)
    assert batch.Kd == Kd and (batch.cost.ndim == 2) == batched and (batch.c_extra is not None) == barrier
    return batch


@functools.lru_cache(maxsize=None)
def _case(nv, Kd, B, barrier=False, batched=None):
    return make_batch(nv, Kd, B, 1000 * nv + Kd + 7 * B + (500000 if barrier else 0), barrier, batched)


@functools.lru_cache(maxsize=None)
def _exact(key, b):
    """Exact H, c of instance ``b`` of the cached batch ``key`` (computed once, shared by the backends)."""
    return exact_stack(_BATCHES[key], b)


_BATCHES = {}


def _register(key, batch):
    _BATCHES.setdefault(key, batch)
    return _BATCHES[key]


def family(backend, batch, aligned=True):
    """Which kernel the launch rule picks (pink_amd/csrc/host_plan.h: plan_stack; ik_stack_mfma.h: stack_staged_ok)."""
    nv, Kd, B = batch.nv, batch.Kd, batch.B
    if nv <= 8 and not len(batch.barrier_safe_gain):
        return "small_tp4" if backend.four_tiles(B) else "small_tp1"
    nt = (nv + 15) // 16
    staged = nv > 32 and (Kd * nv) % 2 == 0 and 0 < Kd <= 32 and aligned
    return f"{'staged' if staged else 'direct'}_nt{nt}"


def _note(backend, fam, rH, rc):
    d = RATIOS.setdefault(backend.name, {}).setdefault(fam, {"H": 0.0, "c": 0.0})
    d["H"], d["c"] = max(d["H"], float(rH.max(initial=0.0))), max(d["c"], float(rc.max(initial=0.0)))


def check_exact(backend, key, batch, H, c, instances=None, fam=None, aligned=True):
    """Every entry of H[b], c[b] within (n + 8) 2^-52 S of the exact value; returns the worst ratios to 2^-52 S."""
    fam = fam or family(backend, batch, aligned)
    batch = _register(key, batch)
    worst = [0.0, 0.0]
    for b in (range(batch.B) if instances is None else instances):
        ex = _exact(key, int(b))
        rH, bH, rc, bc = ex.ratios(H[b], c[b])
        _note(backend, fam, rH, rc)
        worst = [max(worst[0], float(rH.max())), max(worst[1], float(rc.max()))]
        print(f"{backend.name} {fam} nv={batch.nv} Kd={batch.Kd} B={batch.B} b={b}: worst |err| / (2^-52 S): H {rH.max():.3g} (bar {ex.nH[0][0] + 8}), c {rc.max():.3g} (bar {ex.nc[0] + 8})")
        assert not bH.any(), (fam, batch.nv, batch.Kd, batch.B, int(b), "H beyond the bar at", np.argwhere(bH)[:8].tolist(), rH[bH][:8])
        assert not bc.any(), (fam, batch.nv, batch.Kd, batch.B, int(b), "c beyond the bar at", np.nonzero(bc)[0][:8].tolist(), rc[bc][:8])
    return worst


# ---- the shape grid ---------------------------------------------------------------------------------------------------
# (nv, Kd, family the rule must pick): the smallest shapes at which each path exists
MFMA_GRID = [
    (9, 33, "direct_nt1"), (16, 40, "direct_nt1"), (16, 129, "direct_nt1"),
    (17, 32, "direct_nt2"), (17, 33, "direct_nt2"), (30, 36, "direct_nt2"), (30, 129, "direct_nt2"), (32, 130, "direct_nt2"),
    (33, 5, "direct_nt3"),  # odd Kd nv: direct
    (33, 36, "direct_nt3"),  # not one pass
    (34, 31, "staged_nt3"), (48, 32, "staged_nt3"),  # (48, 32): the largest flat stream of NT = 3
    (48, 33, "direct_nt3"),
    (50, 24, "staged_nt4"), (50, 32, "staged_nt4"),
    (49, 31, "direct_nt4"),  # odd Kd nv: direct
    (50, 33, "direct_nt4"), (50, 131, "direct_nt4"), (64, 32, "staged_nt4"), (64, 160, "direct_nt4"),
]
# NOTE (64, 32): Kd nv is even, Kd <= 32, nv > 32 -- stack_staged_ok holds, so the rule stages it (the largest flat stream
# of NT = 4: 2048 doubles, every lane's four NT requests in range)


@pytest.mark.parametrize("nv,Kd,fam", MFMA_GRID, ids=[f"nv{n}-Kd{k}" for n, k, _ in MFMA_GRID])
def test_mfma_grid(backend, nv, Kd, fam):
    B = 1 + (nv + Kd) % 3
    batch = _case(nv, Kd, B)
    assert family(backend, batch) == fam
    H, c = backend.stack(batch)
    check_exact(backend, ("grid", nv, Kd, B), batch, H, c)


SMALL_GRID = [(1, 1), (3, 4), (5, 130), (8, 37), (8, 5)]


@pytest.mark.parametrize("nv,Kd", SMALL_GRID, ids=[f"nv{n}-Kd{k}" for n, k in SMALL_GRID])
def test_small_grid(backend, nv, Kd):
    """Both packings of the nv <= 8 kernel (the emulator takes four tiles per wave for odd B, the library from B = 65 536
    on: test_library_four_tile_switch), full and tail waves."""
    for B in (1, 2, 7, 8, 9, 17):
        batch = _case(nv, Kd, B)
        H, c = backend.stack(batch)
        check_exact(backend, ("small", nv, Kd, B), batch, H, c)


@pytest.mark.parametrize("nv", [8, 30, 50])
def test_no_dense_rows(backend, nv):
    """Kd = 0, diagonal tasks only: H is diagonal and every off-diagonal entry exactly 0."""
    B = 1 + nv % 3
    batch = _case(nv, 0, B)
    H, c = backend.stack(batch)
    check_exact(backend, ("kd0", nv, B), batch, H, c)
    off = ~np.eye(nv, dtype=bool)
    assert not H[:, off].any()
    assert (H[:, ~off] > 0).all()


@pytest.mark.parametrize("nv,Kd", [(8, 5), (30, 36), (50, 24)])
def test_barrier_regulariser_and_c_extra(backend, nv, Kd):
    """One barrier of two rows with safe_displacement_gain = 2.5 and a safe displacement: r / (||Gd_rows||_F^2 dt^2) on the
    diagonal, c_extra in c.  With a barrier nv = 8 runs the MFMA kernel, not the packed one."""
    B = 1 + (nv + Kd) % 3
    batch = _case(nv, Kd, B, barrier=True)
    assert family(backend, batch) == {8: "direct_nt1", 30: "direct_nt2", 50: "staged_nt4"}[nv]
    H, c = backend.stack(batch)
    check_exact(backend, ("barrier", nv, Kd, B), batch, H, c)


# ---- row probes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,Kd", [(30, 129), (50, 131), (50, 32)])
def test_row_probes(backend, nv, Kd):
    """One instance per k in {0, 3, 4, 31, 32, 33, 127, 128, Kd - 1} in which only row k of J and e is non-zero (on about
    half of the columns): a row skipped or read twice by one pass is the whole of the entries it touches.  Same bar
    (a few ulp of one product); outside the row's support H is exactly the diagonal terms and c exactly 0."""
    ks = sorted({k for k in (0, 3, 4, 31, 32, 33, 127, 128, Kd - 1) if k < Kd})
    B = len(ks)
    base = _case(nv, Kd, B)
    key = ("probe", nv, Kd, B)
    if key not in _BATCHES:
        import dataclasses

        rng = np.random.default_rng(nv + Kd)
        J, e = np.zeros_like(base.J), np.zeros_like(base.e)
        support = rng.random(size=(B, nv)) < 0.5
        support[:, [0, 15, nv - 1]] = True
        for m, k in enumerate(ks):
            J[m, k, support[m]] = base.J[m, k, support[m]]
            e[m, k] = base.e[m, k]
        _register(key, dataclasses.replace(base, J=J, e=e, meta={"support": support}))
    batch = _BATCHES[key]
    support = batch.meta["support"]
    H, c = backend.stack(batch)
    check_exact(backend, key, batch, H, c)
    for m, k in enumerate(ks):
        ex = _exact(key, m)
        on = np.outer(support[m], support[m])
        assert (H[m][on] != 0.0).all() and (c[m][support[m]] != 0.0).all(), (k, "the row did not arrive")
        off = ~on & ~np.eye(nv, dtype=bool)
        assert not H[m][off].any() and not c[m][~support[m]].any(), (k, "entries outside the row's support")
        # (diagonal entries outside the support: the exact value check_exact held them to is the diagonal terms alone)
        assert all(ex.SH[i][i] == ex.H[i][i] and ex.Sc[i] == 0 for i in np.nonzero(~support[m])[0])


# ---- misaligned J -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,Kd", [(50, 24), (48, 32), (34, 31)])
def test_misaligned_J(backend, nv, Kd):
    """A J stream that starts 8 bytes behind a 16-byte boundary (every instance's block then does: Kd nv is even): the
    rule must send it to the direct kernel -- the staged one reads 16-byte pairs.  Meets the bar, and agrees with the
    aligned (staged) run of the same data to within two bars."""
    B = 3
    batch = _case(nv, Kd, B)
    key = ("grid", nv, Kd, B)
    assert family(backend, batch).startswith("staged") and family(backend, batch, aligned=False).startswith("direct")
    Ha, ca = _interior(batch, *backend.stack_raw(batch, j_offset=0), 0)
    Hm, cm = _interior(batch, *backend.stack_raw(batch, j_offset=1), 0)
    check_exact(backend, key, batch, Ha, ca)
    check_exact(backend, key, batch, Hm, cm, aligned=False)
    from fractions import Fraction

    from oracle.exact_stack import ULP

    for b in range(B):
        ex = _exact(key, b)
        for i in range(nv):
            assert abs(Fraction(float(ca[b, i])) - Fraction(float(cm[b, i]))) <= 2 * (ex.nc[i] + 8) * ULP * ex.Sc[i]
            for j in range(nv):
                assert abs(Fraction(float(Ha[b, i, j])) - Fraction(float(Hm[b, i, j]))) <= 2 * (ex.nH[i][j] + 8) * ULP * ex.SH[i][j]


# ---- guard bands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,Kd,B", [(8, 5, 9), (8, 5, 17), (50, 24, 3), (33, 5, 3)])
def test_guard_bands(backend, nv, Kd, B):
    """H_out and c_out inside larger buffers (nothing here is out of bounds of an allocation): the 64 doubles in front of
    and behind them keep their sentinel -- the tail of a packed wave writes only its own instances -- and every
    interior element is written."""
    batch = _case(nv, Kd, B)
    Hbuf, cbuf = backend.stack_raw(batch, guard=GUARD)
    for buf in (Hbuf, cbuf):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a store outside H_out / c_out"
        assert np.isfinite(buf[GUARD:-GUARD]).all(), "an element of H_out / c_out was not written"
    H, c = _interior(batch, Hbuf, cbuf, GUARD)
    H0, c0 = backend.stack(batch)
    assert np.array_equal(H, H0) and np.array_equal(c, c0)
    check_exact(backend, ("grid" if nv > 8 else "small", nv, Kd, B), batch, H, c, instances=[B - 1])


# ---- instance isolation in packed waves -------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [3, 8])
def test_packed_instances_are_isolated(backend, nv):
    Kd = 5
    for B in (2, 9, 17):
        batch = _case(nv, Kd, B, batched=True)
        H, c = backend.stack(batch)
        for b in range(B):
            H1, c1 = backend.stack(batch.slice(b, b + 1))
            assert np.array_equal(H1[0], H[b]) and np.array_equal(c1[0], c[b]), (B, b, "differs from the instance stacked alone")
    # an inf in one instance's J: its tile neighbour (b ^ 1) and every other instance stay bit-identical
    import dataclasses

    for B, bad in ((9, 2), (9, 8), (17, 15)):
        batch = _case(nv, Kd, B, batched=True)
        H, c = backend.stack(batch)
        J = batch.J.copy()
        J[bad, Kd // 2, nv // 2] = np.inf
        Hi, ci = backend.stack(dataclasses.replace(batch, J=J))
        others = np.arange(B) != bad
        assert not np.isfinite(Hi[bad]).all()
        assert np.array_equal(Hi[others], H[others]) and np.array_equal(ci[others], c[others]), (B, bad)


# ---- the library's own switch to four tiles per wave ------------------------------------------------------------------
def numpy_stack(batch):
    """fp64 H, c of every instance with numpy.einsum (no barriers)."""
    B, nv, Kd, K = batch.B, batch.nv, batch.Kd, batch.K
    w = np.broadcast_to(batch.cost, (B, K))
    rows = np.asarray(batch.task_rows)
    g, lm = np.zeros(K), np.zeros(K)
    for t in range(batch.T):
        g[rows[t]:rows[t + 1]], lm[rows[t]:rows[t + 1]] = batch.gain[t], batch.lm_damping[t]
    w2 = w * w
    H = np.einsum("bk,bki,bkj->bij", w2[:, :Kd], batch.J, batch.J)
    c = np.einsum("bk,bki->bi", g[:Kd] * w2[:, :Kd] * batch.e[:, :Kd], batch.J)
    mu = (lm * g * g * w2 * batch.e * batch.e).sum(axis=1) + batch.damping
    d = np.repeat(mu[:, None], nv, axis=1)
    for t in range(batch.T):
        if int(batch.task_kind[t]) == 1:
            r0, r1, c0 = int(rows[t]), int(rows[t + 1]), int(batch.task_col0[t])
            d[:, c0:c0 + r1 - r0] += w2[:, r0:r1]
            c[:, c0:c0 + r1 - r0] += g[r0:r1] * w2[:, r0:r1] * batch.e[:, r0:r1]
    H[:, np.arange(nv), np.arange(nv)] += d
    return H, c


@pytest.mark.gpu
def test_library_four_tile_switch(gpu_solver):
    """B = 65 536 + 3 at nv = 6, Kd = 7: the library itself picks ik_stack_small_kernel<4>.  The first 8 instances, the last
    11 (the tail wave: 8 199 waves of eight, three instances in the last) and 32 drawn ones meet the exact bar; all
    others agree with numpy.einsum in fp64 to the suite's 1e-13 max(1, max|.|)."""
    backend = _Gpu(gpu_solver)
    nv, Kd, B = 6, 7, 65536 + 3
    batch = _case(nv, Kd, B)
    assert family(backend, batch) == "small_tp4"
    H, c = backend.stack(batch)
    picked = np.concatenate([np.arange(8), np.arange(B - 11, B), np.sort(np.random.default_rng(4).choice(np.arange(8, B - 11), 32, replace=False))])
    check_exact(backend, ("switch", nv, Kd, B), batch, H, c, instances=picked)
    Hr, cr = numpy_stack(batch)
    assert np.abs(H - Hr).max() <= 1e-13 * max(1.0, np.abs(Hr).max())
    assert np.abs(c - cr).max() <= 1e-13 * max(1.0, np.abs(cr).max())


def test_numpy_stack_restates_the_definition():
    """The fp64 einsum reference of test_library_four_tile_switch against the exact one (no GPU needed)."""
    batch = _case(6, 7, 3)
    H, c = numpy_stack(batch)
    for b in range(3):
        rH, bH, rc, bc = exact_stack(batch, b).ratios(H[b], c[b])
        assert not bH.any() and not bc.any()
