"""pinkhip_barrier_rows_device -- the rows of PositionBarriers, BodySphericalBarriers and the sphere pairs of one
SelfCollisionBarrier formed on the device in one launch, in the form the solve consumes -- on the CPU wave emulator and on
the GPU: against 60-digit values (tests/barrier_rows_cases.py builds them), against the host classes, the exact structure of
the rows, that it writes its own rows only, that no instance's bits depend on who shares its wavefront, and what it refuses."""
import ctypes

import numpy as np
import pytest

from pink_amd import batch_eval as be
from pink_amd._lib import BarrierRowsArgs, PinkHipError
from pink_amd.batch import pack_terms
from pink_amd.kinematics_batch import BatchKinematics
from pink_amd.rollout import sphere_pairs_args
from tests.barrier_rows_cases import (BATCH, DT, K_BAR, NAMES, WIDTH, barriers_of, configurations, models, n_rows_of, note_ratios, reference,
                                      tables, with_barrier_rows, worst, write_ratios)

# a quiet NaN with a payload of its own: never the result of an operation, and NaN != NaN cannot hide a written NaN from a
# comparison of bit patterns
SENTINELS = (np.uint64(0x7FF8DEAD0000BEEF), np.uint64(0xFFF800BADC0FFEE0))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    return with_barrier_rows(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_BARRIER_ROWS_RATIOS=<file>: the worst ratios of this run as JSON (profiles/barrier_rows_exact.json)


def _backend(api):
    return "emu" if "Emu" in type(api).__name__ else "gpu"


def _filled(shape, bits):
    return np.full(shape, bits, dtype=np.uint64).view(np.float64)


class Call:
    """The device side of one call on model ``name``: model, tables, q; ``run`` launches on fresh buffers filled with a
    sentinel and returns (Gd [B, sG], hd [B, sH], dist [B, n]) -- Gd and hd as they are in memory, every stride included."""

    def __init__(self, api, name, q, n_pairs_rows=2, with_rows=True):
        self.api, self.name, self.q, self.npr = api, name, np.ascontiguousarray(q), n_pairs_rows
        arr, rows, sp, _ = tables(name, n_pairs_rows)
        self.nv, self.nq = models()[name][0].nv, models()[name][0].nq
        self.n_bar = len(rows[0]) if with_rows else 0
        self.n = self.n_bar + n_pairs_rows
        self.dm = api.model_create(arr.desc)
        self.ptrs = []
        self.rows = None
        if with_rows:
            self.rows = BarrierRowsArgs()
            self.rows.n_rows = len(rows[0])
            self.rows.frame, self.rows.axis, self.rows.sign, self.rows.bound, self.rows.gain, self.rows.frame2 = (self._up(a) for a in rows)
        self.pairs = None
        if n_pairs_rows:
            self.pairs = sphere_pairs_args([self._up(a) for a in sp], sp, barriers_of(name, n_pairs_rows)[-1])
        self.d_q = self._up(self.q)

    def _up(self, a):
        p = self.api.alloc(max(a.nbytes, 8))
        self.api.put(p, a)
        self.ptrs.append(p)
        return p

    def run(self, sG=None, sH=None, row0=0, fill=SENTINELS[0], with_dist=True, B=None, **kw):
        B = self.q.shape[0] if B is None else B
        sG = self.n * self.nv if sG is None else sG
        sH = self.n if sH is None else sH
        G, h, d = _filled((self.q.shape[0], sG), fill), _filled((self.q.shape[0], sH), fill), _filled((self.q.shape[0], max(self.npr, 1)), fill)
        d_G, d_h, d_d = (self._up(a) for a in (G, h, d))
        args = dict(model=self.dm, B=B, q=self.d_q, dt=DT, rows=self.rows, pairs=self.pairs, Gd=d_G, sG=sG, hd=d_h, sH=sH, row0=row0,
                    dist=d_d if with_dist else None)
        args.update(kw)
        try:
            self.api.barrier_rows(*(args[k] for k in ("model", "B", "q", "dt", "rows", "pairs", "Gd", "sG", "hd", "sH", "row0", "dist")))
        finally:
            self.api.sync()
            self.api.get(G, d_G), self.api.get(h, d_h), self.api.get(d, d_d)
            for p in (d_G, d_h, d_d):
                self.api.release(p)
                self.ptrs.remove(p)
        return G, h, d

    def close(self):
        for p in self.ptrs:
            self.api.release(p)
        self.api.model_destroy(self.dm)


def device_rows(api, name, q, n_pairs_rows=2, **kw):
    c = Call(api, name, q, n_pairs_rows)
    try:
        return c.run(**kw)
    finally:
        c.close()


def _off_path_columns(model, joints):
    path = set()
    for j in joints:
        while j >= 0:
            path.add(j)
            j = model.joints[j].parent
    return [c for i, jt in enumerate(model.joints) if i not in path for c in range(jt.idx_v, jt.idx_v + jt.nv)]


# ---- 1. exact anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs_rows", [2, 5])
@pytest.mark.parametrize("name", NAMES)
def test_rows_against_60_digits(api, name, n_pairs_rows):
    """Gd, hd and the selected distances within K_BAR = 8 units of u = S + eps max|exact| (what one ulp on the inputs -- model,
    q, bounds, gains, spheres, dt -- does to the exact result), and the exact structure: columns of joints off a row's paths
    == 0.0, the row of the touching pair == 0.0, hd of the pair rows == gain (dist_out - d_min) bit for bit, ascending."""
    model, _ = models()[name]
    arr, rows, sp, (_, d_min, gain) = tables(name, n_pairs_rows)
    q, _ = reference(name, n_pairs_rows)
    B, nv, n = q.shape[0], model.nv, n_rows_of(name, n_pairs_rows)
    G, h, d = device_rows(api, name, q, n_pairs_rows)
    G = G.reshape(B, n, nv)
    rg, rh, rd = worst(name, G, h, d, n_pairs_rows)
    print(f"{_backend(api):4s} {name} W {WIDTH[name]:2d} pair rows {n_pairs_rows} G {rg:.3g} h {rh:.3g} dist {rd:.3g} (bar {K_BAR:.3g})")
    note_ratios(_backend(api), f"{name}_{n_pairs_rows}", rg, rh, rd)
    assert rg <= K_BAR and rh <= K_BAR and rd <= K_BAR, (rg, rh, rd)
    n_bar = len(rows[0])
    for r in range(n_bar):
        joints = [int(arr.frame_joint[rows[0][r]])] + ([int(arr.frame_joint[rows[5][r]])] if rows[1][r] == 3 else [])
        off = _off_path_columns(model, joints)
        assert (G[:, r, off] == 0.0).all() and (G[:, r] != 0.0).any(), r
    off = _off_path_columns(model, [int(j) for j in sp[0]])
    assert (G[:, n_bar:][:, :, off] == 0.0).all()
    assert np.array_equal(h[:, n_bar:], gain * (d - d_min)) and (np.diff(d, axis=1) >= 0.0).all()
    touching = np.abs(d) < 1e-12  # (spheres 2 and 3 ride on one joint, 0.25 apart with radii 0.125: the smallest distance bar overlaps)
    assert touching.any(axis=1).all() and (G[:, n_bar:][touching] == 0.0).all() and (G[:, n_bar:][~touching] != 0.0).any()


# ---- 2. the host classes ----------------------------------------------------------------------------------------------------
def _host_rows(name, q, n_pairs_rows=2):
    """(G [B, n, nv], h [B, n]) of the same barriers through the batched host evaluation and pack_terms; the rows of the
    SelfCollisionBarrier (the host keeps the closest pairs in no particular order) sorted by ascending right-hand side."""
    model, _ = models()[name]
    kin = BatchKinematics(model, q)
    terms = [be.barrier_term(kin, bar) for bar in barriers_of(name, n_pairs_rows)]
    b0 = pack_terms(model.nv, [], DT, barriers=terms, batch_size=q.shape[0])
    G, h = b0.Gd.copy(), b0.hd.copy()
    k = G.shape[1] - n_pairs_rows
    for b in range(q.shape[0]):
        order = k + np.argsort(h[b, k:], kind="stable")
        G[b, k:], h[b, k:] = G[b, order], h[b, order]
    return G, h


def _rel(X, Y):
    """Largest |X - Y| of an instance over its largest |Y|, the worst instance."""
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(X, Y))


@pytest.mark.parametrize("name", NAMES)
def test_rows_against_the_host_classes(api, name):
    """The relative difference from be.barrier_term + pack_terms stays below ten times the relative difference of that host
    evaluation itself from the 60-digit reference on the same cases."""
    model, _ = models()[name]
    q, ref = reference(name)
    B, nv, n = q.shape[0], model.nv, n_rows_of(name)
    Gh, hh = _host_rows(name, q)
    hostG, hosth, _ = worst(name, Gh, hh)
    exact_G = [ref[b][0][0][0].reshape(n, nv) for b in range(B)]
    exact_h = [ref[b][1][0][0] for b in range(B)]
    bar_G, bar_h = 10.0 * _rel(Gh, exact_G), 10.0 * _rel(hh, exact_h)
    G, h, _ = device_rows(api, name, q)
    dG, dh = _rel(G.reshape(B, n, nv), Gh), _rel(h, hh)
    print(f"{_backend(api):4s} {name} host vs exact: {hostG:.3g} / {hosth:.3g} units, bars {bar_G:.3g} / {bar_h:.3g}; device vs host {dG:.3g} / {dh:.3g}")
    note_ratios("host", f"{name}_2", hostG, hosth)
    note_ratios("host_relative_bar", f"{name}_2", bar_G, bar_h)
    note_ratios(f"{_backend(api)}_vs_host_relative", f"{name}_2", dG, dh)
    assert bar_G < 1e-13 and bar_h < 1e-13  # (the host evaluation is a double-precision one)
    assert dG <= bar_G and dh <= bar_h, (dG, bar_G, dh, bar_h)


# ---- 3. only its rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_only_its_rows_are_written(api, name):
    """row0 = 3 and strides larger than the rows, on buffers poisoned with NaN-patterned sentinels: exactly the n entries of hd
    and the n nv entries of Gd of every instance change, and they are the bits of the call at row0 = 0 with natural strides;
    the padded lanes of a group and the robots b >= B of the last wavefront write nothing; dist_out = NULL leaves that buffer
    alone; rows without pairs and pairs without rows write what the full call writes there."""
    model, _ = models()[name]
    q = configurations(name)
    B, nv, n = q.shape[0], model.nv, n_rows_of(name)
    c = Call(api, name, q)
    try:
        G0, h0, d0 = c.run()
        sG, sH, row0 = (3 + n + 2) * nv + 7, 3 + n + 5, 3
        for fill in SENTINELS:  # (two sentinels: a written value equal to one of them cannot hide)
            G, h, d = c.run(sG=sG, sH=sH, row0=row0, fill=fill, with_dist=False)
            want_h = np.zeros((B, sH), bool)
            want_h[:, row0:row0 + n] = True
            want_G = np.zeros((B, sG), bool)
            want_G[:, row0 * nv:(row0 + n) * nv] = True
            assert np.array_equal(h.view(np.uint64) != fill, want_h) and np.array_equal(G.view(np.uint64) != fill, want_G)
            assert (d.view(np.uint64) == fill).all()
            assert h[:, row0:row0 + n].tobytes() == h0.tobytes() and G[:, row0 * nv:(row0 + n) * nv].tobytes() == G0.tobytes()
        # a batch shorter than the buffers: the instances behind it stay as they were
        G, h, d = c.run(B=B - 1)
        assert (G[B - 1].view(np.uint64) == SENTINELS[0]).all() and (h[B - 1].view(np.uint64) == SENTINELS[0]).all()
        assert (d[B - 1].view(np.uint64) == SENTINELS[0]).all() and G[:B - 1].tobytes() == G0[:B - 1].tobytes()
    finally:
        c.close()
    k = n - 2
    rows_only = Call(api, name, q, 0)
    pairs_only = Call(api, name, q, 2, with_rows=False)
    try:
        G, h, _ = rows_only.run()
        assert G.tobytes() == np.ascontiguousarray(G0[:, :k * nv]).tobytes() and h.tobytes() == np.ascontiguousarray(h0[:, :k]).tobytes()
        G, h, d = pairs_only.run()
        assert G.tobytes() == np.ascontiguousarray(G0[:, k * nv:]).tobytes() and h.tobytes() == np.ascontiguousarray(h0[:, k:]).tobytes()
        assert d.tobytes() == d0.tobytes()
    finally:
        rows_only.close()
        pairs_only.close()


# ---- 4. company -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_no_instance_depends_on_who_shares_its_wavefront(api, name):
    """Every instance alone (a wavefront of its own, its other groups idle) and in every group slot of a wavefront whose other
    robots sit at NaN / Inf / 1e6 rad: the same bits (tests/test_wave_isolation.py), and finite rows."""
    model, _ = models()[name]
    q = configurations(name)[:5]
    B, nq, per = q.shape[0], model.nq, 64 // WIDTH[name]
    alone = [device_rows(api, name, q[b:b + 1]) for b in range(B)]
    poison = [np.nan, np.inf, 1e6, -np.inf]
    big = np.empty((B * per * per, nq))
    for b in range(B):
        for s in range(per):
            wave = big[(b * per + s) * per:(b * per + s + 1) * per]
            for o in range(per):
                wave[o] = poison[(o + s + b) % 4]
            wave[s] = q[b]
    G, h, d = device_rows(api, name, big)
    for b in range(B):
        for s in range(per):
            i = (b * per + s) * per + s
            for got, ref in zip((G[i], h[i], d[i]), alone[b]):
                assert got.tobytes() == ref[0].tobytes(), (b, s)
    own = [(b * per + s) * per + s for b in range(B) for s in range(per)]
    assert np.isfinite(G[own]).all() and np.isfinite(h[own]).all() and np.isfinite(d[own]).all()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _refused(c, kw):
    """(code, Gd, hd, dist) of a call that must be refused, the buffers as they are afterwards."""
    B, sG, sH = c.q.shape[0], c.n * c.nv, c.n
    G, h, d = _filled((B, sG), SENTINELS[0]), _filled((B, sH), SENTINELS[0]), _filled((B, 2), SENTINELS[0])
    d_G, d_h, d_d = (c._up(a) for a in (G, h, d))
    args = dict(model=c.dm, B=B, q=c.d_q, dt=DT, rows=c.rows, pairs=c.pairs, Gd=d_G, sG=sG, hd=d_h, sH=sH, row0=0, dist=d_d)
    args.update(kw)
    with pytest.raises(PinkHipError) as ex:
        c.api.barrier_rows(*(args[k] for k in ("model", "B", "q", "dt", "rows", "pairs", "Gd", "sG", "hd", "sH", "row0", "dist")))
    c.api.sync()
    c.api.get(G, d_G), c.api.get(h, d_h), c.api.get(d, d_d)
    return ex.value.code, G, h, d


def _copy_of(struct, **kw):
    out = type(struct)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(struct), ctypes.sizeof(out))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def test_refusals_leave_the_outputs_alone(api):
    """Each refusal of the header returns its code and touches nothing; B = 0 is fine."""
    name = "B"
    c = Call(api, name, configurations(name))
    n, nv = c.n, c.nv
    rows, pairs = (lambda **kw: _copy_of(c.rows, **kw)), (lambda **kw: _copy_of(c.pairs, **kw))
    invalid = [dict(q=None), dict(Gd=None), dict(hd=None), dict(row0=-1), dict(sH=n - 1), dict(sG=n * nv - 1), dict(row0=1),
               dict(dt=0.0), dict(dt=-1e-3), dict(dt=np.inf), dict(dt=np.nan),
               dict(rows=None, pairs=None), dict(rows=rows(n_rows=0), pairs=None), dict(rows=rows(n_rows=-1)),
               dict(rows=rows(frame=None)), dict(rows=rows(axis=None)), dict(rows=rows(frame2=None)), dict(rows=rows(sign=None)),
               dict(rows=rows(bound=None)), dict(rows=rows(gain=None)),
               dict(pairs=pairs(n_rows=0)), dict(pairs=pairs(n_rows=6)), dict(pairs=pairs(sphere_joint=None)),
               dict(pairs=pairs(sphere_centre=None)), dict(pairs=pairs(sphere_radius=None)), dict(pairs=pairs(column_mask=None)),
               dict(pairs=pairs(pair_sphere=None)), dict(pairs=pairs(n_spheres=0)), dict(pairs=pairs(n_pairs=0)), dict(model=None)]
    unsupported = [dict(pairs=pairs(n_spheres=33)), dict(pairs=pairs(n_pairs=65)),
                   dict(rows=rows(n_rows=63)), dict(rows=rows(n_rows=65), pairs=None)]  # (more than PINKHIP_MAX_MD = 64 rows)
    try:
        for want, cases in ((-1, invalid), (-5, unsupported)):
            for kw in cases:
                code, G, h, d = _refused(c, kw)
                assert code == want, kw
                for a in (G, h, d):
                    assert (a.view(np.uint64) == SENTINELS[0]).all(), kw
        for kw in (dict(B=0), dict(B=0, q=None, Gd=None, hd=None)):  # an empty batch is fine, whatever the pointers
            G, h, d = c.run(**kw)
            for a in (G, h, d):
                assert (a.view(np.uint64) == SENTINELS[0]).all()
        G, h, d = c.run()  # and the valid call writes every row
        for a in (G, h, d):
            assert (a.view(np.uint64) != SENTINELS[0]).all()
    finally:
        c.close()


def test_more_than_64_joints_are_unsupported(emu):
    """One lane per joint: PINKHIP_E_UNSUPPORTED (-5) for nj > 64, from the check the library and the emulator share
    (plan_barrier_rows).  A model with more than 64 joints has nv > PINKHIP_MAX_NV and cannot be created, so the check is
    asked about a bare joint count."""
    lib = emu.lib
    lib.pinkhip_emu_barrier_rows_joint_check.argtypes = [ctypes.c_int]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
    assert lib.pinkhip_emu_barrier_rows_joint_check(64) == 0
    assert lib.pinkhip_emu_barrier_rows_joint_check(65) == -5 and "nj <= 64" in lib.pinkhip_emu_last_error().decode()


def test_the_library_exports_the_call():
    """include/pinkhip.h declares pinkhip_barrier_rows_device under PINKHIP_HAS_BARRIER_ROWS, pink_amd._lib lists it among
    the ABI symbols, and the struct has the header's layout (tests/test_abi.py holds the whole list to the header)."""
    import os

    from pink_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinkhip.h")).read()
    assert "#define PINKHIP_HAS_BARRIER_ROWS 1" in header and "pinkhip_barrier_rows_device(" in header
    assert "pinkhip_barrier_rows_device" in _lib.ABI_SYMBOLS
    assert ctypes.sizeof(BarrierRowsArgs) == 8 + 6 * 8
    assert BATCH == {"A": 19, "B": 5, "C": 3}
