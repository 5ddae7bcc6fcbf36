"""The group primitives of pink_amd/csrc/wave.h against NumPy on each group's own W values, bit for bit.

Every solver family packs 64 / W problems into one wavefront and keeps them apart with nothing but these primitives: DPP
butterflies (quad_perm, row_half_mirror, row_mirror, row_shr, row_bcast15 / 31, row_newbcast), v_permlane16 / 32_swap,
ds_bpermute, raw v_min_f64 and EXEC masking (lanes_on).  The CPU emulator replaces all of that with rendezvous of 64 fibers
(emu/wave_emu.h), so the kernel tests under ``-m "not gpu"`` never run it.  Here one probe kernel
(tests/wave/wave_probe_kernel.h) applies each primitive to a [64] input, one wavefront per input set, for W = 8, 16, 32, 64;
the same source is compiled for gfx950 against wave.h (tests/wave/wave_probe.hip -> tests/wave/libwaveprobe.so, built by
``build()``) and into the emulator library against wave_emu.h (emu/emu_wave_probe.cpp), and both face the same reference.

Inputs are integer-valued doubles of mixed sign below 2^40: a sum of 64 of them is exact in any order, a product with a
small integer is exact, and acc + s * x of fma_bcast is the correctly rounded value of the exact integer -- so every
comparison is on bits, with no tolerance.

Poison pass: the other groups of the wave hold NaN, +-Inf, -0.0, denormals, 1e300 and extreme integers / predicates.  With
one clean group at each position in turn (everything else poisoned) and with one poisoned group at each position in turn
(everything else clean), every clean lane must return the bits of the clean launch.  Wave-wide primitives (wave_sum,
wave_min, wave_any, wave_ballot, groups_max / groups_min) have nothing to isolate and are held to the reference on clean
inputs only.

Contracts the source states inside a group: min_raw is v_min_f64 on operands that are never signalling NaNs, i.e. fmin --
a quiet NaN loses against a number; wave_min is fmin; key32_pack clamps into the normal negative floats, so that -Inf and
anything that rounds to -0.0f or a denormal still carry their payload and read as candidates.  The sign of a zero minimum
is not stated anywhere and not asserted."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [8, 16, 32, 64]

# slots of tests/wave/wave_probe_kernel.h
D = {n: i for i, n in enumerate(["group_sum", "group_min", "group_scan_sum", "group_bcast", "lane_shfl", "row_pair_a", "row_pair_b",
                                 "wave_sum", "wave_min", "on_sum", "on_min", "on_scan"])}
TABLES = ["value_bcast", "fma_bcast", "bcast_indicator", "bcast_select", "bcast_scale"]
I = {n: i for i, n in enumerate(["group_first_lane", "group_bcast_i", "groups_max", "groups_min", "wave_any", "min32_payload", "min32_bits",
                                 "key32_bits", "lane_shfl_i", "ballot_lo", "ballot_hi", "on_first_lane"])}
# primitive -> the slots that show it (the rows of the table in profiles/wave_isolation.json)
PRIMITIVES = {
    "group_sum": ["group_sum"], "group_min": ["group_min"], "group_min32": ["min32_payload", "min32_bits"], "key32_pack": ["key32_bits"],
    "group_scan_sum": ["group_scan_sum"], "group_first_lane": ["group_first_lane"], "group_bcast": ["group_bcast"],
    "group_bcast_i": ["group_bcast_i"], "groups_max": ["groups_max"], "groups_min": ["groups_min"], "row_pair": ["row_pair_a", "row_pair_b"],
    "lane_shfl": ["lane_shfl", "lane_shfl_i"], "value_bcast": ["value_bcast"], "fma_bcast": ["fma_bcast"], "bcast_indicator": ["bcast_indicator"],
    "bcast_select": ["bcast_select"], "bcast_scale": ["bcast_scale"], "wave_sum": ["wave_sum"], "wave_min": ["wave_min"], "wave_any": ["wave_any"],
    "wave_ballot": ["ballot_lo", "ballot_hi"], "lanes_on": ["on_sum", "on_min", "on_scan", "on_first_lane"],
}
WAVE_WIDE = {"wave_sum", "wave_min", "wave_any", "ballot_lo", "ballot_hi", "groups_max", "groups_min"}
FIELDS_D, FIELDS_I = ("v", "x", "acc", "key"), ("pred", "gsrc", "isrc", "lsrc", "gint", "ival", "on")
TABLE = {}  # (backend, primitive, W) -> [lanes compared, lanes that differed], written by _compare


class Probe:
    """``wave_probe_run`` of the device library or its emulator twin: a dict of [sets, 64] arrays in, the slots out."""

    def __init__(self, lib, prefix):
        self.run_fn = getattr(lib, prefix + "wave_probe_run")
        self.slots_d, self.slots_i = getattr(lib, prefix + "wave_probe_slots_d"), getattr(lib, prefix + "wave_probe_slots_i")
        self.run_fn.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 13
        self.error = getattr(lib, "wave_probe_last_error", None)
        if self.error is not None:
            self.error.restype = ctypes.c_char_p

    def run(self, W, inp):
        sets = inp["v"].shape[0]
        arrs = [np.ascontiguousarray(inp[k], dtype=np.float64) for k in FIELDS_D] + [np.ascontiguousarray(inp[k], dtype=np.int32) for k in FIELDS_I]
        assert all(a.shape == (sets, 64) for a in arrs)
        assert ((arrs[5] >= 0) & (arrs[5] < W)).all() and ((arrs[7] >= 0) & (arrs[7] < 64)).all()  # gsrc, lsrc: lanes that exist
        nd, ni = self.slots_d(W), self.slots_i()
        assert nd == len(D) + (len(TABLES) * W if W >= 16 else 0) and ni == len(I)
        out_d, out_i = np.full((sets, nd, 64), -777.5), np.full((sets, ni, 64), -777, dtype=np.int32)
        rc = self.run_fn(W, sets, *[a.ctypes.data for a in arrs], out_d.ctypes.data, out_i.ctypes.data)
        assert rc == 0, (rc, self.error().decode() if self.error else "")
        return out_d, out_i


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def probe(request, built):
    if request.param == "emu":
        return "emu", Probe(ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libpinkemu.so")), "pinkhip_emu_")
    return "gpu", Probe(ctypes.CDLL(os.path.join(ROOT, "tests", "wave", "libwaveprobe.so")), "")


# ------------------------------------------------------------------------------------------------------------- inputs


def _ints(rng, n, bits):
    """integer-valued doubles of mixed sign, magnitudes spread over 1 .. 2^bits"""
    mag = np.floor(2.0 ** rng.uniform(0.0, bits, size=n))
    return np.where(rng.random(n) < 0.5, -mag, mag)


def clean_set(rng, W, local_shfl=False):
    g = np.arange(64) // W
    ng = 64 // W
    per_group = lambda a: np.asarray(a)[g]
    pred = (rng.random(64) < rng.choice([0.05, 0.3, 0.9], size=ng)[g]).astype(np.int32)
    if ng > 1:
        pred[g == int(rng.integers(ng))] = 0  # a group without any (first lane = W)
    s = dict(v=_ints(rng, 64, 40), x=_ints(rng, 64, 40), acc=_ints(rng, 64, 40), key=-(10.0 ** rng.uniform(-3, 3, size=64)), pred=pred,
             gsrc=per_group(rng.integers(0, W, size=ng)), isrc=per_group(rng.integers(-1, W, size=ng)),
             lsrc=(g * W + rng.integers(0, W, size=64)) if local_shfl else rng.integers(0, 64, size=64),
             gint=per_group(rng.integers(-2000, 2001, size=ng)), ival=rng.integers(-2 ** 31, 2 ** 31, size=64), on=per_group(rng.integers(0, 2, size=ng)))
    return {k: np.asarray(a, dtype=np.float64 if k in FIELDS_D else np.int64) for k, a in s.items()}


POISON_D = [np.nan, np.inf, -np.inf, -0.0, 5e-324, -2.5e-310, 1e300, -1e300]
POISON_I = [-2 ** 31, 2 ** 31 - 1, -1, 0]


def poisoned(base, W, clean_groups, variant):
    """``base`` with every group outside ``clean_groups`` poisoned: the doubles with POISON_D (rotated by ``variant``), the keys
    with values key32_pack is not made for, predicates all set or all clear, extreme integers, other source lanes."""
    s = {k: a.copy() for k, a in base.items()}
    g = np.arange(64) // W
    bad = ~np.isin(g, clean_groups)
    lanes = np.nonzero(bad)[0]
    for n, k in enumerate(FIELDS_D):
        s[k][lanes] = [POISON_D[(l + variant + 3 * n) % len(POISON_D)] for l in lanes]
    s["key"][lanes] = [[np.nan, np.inf, 1.0, 0.0, -np.inf, -0.0][(l + variant) % 6] for l in lanes]
    s["pred"][lanes] = (g[lanes] + variant) % 2
    s["on"][lanes] = (g[lanes] + variant // 2) % 2
    s["gint"][lanes] = [POISON_I[(g[l] + variant) % 4] for l in lanes]
    s["ival"][lanes] = [POISON_I[(l + variant) % 4] for l in lanes]
    s["gsrc"][lanes] = (s["gsrc"][lanes] + 1 + variant) % W
    s["isrc"][lanes] = (s["isrc"][lanes] + 2 + variant) % (W + 1) - 1
    s["lsrc"][lanes] = (lanes + 17 * (variant + 1)) % 64  # (the poisoned lanes may read anywhere; the clean ones read their group)
    return s, ~bad


def stack(sets):
    return {k: np.stack([s[k] for s in sets]) for k in sets[0]}


# ---------------------------------------------------------------------------------------------------------- reference


def _rn(i):
    return float(i)  # (int -> float is correctly rounded)


def reference(W, s, lanes):
    """NumPy / exact integers on each group's own W values, for the lanes in the boolean mask ``lanes`` (whole groups); other
    lanes are left NaN / -777.  Wave-wide slots are filled only when every lane is asked for."""
    nd = len(D) + (len(TABLES) * W if W >= 16 else 0)
    rd, ri = np.full((nd, 64), np.nan), np.full((len(I), 64), -777, dtype=np.int64)
    v, x, acc, on = s["v"], s["x"], s["acc"], s["on"] != 0
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        kf = np.maximum(np.minimum(s["key"].astype(f32), f32(-1.17549435e-38)), f32(-3.0e38))
    kbits = (kf.view(np.int32) & ~np.int32(0xFF)) | (np.arange(64, dtype=np.int32) & (W - 1))
    for g0 in range(0, 64, W):
        if not lanes[g0]:
            continue
        sl = slice(g0, g0 + W)
        gv, gon, gp = v[sl], bool(on[g0]), s["pred"][sl] != 0
        first = int(np.argmax(gp)) if gp.any() else W
        rd[D["group_sum"], sl], rd[D["group_min"], sl], rd[D["group_scan_sum"], sl] = gv.sum(), gv.min(), np.cumsum(gv)
        rd[D["group_bcast"], sl] = gv[s["gsrc"][g0]]
        rd[D["on_sum"], sl] = gv.sum() if gon else gv
        rd[D["on_min"], sl] = gv.min() if gon else gv
        rd[D["on_scan"], sl] = np.cumsum(gv) if gon else gv
        ri[I["group_first_lane"], sl] = first
        ri[I["on_first_lane"], sl] = first if gon else -1
        ri[I["group_bcast_i"], sl] = s["ival"][g0 + s["gsrc"][g0]]
        win = kbits[sl][np.argmin(kbits[sl].view(f32))]  # (distinct payloads: one smallest key)
        ri[I["min32_bits"], sl], ri[I["min32_payload"], sl] = win, win & 0xFF
        ri[I["key32_bits"], sl] = kbits[sl]
        if W >= 16:
            t = len(D)
            for J in range(W):
                rd[t + 0 * W + J, sl] = gv[J]
                rd[t + 1 * W + J, sl] = [_rn(int(acc[l]) + int(gv[J]) * int(x[l])) for l in range(g0, g0 + W)]
                rd[t + 2 * W + J, sl] = 1.0 if J == s["isrc"][g0] else 0.0
                rd[t + 3 * W + J, sl] = gv[J] if gon else x[g0 + J]
                rd[t + 4 * W + J, sl] = gv[J] * float(s["gint"][g0])
    ls = s["lsrc"]
    ok = lanes & lanes[ls]  # (a lane that reads a poisoned lane is not compared)
    rd[D["lane_shfl"], ok], ri[I["lane_shfl_i"], ok] = v[ls[ok]], s["ival"][ls[ok]]
    if W <= 16:  # (whole rows of 16 inside one group, or groups inside a row: the partner row may be poisoned)
        ok = lanes & lanes[np.arange(64) ^ 16]
    else:
        ok = lanes
    rd[D["row_pair_a"], ok], rd[D["row_pair_b"], ok] = v[np.arange(64)[ok] & ~16], v[np.arange(64)[ok] | 16]
    if lanes.all():
        rd[D["wave_sum"]], rd[D["wave_min"]] = v.sum(), v.min()
        ri[I["groups_max"]], ri[I["groups_min"]] = s["gint"].max(), s["gint"].min()
        ri[I["wave_any"]] = int((s["pred"] != 0).any())
        ballot = sum(1 << l for l in range(64) if s["pred"][l])
        ri[I["ballot_lo"]], ri[I["ballot_hi"]] = np.int64(ballot & 0xFFFFFFFF).astype(np.int32), np.int64(ballot >> 32).astype(np.int32)
    return rd, ri.astype(np.int32), ~np.isnan(rd), ri != -777


def _slot_rows(name, W):
    """(is double, rows of the output) of one slot name"""
    if name in D:
        return True, [D[name]]
    if name in TABLES:
        return True, list(range(len(D) + TABLES.index(name) * W, len(D) + (TABLES.index(name) + 1) * W)) if W >= 16 else []
    return False, [I[name]]


def _compare(backend, W, out_d, out_i, ref_d, ref_i, have_d, have_i, what):
    """Bits of every referenced lane; fills TABLE and returns the list of differences."""
    diffs = []
    for prim, slots in PRIMITIVES.items():
        n = bad = 0
        for name in slots:
            dbl, rows = _slot_rows(name, W)
            for r in rows:
                got, ref, have = (out_d[r], ref_d[r], have_d[r]) if dbl else (out_i[r], ref_i[r], have_i[r])
                eq = (got.view(np.uint64) == ref.view(np.uint64)) if dbl else (got == ref)
                wrong = np.nonzero(have & ~eq)[0]
                n, bad = n + int(have.sum()), bad + len(wrong)
                for l in wrong[:4]:
                    diffs.append(f"{backend} W={W} {what}: {name} source lane {r - rows[0]} lane {l}: got {got[l]!r}, reference {ref[l]!r}")
        if n:  # (the broadcast-FMA primitives have no W = 8)
            t = TABLE.setdefault((backend, prim, W), [0, 0])
            t[0], t[1] = t[0] + n, t[1] + bad
    return diffs


def _dump(backend):
    """With PINKHIP_WAVE_ISOLATION_RECORD=<prefix>: the primitive x W table of this run so far, for scripts/wave_isolation_record.py"""
    out = os.environ.get("PINKHIP_WAVE_ISOLATION_RECORD")
    if out:
        with open(f"{out}.primitives.{backend}.json", "w") as f:
            json.dump({f"{prim}/W{W}": v for (b, prim, W), v in sorted(TABLE.items()) if b == backend}, f, indent=1)


# -------------------------------------------------------------------------------------------------------------- tests


@pytest.mark.parametrize("W", WIDTHS)
def test_primitives_against_numpy_on_clean_inputs(probe, W):
    backend, p = probe
    rng = np.random.default_rng(100 + W)
    sets = [clean_set(rng, W) for _ in range(6)]
    ng = 64 // W
    # lanes_on with exactly one group on, exactly one off, none, all; a wave without any predicate set
    for k in range(ng):
        for invert in (0, 1):
            s = clean_set(rng, W)
            s["on"] = ((np.arange(64) // W == k) ^ invert).astype(np.int64)
            sets.append(s)
    s = clean_set(rng, W)
    s["pred"][:] = 0
    sets.append(s)
    out_d, out_i = p.run(W, stack(sets))
    diffs, everything = [], np.ones(64, bool)
    for n, s in enumerate(sets):
        diffs += _compare(backend, W, out_d[n], out_i[n], *reference(W, s, everything), f"clean set {n}")
    # every slot of every lane was written and referenced
    assert not (out_d == -777.5).any() and not (out_i == -777).any()
    _dump(backend)
    assert not diffs, "\n".join(diffs[:40])


@pytest.mark.parametrize("W", [8, 16, 32])
def test_clean_groups_keep_their_bits_next_to_poisoned_groups(probe, W):
    backend, p = probe
    rng = np.random.default_rng(200 + W)
    ng = 64 // W
    bases = [clean_set(rng, W, local_shfl=True) for _ in range(2)]
    for b in bases:
        b["on"][:] = 1  # (clean groups on; the poisoned groups are on or off, by variant)
    bases[1]["on"][:] = np.asarray(rng.integers(0, 2, size=ng))[np.arange(64) // W]
    sets, masks, origin = list(bases), [np.ones(64, bool)] * 2, [0, 1]
    for bi, b in enumerate(bases):
        for k in range(ng):
            for clean_groups in ([k], [j for j in range(ng) if j != k]):  # one clean group at k / one poisoned group at k
                for variant in range(4 if bi == 0 else 2):
                    s, m = poisoned(b, W, clean_groups, variant + k)
                    sets.append(s), masks.append(m), origin.append(bi)
    covered = np.zeros((2, ng), int)
    for m, o in zip(masks[2:], origin[2:]):
        g = m.reshape(ng, W)[:, 0]
        covered[0, g] += g.sum() == 1  # this position was the only clean group
        covered[1, ~g] += (~g).sum() == 1  # this position was the only poisoned group
    assert (covered > 0).all(), covered
    out_d, out_i = p.run(W, stack(sets))
    diffs = []
    for n, (s, m, o) in enumerate(zip(sets, masks, origin)):
        ref_d, ref_i, have_d, have_i = reference(W, s, m)
        diffs += _compare(backend, W, out_d[n], out_i[n], ref_d, ref_i, have_d, have_i, f"poison set {n}")
        if n >= 2:  # ... and the very bits of the launch without poison, wherever the reference speaks
            same_d = out_d[n].view(np.uint64) == out_d[o].view(np.uint64)
            same_i = out_i[n] == out_i[o]
            wide_d = np.zeros(out_d[n].shape[0], bool)
            wide_d[[D[k] for k in D if k in WAVE_WIDE]] = True
            wide_i = np.zeros(len(I), bool)
            wide_i[[I[k] for k in I if k in WAVE_WIDE]] = True
            for r, l in zip(*np.nonzero(have_d & ~same_d & ~wide_d[:, None])):
                diffs.append(f"{backend} W={W} poison set {n}: double slot {r} lane {l} differs from the clean launch")
            for r, l in zip(*np.nonzero(have_i & ~same_i & ~wide_i[:, None])):
                diffs.append(f"{backend} W={W} poison set {n}: int slot {r} lane {l} differs from the clean launch")
    for n_bad in (len(diffs),):  # (a difference from the clean launch is a lane that differed, whichever slot)
        t = TABLE.setdefault((backend, "poison_pass", W), [0, 0])
        t[0], t[1] = t[0] + sum(int(m.sum()) for m in masks[2:]), t[1] + n_bad
    _dump(backend)
    assert not diffs, "\n".join(diffs[:40])


@pytest.mark.parametrize("W", WIDTHS)
def test_contracts_inside_a_group(probe, W):
    """min_raw / group_min / wave_min on quiet NaNs and infinities (fmin: a NaN loses against a number, a group of NaNs
    gives NaN), key32_pack's clamping at -Inf, -0.0, a double below the floats' normal range and one beyond their largest."""
    backend, p = probe
    rng = np.random.default_rng(300 + W)
    ng, g = 64 // W, np.arange(64) // W
    sets = []
    for n in range(4):
        s = clean_set(rng, W)
        s["v"][rng.random(64) < [0.1, 0.5, 0.9, 0.3][n]] = np.nan
        s["v"][rng.random(64) < 0.1] = np.inf
        if n == 3:
            s["v"][rng.random(64) < 0.1] = -np.inf
        if ng > 1:
            s["v"][g == n % ng] = np.nan  # a whole group of NaNs
        s["v"][(n * 9) % 64] = 7.0  # (the wave keeps a number)
        special = [-np.inf, -0.0, -1e-300, -1e300, -1e-45, -3.5e38]
        for k in range(ng):
            lanes = k * W + rng.permutation(W)[:3]
            s["key"][lanes] = [special[(k + n + j) % len(special)] for j in range(3)]
        s["on"][:] = 1
        sets.append(s)
    out_d, out_i = p.run(W, stack(sets))
    f32 = np.float32
    for n, s in enumerate(sets):
        v = s["v"]
        for g0 in range(0, 64, W):
            gv = v[g0:g0 + W]
            want = np.nan if np.isnan(gv).all() else np.nanmin(gv)
            for slot in ("group_min", "on_min"):
                got = out_d[n, D[slot], g0:g0 + W]
                assert (np.isnan(got).all() if np.isnan(want) else (got == want).all()), (backend, W, n, g0, slot, got, want)
            kb = out_i[n, I["key32_bits"], g0:g0 + W]
            kf = kb.view(f32)
            assert np.isfinite(kf).all() and (kf <= f32(-1.17549435e-38)).all() and (kf >= f32(-3.0e38)).all(), (backend, W, n, g0, kf)
            assert ((kb & 0xFF) == np.arange(W)).all()
            win = kb[np.argmin(kf)]
            assert (out_i[n, I["min32_bits"], g0:g0 + W] == win).all() and (out_i[n, I["min32_payload"], g0:g0 + W] == (win & 0xFF)).all()
            # -Inf (the most violated row there can be) wins its group unless another lane clamps to the same float
            inf_lanes = np.nonzero(np.isneginf(s["key"][g0:g0 + W]) | (s["key"][g0:g0 + W] <= -3.0e38))[0]
            if len(inf_lanes):
                assert (win & 0xFF) in inf_lanes, (backend, W, n, g0, win & 0xFF, inf_lanes)
        assert (out_d[n, D["wave_min"]] == np.nanmin(v)).all(), (backend, W, n)
        t = TABLE.setdefault((backend, "contracts", W), [0, 0])
        t[0] += 64
    _dump(backend)


def test_committed_record_covers_this_table(probe):
    """profiles/wave_isolation.json lists every primitive x W of this module, on this backend, with no lane differing."""
    backend, _ = probe
    with open(os.path.join(ROOT, "profiles", "wave_isolation.json")) as f:
        rec = json.load(f)["primitives"][backend]
    want = {f"{prim}/W{W}" for prim in PRIMITIVES for W in WIDTHS if not (W < 16 and prim in ("value_bcast", "fma_bcast", "bcast_indicator", "bcast_select", "bcast_scale"))}
    assert want <= set(rec), sorted(want - set(rec))
    assert all(v[0] > 0 and v[1] == 0 for k, v in rec.items()), rec
