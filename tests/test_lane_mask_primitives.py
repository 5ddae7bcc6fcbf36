"""The lane-mask primitives of pink_amd/csrc/wave.h -- lane_pred (the inverse ballot: a wave-uniform 64-bit mask as a
per-lane bool) and the builders mask_lane / mask_lanes_below / mask_groups / mask_groups_of_lane for W = 16, 32, 64 --
against plain bit arithmetic in NumPy, exactly.  One probe kernel (tests/wave/lane_mask_probe_kernel.h) is compiled for
gfx950 against wave.h (tests/wave/lane_mask_probe.hip -> tests/wave/liblanemaskprobe.so, built by ``build()``) and into the
emulator library against emu/wave_emu.h (emu/emu_lane_mask_probe.cpp), where lane_pred is a bit test; both face the same
reference.  The existing tests/test_wave_primitives.py and its probe stay as they are.

Masks: none, all, single lanes at the ends of the wave and of every group, alternating bits, one whole group, random ones.
key32_packf_quiet (raw v_min_f32 / v_max_f32 on the device) is held to key32_packf bit for bit over ordinary keys, both
zeros, denormals, both infinities, keys beyond either clamp and quiet NaNs.  The mask is used as the value of a bool, as the condition of a select and of a branch, under lanes_on (EXEC), and goes back
through wave_ballot unchanged."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [16, 32, 64]
FIXED = ["lane_pred", "select", "branch", "ballot_lo", "ballot_hi", "groups", "groups_of_lane", "on_count", "key_packf", "key_quiet"]


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def probe(request, built):
    if request.param == "emu":
        lib, prefix = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libpinkemu.so")), "pinkhip_emu_"
    else:
        lib, prefix = ctypes.CDLL(os.path.join(ROOT, "tests", "wave", "liblanemaskprobe.so")), ""
    run = getattr(lib, prefix + "lane_mask_probe_run")
    run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    return request.param, run, getattr(lib, prefix + "lane_mask_probe_slots")


def _masks(rng, W):
    ng = 64 // W
    m = [0, 2 ** 64 - 1, 1, 1 << 63, 1 << 31, 1 << 32, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFFFFFF, 0xFFFFFFFF00000000]
    for g in range(ng):
        m += [1 << (g * W), 1 << (g * W + W - 1), ((1 << W) - 1) << (g * W) if W < 64 else 2 ** 64 - 1]
    m += [int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) for _ in range(12)]
    return m


@pytest.mark.parametrize("W", WIDTHS)
def test_lane_pred_and_mask_builders(probe, W):
    backend, run, slots = probe
    rng = np.random.default_rng(400 + W)
    ng = 64 // W
    masks = _masks(rng, W)
    sets = len(masks)
    mask = np.array(masks, dtype=np.uint64)
    lo, hi = (mask & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), (mask >> np.uint64(32)).astype(np.uint32).view(np.int32)
    bits = (np.arange(sets) % (1 << ng)).astype(np.int32)  # every per-group bit field, in turn
    bits[-1] = -1  # (bits above the groups are ignored)
    K = rng.integers(0, W, size=sets).astype(np.int32)
    K[:3] = [0, W - 1, W // 2]
    pred = (rng.random((sets, 64)) < 0.5).astype(np.int32)
    pred[0], pred[1] = 0, 1
    ival = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(sets, 64)).astype(np.int32)
    ns = slots(W)
    assert ns == len(FIXED) + 2 * W + 1
    out = np.full((sets, ns, 64), -777, dtype=np.int32)
    # keys for key32_packf against key32_packf_quiet: ordinary negative keys, +-0, denormals, +-inf, beyond both clamps, quiet NaNs
    f32 = np.float32
    special = np.array([0.0, -0.0, 1e-45, -1e-45, -1e-39, np.inf, -np.inf, -3.0e38, -3.4e38, -1.17549435e-38, -1.2e-38, 1.0, np.nan, -np.nan], dtype=f32)
    keys = (-(10.0 ** rng.uniform(-40, 38.5, size=(sets, 64)))).astype(f32)
    keys[:, :len(special)] = special
    keybits = keys.view(np.int32).copy()
    keybits[:, 14], keybits[:, 15] = 0x7FC12345, np.int32(-4194304 + 77)  # quiet NaNs with payload bits, either sign
    arrs = [np.ascontiguousarray(a) for a in (lo, hi, bits, K, pred, ival, keybits)]
    rc = run(W, sets, *[a.ctypes.data for a in arrs], out.ctypes.data)
    assert rc == 0
    assert not (out[:, :len(FIXED)] == -777).any()

    lane = np.arange(64)
    li, g = lane % W, lane // W
    slot = {n: i for i, n in enumerate(FIXED)}
    for s in range(sets):
        p = np.array([(masks[s] >> l) & 1 for l in range(64)], dtype=np.int64)
        what = f"{backend} W={W} set {s} mask {masks[s]:#018x}"
        assert np.array_equal(out[s, slot["lane_pred"]], p), what
        assert np.array_equal(out[s, slot["select"]], np.where(p == 1, ival[s], ~ival[s])), what
        assert np.array_equal(out[s, slot["branch"]].astype(np.int64), (ival[s].astype(np.int64) + p + 2 ** 31) % 2 ** 32 - 2 ** 31), what
        assert (out[s, slot["ballot_lo"]] == lo[s]).all() and (out[s, slot["ballot_hi"]] == hi[s]).all(), what
        gon = (int(bits[s]) >> g) & 1
        assert np.array_equal(out[s, slot["groups"]], gon), what
        flag = pred[s].reshape(ng, W)[:, K[s]]  # lane K of every group
        assert np.array_equal(out[s, slot["groups_of_lane"]], flag[g]), what
        with np.errstate(invalid="ignore"):
            kf = np.fmax(np.fmin(keybits[s].view(f32), f32(-1.17549435e-38)), f32(-3.0e38))  # (fmin / fmax: a NaN loses)
        want = (kf.view(np.int32) & ~np.int32(0xFF)) | li.astype(np.int32)
        assert np.array_equal(out[s, slot["key_packf"]], want), what
        assert np.array_equal(out[s, slot["key_quiet"]], out[s, slot["key_packf"]]), (what, "key32_packf_quiet differs from key32_packf")
        count = pred[s].reshape(ng, W).sum(axis=1)
        assert np.array_equal(out[s, slot["on_count"]], np.where(gon == 1, count[g], -1)), what
        t = len(FIXED)
        for J in range(W):
            assert np.array_equal(out[s, t + J], (li == J).astype(np.int32)), (what, "mask_lane", J)
            assert np.array_equal(out[s, t + W + J], (li < J).astype(np.int32)), (what, "mask_lanes_below", J)
        assert (out[s, t + 2 * W] == 1).all(), (what, "mask_lanes_below(W)")
