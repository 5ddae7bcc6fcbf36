"""pinkhip_manipulability_task_device -- the ManipulabilityTask row formed on the device -- on the CPU wave emulator and on
the GPU: against 60-digit values of the reference's formula, exact structure, that it writes its own row only, that no
instance's bits depend on who shares its wavefront, and what it refuses."""
import ctypes

import numpy as np
import pytest

from pink_amd._lib import PinkHipError
from pink_amd.rollout import ModelArrays
from tests.manipulability_cases import (CASES, LOCAL, WORLD, bar, configurations, mask_bits, models, note_ratios, with_manipulability,
                                        worst, write_ratios)

SENTINEL = -7.25e300


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    return with_manipulability(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_MANIPULABILITY_RATIOS=<file>: the worst ratios of this run as JSON (profiles/manipulability_exact.json)


def _backend(api):
    return "emu" if "Emu" in type(api).__name__ else "gpu"


def device_row(api, mname, frame, rf, mask, q, rate=0.1, sE=1, sJ=None, row0=0, with_m_out=True, fill=SENTINEL):
    """(e [B, sE], J [B, sJ], m [B]) after the call on buffers filled with ``fill``."""
    model, frames = models()[mname]
    arr = ModelArrays(model, frames)
    B, nv, nq = q.shape[0], model.nv, model.nq
    sJ = nv if sJ is None else sJ
    dm = api.model_create(arr.desc)
    e, J, m = np.full((B, sE), fill), np.full((B, sJ), fill), np.full(B, fill)
    d_q, d_e, d_J, d_m = (api.alloc(8 * n) for n in (B * nq, e.size, J.size, m.size))
    try:
        for p, a in ((d_q, q), (d_e, e), (d_J, J), (d_m, m)):
            api.put(p, a)
        api.manipulability_task(dm, B, d_q, frames.index(frame), int(rf), mask_bits(mask), rate, d_e, sE, d_J, sJ, row0,
                                d_m if with_m_out else None)
        api.sync()
        api.get(e, d_e), api.get(J, d_J), api.get(m, d_m)
    finally:
        for p in (d_q, d_e, d_J, d_m):
            api.release(p)
        api.model_destroy(dm)
    return e, J, m


# ---- 2. exact anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_row_against_60_digits(api, name):
    """m and dm/dq within bar(name) units of u = (what one ulp on q does to the exact result) + eps max|exact|: the project's
    8 where the host class stays below 2, four times the host class's worst ratio elsewhere (tests/manipulability_cases.py)."""
    mname, frame, rf, mask, B, _ = CASES[name]
    q, cond = configurations(name)
    e, J, m = device_row(api, mname, frame, rf, mask, q, rate=0.25)
    rm, rj = worst(name, m, J)
    print(f"{_backend(api):4s} {name:22s} cond <= {cond.max():.2g}  m {rm:.3g}  J {rj:.3g}")
    note_ratios(_backend(api), name, rm, rj)
    assert rm <= bar(name) and rj <= bar(name), (rm, rj, bar(name))
    assert (e == -0.25).all()
    # m_out = NULL changes no bit of e / J
    e1, J1, m1 = device_row(api, mname, frame, rf, mask, q, rate=0.25, with_m_out=False)
    assert e1.tobytes() == e.tobytes() and J1.tobytes() == J.tobytes() and (m1 == SENTINEL).all()


# ---- 3. structure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname, frame", [("tree12", "hand"), ("tree12", "foot"), ("tree36", "hand"), ("tree36", "deep")])
def test_off_path_columns_are_exactly_zero(api, mname, frame):
    model, frames = models()[mname]
    rng = np.random.default_rng(3)
    q = rng.uniform(-2.0, 2.0, size=(3, model.nq))
    mask = "position" if frame != "hand" else None  # (three rows: regular behind four joints and more)
    e, J, m = device_row(api, mname, frame, LOCAL, mask, q)
    on = np.zeros(model.nv, bool)
    j = model.frames[model.getFrameId(frame)].joint
    while j >= 0:
        on[model.joints[j].idx_v] = True
        j = model.joints[j].parent
    assert (J[:, ~on] == 0.0).all() and not np.signbit(J[:, ~on]).any()
    assert (J[:, on] != 0.0).all() and (m > 0.0).all() and np.isfinite(J).all()


def test_singular_A_gives_an_exactly_zero_row(api):
    """tree12's "foot" sits behind four revolute joints: six rows of rank four.  The reference's det there is round-off (m
    may be NaN); here a pivot of L D L^T falls to r eps max A_ii, m = 0 and the row is exactly zero -- LOCAL and WORLD."""
    model, _ = models()["tree12"]
    rng = np.random.default_rng(8)
    q = rng.uniform(-3.0, 3.0, size=(37, model.nq))
    for rf in (LOCAL, WORLD):
        e, J, m = device_row(api, "tree12", "foot", rf, None, q, rate=-0.5)
        assert (J == 0.0).all() and (m == 0.0).all() and (e == 0.5).all()


@pytest.mark.parametrize("name", ["planar2", "arm6", "tree12", "tree36"])
def test_only_its_row_is_written(api, name):
    """Strides larger than natural, row0 = 6, B not a multiple of the robots per wavefront: exactly one entry of e and nv of
    J per instance change -- padded lanes and the robots b >= B of the last wavefront write nothing."""
    mname, frame, rf, mask, _, _ = CASES[name]
    model, _ = models()[mname]
    rng = np.random.default_rng(5)
    B, nv = (13 if name != "tree36" else 2), model.nv
    q = rng.uniform(-2.0, 2.0, size=(B, model.nq))
    sE, sJ, row0 = 6 + 1 + 5, (6 + 1 + 2) * nv + 7, 6
    e0, J0, m0 = device_row(api, mname, frame, rf, mask, q)
    for fill in (SENTINEL, 0.5):  # (two sentinels: a written value equal to one of them cannot hide)
        e, J, m = device_row(api, mname, frame, rf, mask, q, sE=sE, sJ=sJ, row0=row0, fill=fill)
        want_e = np.zeros((B, sE), bool)
        want_e[:, row0] = True
        want_J = np.zeros((B, sJ), bool)
        want_J[:, row0 * nv:(row0 + 1) * nv] = True
        assert np.array_equal(e != fill, want_e) and np.array_equal(J != fill, want_J)
        assert np.array_equal(e[:, row0:row0 + 1], e0) and np.array_equal(J[:, row0 * nv:(row0 + 1) * nv], J0) and np.array_equal(m, m0)


# ---- 4. company -------------------------------------------------------------------------------------------------------------
def test_no_instance_depends_on_who_shares_its_wavefront(api):
    """Every instance of arm6 alone and in every one of the eight slots of a wavefront whose other robots sit at NaN / Inf /
    1e6 rad: the same bits (tests/test_com_task_device.py)."""
    q, _ = configurations("arm6")
    mname, frame, rf, mask, B, _ = CASES["arm6"]
    nq = q.shape[1]
    alone = [device_row(api, mname, frame, rf, mask, q[b:b + 1]) for b in range(B)]
    poison = [np.nan, np.inf, 1e6, -np.inf]
    big = np.empty((B * 8 * 8, nq))
    for b in range(B):
        for s in range(8):
            wave = big[(b * 8 + s) * 8:(b * 8 + s + 1) * 8]
            for o in range(8):
                wave[o] = poison[(o + s + b) % 4]
            wave[s] = q[b]
    e, J, m = device_row(api, mname, frame, rf, mask, big)
    for b in range(B):
        for s in range(8):
            i = (b * 8 + s) * 8 + s
            for got, ref in zip((e[i], J[i], m[i:i + 1]), alone[b]):
                assert got.tobytes() == np.asarray(ref[0]).tobytes(), (b, s)
    assert np.isfinite(J[[(b * 8 + s) * 8 + s for b in range(B) for s in range(8)]]).all()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(api):
    model, frames = models()["tree12"]
    arr = ModelArrays(model, frames)
    B, nv = 3, model.nv
    q = np.zeros((B, model.nq))
    dm = api.model_create(arr.desc)
    e, J = np.full((B, 1), SENTINEL), np.full((B, nv), SENTINEL)
    d_q, d_e, d_J = (api.alloc(8 * n) for n in (q.size, e.size, J.size))
    for p, a in ((d_q, q), (d_e, e), (d_J, J)):
        api.put(p, a)
    good = dict(frame=0, rf=0, mask=63, q=d_q, e=d_e, sE=1, J=d_J, sJ=nv, row0=0)

    def call(**kw):
        a = dict(good, **kw)
        api.manipulability_task(dm, B, a["q"], a["frame"], a["rf"], a["mask"], 0.1, a["e"], a["sE"], a["J"], a["sJ"], a["row0"])

    for bad in (dict(frame=-1), dict(frame=len(frames)), dict(mask=0), dict(mask=64), dict(rf=2), dict(rf=-1), dict(q=None), dict(e=None),
                dict(J=None), dict(row0=-1), dict(sE=0), dict(sJ=nv - 1), dict(row0=1)):
        with pytest.raises(PinkHipError) as ex:
            call(**bad)
        assert ex.value.code == -1, bad
    with pytest.raises(PinkHipError) as ex:  # "deep": a prismatic joint on the path
        call(frame=frames.index("deep"))
    assert ex.value.code == -5 and "revolute" in str(ex.value)
    api.sync()
    api.get(e, d_e), api.get(J, d_J)
    assert (e == SENTINEL).all() and (J == SENTINEL).all()
    api.manipulability_task(dm, 0, d_q, 0, 0, 63, 0.1, d_e, 1, d_J, nv, 0)  # an empty batch is fine
    call()  # ... and "hand", with the prismatic joint on another branch, is served
    api.sync()
    api.get(J, d_J)
    assert np.isfinite(J).all() and (J[:, model.joints[9].idx_v] == 0.0).all()
    for p in (d_q, d_e, d_J):
        api.release(p)
    api.model_destroy(dm)


def test_the_path_check_on_its_own(emu):
    """manip_path_fault (shared by the library and the emulator) without a device model in front of it: PINKHIP_E_UNSUPPORTED
    (-5) for more than 64 joints (such a model has nv > PINKHIP_MAX_NV and cannot be created), for a prismatic joint or a
    free-flyer on the path; 0 for a revolute chain of 64 and for a frame on the world."""
    lib, vp, ci = emu.lib, ctypes.c_void_p, ctypes.c_int
    lib.pinkhip_emu_manipulability_path_check.argtypes = [ci, vp, vp, ci]

    def check(nj, jtype, frame_joint):
        parent = np.arange(-1, nj - 1, dtype=np.int32)
        jt = np.ascontiguousarray(jtype, dtype=np.int32)
        return lib.pinkhip_emu_manipulability_path_check(nj, parent.ctypes.data, jt.ctypes.data, frame_joint)

    assert check(65, np.zeros(65), 64) == -5
    assert check(64, np.zeros(64), 63) == 0 and check(5, np.zeros(5), -1) == 0
    assert check(5, [0, 0, 1, 0, 0], 4) == -5 and check(5, [2, 0, 0, 0, 0], 4) == -5
    assert check(5, [0, 0, 1, 0, 0], 1) == 0  # (the prismatic joint is behind the frame)
