"""pinkhip_com_task_device -- the three ComTask rows formed on the device -- on the CPU wave emulator and on the GPU:
against 60-digit values (tests/test_com_task.py builds them), that it writes its own rows only, that no instance's bits
depend on who shares its wavefront, and what it refuses."""
import ctypes

import numpy as np
import pytest

from pink_amd._lib import PinkHipError
from pink_amd.rollout import ModelArrays
from tests.com_task_cases import EPS, K_COM, configurations, models, note_ratios, reference, with_com, worst, write_ratios

SENTINEL = -7.25e300


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    return with_com(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_COM_TASK_RATIOS=<file>: the worst ratios of this run as JSON (profiles/com_task_exact.json)


def _backend(api):
    return "emu" if "Emu" in type(api).__name__ else "gpu"


def device_rows(api, name, q, target, sE=None, sJ=None, row0=0, with_com_out=True, fill=SENTINEL, mass_tables=None):
    """(e [B, sE], J [B, sJ], com [B, 3]) after the call on buffers filled with ``fill``."""
    model, frames = models()[name]
    arr = ModelArrays(model, frames)
    B, nv, nq = q.shape[0], model.nv, model.nq
    sE = 3 if sE is None else sE
    sJ = 3 * nv if sJ is None else sJ
    target = np.ascontiguousarray(target, dtype=np.float64)
    dm = api.model_create(arr.desc)
    dc = api.com_create(dm, *(model.mass_tables() if mass_tables is None else mass_tables))
    e, J, c = np.full((B, sE), fill), np.full((B, sJ), fill), np.full((B, 3), fill)
    d_q, d_t, d_e, d_J, d_c = (api.alloc(8 * n) for n in (B * nq, target.size, e.size, J.size, c.size))
    try:
        for p, a in ((d_q, q), (d_t, target), (d_e, e), (d_J, J), (d_c, c)):
            api.put(p, a)
        api.com_task(dm, dc, B, d_q, d_t, target.ndim == 2, d_e, sE, d_J, sJ, row0, d_c if with_com_out else None)
        api.sync()
        api.get(e, d_e), api.get(J, d_J), api.get(c, d_c)
    finally:
        for p in (d_q, d_t, d_e, d_J, d_c):
            api.release(p)
        api.com_destroy(dc)
        api.model_destroy(dm)
    return e, J, c


# ---- 1. exact anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arm6", "tree12", "tree34", "pend", "chain8", "chain32"])
def test_rows_against_60_digits(api, name):
    """com and J within K_COM = 8 units of u = S + eps max|exact| (what one ulp on the inputs does to the exact result);
    e = com - target to the rounding of that one subtraction."""
    model, _ = models()[name]
    q, _ = reference(name)
    B, nv = q.shape[0], model.nv
    rng = np.random.default_rng(5)
    target = rng.normal(size=(B, 3))
    e, J, c = device_rows(api, name, q, target)
    rc, rj = worst(name, c, J.reshape(B, 3, nv))
    print(f"{_backend(api):4s} {name:7s} com {rc:.3g} J {rj:.3g}")
    note_ratios(_backend(api), name, rc, rj)
    assert rc <= K_COM and rj <= K_COM, (rc, rj)
    # (the device may form c M^-1 - t in one fused operation: half an ulp of c apart from the difference of the rounded c)
    assert (np.abs(e - (c - target)) <= EPS * (np.abs(c) + np.abs(target))).all()
    # one target for all, and no com_out
    e1, J1, c1 = device_rows(api, name, q, target[0], with_com_out=False)
    assert (np.abs(e1 - (c - target[0])) <= EPS * (np.abs(c) + np.abs(target[0]))).all()
    assert np.array_equal(J1, J) and (c1 == SENTINEL).all()
    # exact structure: a column whose subtree is massless is zero; the massless joints themselves change nothing
    sub, _ = model.subtree_tables()
    for k, j in enumerate(model.joints):
        if sub[k] == 0.0:
            assert (J.reshape(B, 3, nv)[:, :, j.idx_v:j.idx_v + j.nv] == 0.0).all()


# ---- 2. only its rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["arm6", "tree12", "tree34", "chain8", "chain32"])
def test_only_its_rows_are_written(api, name):
    """Strides larger than natural, row0 = 6: exactly 3 entries of e and 3 nv of J per instance change -- the lanes of a
    padded group (columns j >= nv, robots b >= B of the last wavefront) write nothing."""
    model, _ = models()[name]
    q = configurations(name)
    B, nv = q.shape[0], model.nv
    sE, sJ, row0 = 6 + 3 + 5, (6 + 3 + 2) * nv + 7, 6
    for fill in (SENTINEL, 0.5):  # (two sentinels: a written value equal to one of them cannot hide)
        e, J, c = device_rows(api, name, q, np.zeros(3), sE=sE, sJ=sJ, row0=row0, fill=fill)
        we, wJ = e != fill, J != fill
        want_e = np.zeros((B, sE), bool)
        want_e[:, row0:row0 + 3] = True
        want_J = np.zeros((B, sJ), bool)
        want_J[:, row0 * nv:(row0 + 3) * nv] = True
        assert np.array_equal(we, want_e) and np.array_equal(wJ, want_J)
        e0, J0, _ = device_rows(api, name, q, np.zeros(3))
        assert np.array_equal(e[:, row0:row0 + 3], e0) and np.array_equal(J[:, row0 * nv:(row0 + 3) * nv], J0)


# ---- 3. company -------------------------------------------------------------------------------------------------------------
def test_no_instance_depends_on_who_shares_its_wavefront(api):
    """Every instance of arm6 alone (a wavefront of its own, its seven other groups idle) and in every one of the eight
    slots of a wavefront whose other robots sit at NaN / Inf / 1e6 rad: the same bits (tests/test_wave_isolation.py)."""
    name = "arm6"
    model, _ = models()[name]
    q = configurations(name)
    B, nq, nv = q.shape[0], model.nq, model.nv
    target = np.array([0.1, -0.2, 0.3])
    alone = [device_rows(api, name, q[b:b + 1], target) for b in range(B)]
    poison = [np.nan, np.inf, 1e6, -np.inf]
    big = np.empty((B * 8 * 8, nq))
    for b in range(B):
        for s in range(8):
            wave = big[(b * 8 + s) * 8:(b * 8 + s + 1) * 8]
            for o in range(8):
                wave[o] = poison[(o + s + b) % 4]
            wave[s] = q[b]
    e, J, c = device_rows(api, name, big, target)
    for b in range(B):
        for s in range(8):
            i = (b * 8 + s) * 8 + s
            for got, ref in zip((e[i], J[i], c[i]), alone[b]):
                assert got.tobytes() == ref[0].tobytes(), (b, s)
    assert np.isfinite(J[[(b * 8 + s) * 8 + s for b in range(B) for s in range(8)]]).all()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(api):
    name = "tree12"
    model, frames = models()[name]
    q = configurations(name)
    mass, com = model.mass_tables()
    with pytest.raises(PinkHipError) as ex:  # zero total mass
        device_rows(api, name, q, np.zeros(3), mass_tables=(np.zeros_like(mass), com))
    assert ex.value.code == -1 and "total mass" in str(ex.value)
    for bad in (np.where(np.arange(len(mass)) == 1, np.inf, mass), np.where(np.arange(len(mass)) == 1, -1.0, mass)):
        with pytest.raises(PinkHipError) as ex:
            device_rows(api, name, q, np.zeros(3), mass_tables=(bad, com))
        assert ex.value.code == -1
    with pytest.raises(PinkHipError) as ex:  # tables of another length than the model's
        device_rows(api, name, q, np.zeros(3), mass_tables=(mass[:-1], com[:-1]))
    assert ex.value.code == -1 and "nj" in str(ex.value)
    with pytest.raises(ValueError):  # mass and com that disagree
        device_rows(api, name, q, np.zeros(3), mass_tables=(mass, com[:-1]))
    # NULL pointers: nothing is launched, the buffers keep their sentinel
    arr = ModelArrays(model, frames)
    B, nv = q.shape[0], model.nv
    dm = api.model_create(arr.desc)
    dc = api.com_create(dm, mass, com)
    e, J = np.full((B, 3), SENTINEL), np.full((B, 3 * nv), SENTINEL)
    d_q, d_t, d_e, d_J = (api.alloc(8 * n) for n in (q.size, 3, e.size, J.size))
    for p, a in ((d_q, q), (d_t, np.zeros(3)), (d_e, e), (d_J, J)):
        api.put(p, a)
    for args in ((None, d_t, False, d_e, 3, d_J, 3 * nv, 0), (d_q, None, False, d_e, 3, d_J, 3 * nv, 0),
                 (d_q, d_t, False, None, 3, d_J, 3 * nv, 0), (d_q, d_t, False, d_e, 3, None, 3 * nv, 0),
                 (d_q, d_t, False, d_e, 3, d_J, 3 * nv, -1), (d_q, d_t, False, d_e, 2, d_J, 3 * nv, 0)):
        with pytest.raises(PinkHipError) as ex:
            api.com_task(dm, dc, B, *args)
        assert ex.value.code == -1
    with pytest.raises(PinkHipError):
        api.com_task(dm, None, B, d_q, d_t, False, d_e, 3, d_J, 3 * nv, 0)
    api.sync()
    api.get(e, d_e), api.get(J, d_J)
    assert (e == SENTINEL).all() and (J == SENTINEL).all()
    api.com_task(dm, dc, 0, d_q, d_t, False, d_e, 3, d_J, 3 * nv, 0)  # an empty batch is fine
    for p in (d_q, d_t, d_e, d_J):
        api.release(p)
    api.com_destroy(dc)
    api.model_destroy(dm)


def test_more_than_64_joints_never_reach_the_kernel(api):
    """One lane per joint: 64 at the most.  A model with more joints has nv > PINKHIP_MAX_NV = 64 and is refused when
    its device model is created (PINKHIP_E_INVALID), in front of pinkhip_com_create's own check."""
    from pink_amd import build_chain

    arr = ModelArrays(build_chain(65, mass_seed=1), ["tool0"])
    with pytest.raises(RuntimeError, match=r"nv must be in 1\.\.PINKHIP_MAX_NV") as ex:
        api.model_create(arr.desc)
    if _backend(api) == "gpu":  # (the library's error type carries the code; the emulator's test harness raises RuntimeError)
        assert type(ex.value) is PinkHipError and ex.value.code == -1
    else:
        assert type(ex.value) is RuntimeError


def test_the_mass_tables_own_refusals(emu):
    """pinkhip_com_create's checks (build_com_image, shared by the library and the emulator) without a device model in
    front of them: PINKHIP_E_UNSUPPORTED (-5) for more than 64 joints, PINKHIP_E_INVALID (-1) for a length that is not
    the model's, NULL tables, a total mass that is not positive; 0 for a valid chain of 64."""
    lib, vp, ci = emu.lib, ctypes.c_void_p, ctypes.c_int
    lib.pinkhip_emu_com_image_check.argtypes = [ci, vp, ci, vp, vp]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p

    def check(model_nj, nj, mass=None, null=False):
        parent = np.arange(-1, model_nj - 1, dtype=np.int32)
        mass = np.ones(nj) if mass is None else np.asarray(mass, dtype=np.float64)
        com = np.zeros((nj, 3))
        rc = lib.pinkhip_emu_com_image_check(model_nj, parent.ctypes.data, nj, None if null else mass.ctypes.data, com.ctypes.data)
        return rc, lib.pinkhip_emu_last_error().decode()

    rc, why = check(65, 65)
    assert rc == -5 and "nj <= 64" in why
    assert check(64, 64)[0] == 0
    assert check(12, 11)[0] == -1 and check(12, 12, null=True)[0] == -1
    assert check(12, 12, mass=np.zeros(12))[0] == -1 and check(12, 12, mass=np.r_[np.ones(11), np.nan])[0] == -1
