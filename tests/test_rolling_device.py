"""pinkhip_rolling_tasks_device -- the RollingTask / OmniwheelTask rows of up to eight wheels formed on the device in one
launch -- on the CPU wave emulator and on the GPU: against 60-digit values (tests/rolling_cases.py builds them), the exact
structure of the rows, that it writes its own rows only, that one launch equals one launch per wheel, that no instance's
bits depend on who shares its wavefront, and what it refuses."""
import ctypes

import numpy as np
import pytest

from pink_amd._lib import PinkHipError
from tests.rolling_cases import (K_ROLL, OMNI, ROLLING, WIDTH, arrays, configurations, models, note_ratios, reference, reference_bar, rows_of,
                                 with_rolling, worst, write_ratios)

SENTINEL = -7.25e300
NAMES = ["cart", "biped", "quad", "tree34", "chain8", "chain32"]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def api(request):
    return with_rolling(request.getfixturevalue("emu" if request.param == "emu" else "gpu_solver"))


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    write_ratios()  # PINK_ROLLING_TASK_RATIOS=<file>: the worst ratios of this run as JSON (profiles/rolling_task_exact.json)


def _backend(api):
    return "emu" if "Emu" in type(api).__name__ else "gpu"


def device_rows(api, name, q, wheels=None, sE=None, sJ=None, row0=0, with_height=True, fill=SENTINEL, kinds=None, radii=None, into=None):
    """(e [B, sE], J [B, sJ], z [B, n]) after ONE call for the wheels ``wheels`` (indices into the model's; default all) on
    buffers filled with ``fill`` -- or on the arrays ``into = (e, J, z)`` of an earlier call."""
    model, all_wheels = models()[name]
    wheels = list(range(len(all_wheels))) if wheels is None else list(wheels)
    kinds = [all_wheels[w][0] for w in wheels] if kinds is None else kinds
    radii = [all_wheels[w][3] for w in wheels] if radii is None else radii
    arr = arrays(name)
    B, nv, nq, n, nr = q.shape[0], model.nv, model.nq, len(wheels), rows_of(kinds)
    sE = nr if sE is None else sE
    sJ = nr * nv if sJ is None else sJ
    dm = api.model_create(arr.desc)
    e, J, z = (np.full((B, sE), fill), np.full((B, sJ), fill), np.full((B, n), fill)) if into is None else into
    d_q, d_e, d_J, d_z = (api.alloc(8 * k) for k in (B * nq, e.size, J.size, z.size))
    try:
        for p, a in ((d_q, q), (d_e, e), (d_J, J), (d_z, z)):
            api.put(p, a)
        api.rolling_tasks(dm, B, d_q, wheels, kinds, radii, d_e, sE, d_J, sJ, row0, d_z if with_height else None)
        api.sync()
        api.get(e, d_e), api.get(J, d_J), api.get(z, d_z)
    finally:
        for p in (d_q, d_e, d_J, d_z):
            api.release(p)
        api.model_destroy(dm)
    return e, J, z


# ---- 1. exact anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_against_60_digits(api, name):
    """e, J and the heights within K_ROLL = 8 units of u = S + eps max|exact| (what one ulp on the inputs, radius included,
    does to the exact result) -- four times the reference class's own ratio where that sits above 2 units -- and the
    exact structure: off-path columns == 0.0, the in-plane error entries == 0.0."""
    model, wheels = models()[name]
    arr = arrays(name)
    q, _ = reference(name)
    B, nv = q.shape[0], model.nv
    kinds = [w[0] for w in wheels]
    nr = rows_of(kinds)
    bar_e, bar_j = reference_bar(name)
    e, J, z = device_rows(api, name, q)
    J = J.reshape(B, nr, nv)
    re, rj, rz = worst(name, e, J, z)
    print(f"{_backend(api):4s} {name:7s} W {WIDTH[name]:2d} e {re:.3g} J {rj:.3g} z {rz:.3g} (bars {bar_e:.3g} {bar_j:.3g} {K_ROLL:.3g})")
    note_ratios(_backend(api), name, re, rj, rz)
    assert re <= bar_e and rj <= bar_j and rz <= K_ROLL, (re, rj, rz)
    row = 0
    for w, kind in enumerate(kinds):
        k = 2 if kind == OMNI else 3
        path, j = set(), int(arr.frame_joint[w])
        while j >= 0:
            path.add(j)
            j = model.joints[j].parent
        off = [c for i, jt in enumerate(model.joints) if i not in path for c in range(jt.idx_v, jt.idx_v + jt.nv)]
        assert (J[:, row:row + k][:, :, off] == 0.0).all()
        assert (e[:, row:row + k - 1] == 0.0).all() and (e[:, row + k - 1] != 0.0).all()
        row += k


@pytest.mark.parametrize("name", ["biped", "quad"])
def test_omniwheel_rows_are_rows_0_and_2_of_a_rolling_wheel(api, name):
    """Bit for bit, for every wheel of the model taken once as either kind."""
    model, wheels = models()[name]
    q = configurations(name)
    B, nv = q.shape[0], model.nv
    n = len(wheels)
    e3, J3, z3 = device_rows(api, name, q, kinds=[ROLLING] * n)
    e2, J2, z2 = device_rows(api, name, q, kinds=[OMNI] * n)
    J3, J2 = J3.reshape(B, 3 * n, nv), J2.reshape(B, 2 * n, nv)
    keep = [3 * w + r for w in range(n) for r in (0, 2)]
    assert J2.tobytes() == np.ascontiguousarray(J3[:, keep]).tobytes() and e2.tobytes() == np.ascontiguousarray(e3[:, keep]).tobytes()
    assert z2.tobytes() == z3.tobytes()


# ---- 2. only its rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_only_its_rows_are_written(api, name):
    """Strides larger than natural, row0 = 6: exactly nr entries of e and nr nv of J per instance change -- the padded lanes of
    a group and the robots b >= B of the last wavefront write nothing; height_out = NULL leaves that buffer alone."""
    model, wheels = models()[name]
    q = configurations(name)
    B, nv = q.shape[0], model.nv
    nr = rows_of([w[0] for w in wheels])
    sE, sJ, row0 = 6 + nr + 5, (6 + nr + 2) * nv + 7, 6
    e0, J0, z0 = device_rows(api, name, q)
    for fill in (SENTINEL, 0.5):  # (two sentinels: a written value equal to one of them cannot hide)
        e, J, z = device_rows(api, name, q, sE=sE, sJ=sJ, row0=row0, fill=fill, with_height=False)
        want_e = np.zeros((B, sE), bool)
        want_e[:, row0:row0 + nr] = True
        want_J = np.zeros((B, sJ), bool)
        want_J[:, row0 * nv:(row0 + nr) * nv] = True
        assert np.array_equal(e != fill, want_e) and np.array_equal(J != fill, want_J)
        assert (z == fill).all()
        assert np.array_equal(e[:, row0:row0 + nr], e0) and np.array_equal(J[:, row0 * nv:(row0 + nr) * nv], J0)


@pytest.mark.parametrize("name", ["biped", "quad", "tree34"])
def test_one_launch_equals_one_launch_per_wheel(api, name):
    """n wheels in one launch, and n launches of one wheel each at the matching row0 into the same buffers: the same bits."""
    model, wheels = models()[name]
    q = configurations(name)
    B, nv = q.shape[0], model.nv
    kinds = [w[0] for w in wheels]
    nr = rows_of(kinds)
    e, J, z = device_rows(api, name, q)
    bufs = (np.full((B, nr), SENTINEL), np.full((B, nr * nv), SENTINEL), np.full((B, 1), SENTINEL))
    row, zs = 0, []
    for w, kind in enumerate(kinds):
        device_rows(api, name, q, wheels=[w], sE=nr, sJ=nr * nv, row0=row, into=bufs)
        zs.append(bufs[2][:, 0].copy())
        row += 2 if kind == OMNI else 3
    assert bufs[0].tobytes() == e.tobytes() and bufs[1].tobytes() == J.tobytes()
    assert np.stack(zs, axis=1).tobytes() == z.tobytes()


# ---- 3. company -------------------------------------------------------------------------------------------------------------
def test_no_instance_depends_on_who_shares_its_wavefront(api):
    """Every instance of the biped alone (a wavefront of its own, its seven other groups idle) and in every one of the eight
    slots of a wavefront whose other robots sit at NaN / Inf / 1e6 rad: the same bits (tests/test_wave_isolation.py), and
    finite rows."""
    name = "biped"
    model, _ = models()[name]
    q = configurations(name)
    B, nq = q.shape[0], model.nq
    alone = [device_rows(api, name, q[b:b + 1]) for b in range(B)]
    poison = [np.nan, np.inf, 1e6, -np.inf]
    big = np.empty((B * 8 * 8, nq))
    for b in range(B):
        for s in range(8):
            wave = big[(b * 8 + s) * 8:(b * 8 + s + 1) * 8]
            for o in range(8):
                wave[o] = poison[(o + s + b) % 4]
            wave[s] = q[b]
    e, J, z = device_rows(api, name, big)
    for b in range(B):
        for s in range(8):
            i = (b * 8 + s) * 8 + s
            for got, ref in zip((e[i], J[i], z[i]), alone[b]):
                assert got.tobytes() == ref[0].tobytes(), (b, s)
    own = [(b * 8 + s) * 8 + s for b in range(B) for s in range(8)]
    assert np.isfinite(J[own]).all() and np.isfinite(e[own]).all() and np.isfinite(z[own]).all()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(api):
    """Each refusal of the header's table returns its code and touches nothing; B = 0 is fine."""
    from pink_amd.rollout import ModelArrays

    name = "biped"
    model, wheels = models()[name]
    q = configurations(name)
    B, nv, nr = q.shape[0], model.nv, 5
    # slot 2 of this model is an ordinary slot: it has no root
    arr = ModelArrays(model, [(w[1], w[2]) for w in wheels] + ["base"])
    dm = api.model_create(arr.desc)
    e, J, z = np.full((B, nr), SENTINEL), np.full((B, nr * nv), SENTINEL), np.full((B, 2), SENTINEL)
    d_q, d_e, d_J, d_z = (api.alloc(8 * k) for k in (q.size, e.size, J.size, z.size))
    for p, a in ((d_q, q), (d_e, e), (d_J, J), (d_z, z)):
        api.put(p, a)
    S, K, R = [0, 1], [ROLLING, OMNI], [0.1, 0.07]
    ok = (dm, B, d_q, S, K, R, d_e, nr, d_J, nr * nv, 0, d_z)

    def call(**kw):
        names = ("model", "B", "q", "slots", "kinds", "radii", "e", "sE", "J", "sJ", "row0", "z")
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        api.rolling_tasks(*args)

    invalid = [dict(q=None), dict(e=None), dict(J=None),
               dict(slots=[], kinds=[], radii=[]), dict(slots=[0] * 9, kinds=[0] * 9, radii=[0.1] * 9),  # n outside 1..8
               dict(slots=[0, 3]), dict(slots=[-1, 1]),  # a slot outside the model
               dict(slots=[0, 2]),  # a slot without a root
               dict(kinds=[ROLLING, 2]), dict(kinds=[-1, OMNI]),
               dict(radii=[0.1, np.nan]), dict(radii=[np.inf, 0.07]),
               dict(row0=-1), dict(sE=nr - 1), dict(sJ=nr * nv - 1), dict(row0=1)]  # (row0 = 1: the strides no longer hold the rows)
    for kw in invalid:
        with pytest.raises(PinkHipError) as ex:
            call(**kw)
        assert ex.value.code == -1, kw
    with pytest.raises(PinkHipError) as ex:
        call(model=None)
    assert ex.value.code == -1
    api.sync()
    api.get(e, d_e), api.get(J, d_J), api.get(z, d_z)
    assert (e == SENTINEL).all() and (J == SENTINEL).all() and (z == SENTINEL).all()
    call(B=0)  # an empty batch is fine ...
    call(B=0, q=None, e=None, J=None)  # ... whatever the pointers
    api.sync()
    api.get(e, d_e), api.get(J, d_J)
    assert (e == SENTINEL).all() and (J == SENTINEL).all()
    call()  # and the valid call writes every row
    api.sync()
    api.get(e, d_e), api.get(J, d_J), api.get(z, d_z)
    assert (e != SENTINEL).all() and (J != SENTINEL).all() and (z != SENTINEL).all()
    for p in (d_q, d_e, d_J, d_z):
        api.release(p)
    api.model_destroy(dm)


def test_more_than_64_joints_are_unsupported(emu):
    """One lane per joint: PINKHIP_E_UNSUPPORTED (-5) for nj > 64, from the check the library and the emulator share
    (rolling_task_fault).  A model with more than 64 joints has nv > PINKHIP_MAX_NV and cannot be created, so the check is
    asked about a bare joint count."""
    lib = emu.lib
    lib.pinkhip_emu_rolling_joint_check.argtypes = [ctypes.c_int]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
    assert lib.pinkhip_emu_rolling_joint_check(64) == 0
    assert lib.pinkhip_emu_rolling_joint_check(65) == -5 and "nj <= 64" in lib.pinkhip_emu_last_error().decode()
