"""The box-only tableau loop makes its ordinary trips `while some group of the wave exchanges` and its closing trips in a loop
of their own (pink_amd/csrc/ik_sweep.h: PINKHIP_SWEEP_SPLIT_CLOSING).  That may not change any arithmetic, any decision or
the order of the exchanges:

  * the CPU emulator reproduces, bit for bit, what the emulator of the parent commit returned for the runs of
    tests/trip_path_cases.py (tests/golden/trip_paths.npz, recorded by tests/golden/make_trip_paths.py; the parent's hash is
    inside) -- dq as raw bits, status, iters, path, the warm kernels' active_out;
  * on both backends every run agrees with the C oracle (pink/solve_ik.py:206-275 through Goldfarb-Idnani) to the suite's
    1e-10 wherever both solve, has the oracle's statuses under the default cap, and gives bit-equal results when run twice.
    Emulator and GPU are not compared with each other bit for bit: their reciprocal seeds differ;
  * the code objects of the headline instantiation and of its warm twin use no more registers, spills or scratch than the
    parent's (the AMDGPU metadata notes, as scripts/kernel_meta.py reads them; no instruction is inspected).

What makes neighbours in one wave differ -- nothing to exchange, many exchanges, the iteration cap, routed, a pivot of the
wrong sign inside the loop -- is listed in tests/trip_path_cases.py.  Murty's least-index rule starts after 4 nv + 20 trips,
which no batch here makes: the uncapped runs are repeated on a second build of the emulator in which it starts after two
(__graft_entry__.EMU_VARIANTS), again bit for bit against the parent's sources built the same way."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import trip_path_cases as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
RUNS = tp.runs()
MANY = 2 * tp.SMALL_CAP  # exchanges that count as "many": twice what the capped runs allow, and the most of its batch


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(ROOT, "tests", "golden", "trip_paths.npz"))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    from tests.test_warm_start import EmuWarm

    if request.param == "emu":
        emu = request.getfixturevalue("emu")
        return "emu", emu, EmuWarm(emu)
    gpu = request.getfixturevalue("gpu_solver")
    return "gpu", gpu, gpu


def test_fixture_names_its_parent(recorded):
    commit = str(recorded["parent_commit"])
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef")
    want = {r[0] for r in RUNS} | {"murty/" + r[0] for r in tp.runs_murty()}
    assert {k.rsplit("/", 1)[0] for k in recorded.files if "/" in k} == want


@pytest.mark.parametrize("run,shape,max_iter,warm", RUNS, ids=[r[0] for r in RUNS])
def test_run(backend, recorded, run, shape, max_iter, warm):
    name, solver, warm_api = backend
    one = tp.execute(solver, warm_api, shape, max_iter, warm)
    two = tp.execute(solver, warm_api, shape, max_iter, warm)
    ref = tp.oracle(shape)
    roles = tp.build(shape)[3]
    who = {r: b for b, r in roles.items()}
    solved = (ref["status"] == 0) & (one["status"] == 0)
    err = float(np.abs(one["dq"][solved] - ref["dq"][solved]).max())
    print(f"{name} {run}: max|dq - dq_ref| = {err:.3e} over {int(solved.sum())} instances, status {one['status'].tolist()}, "
          f"oracle {ref['status'].tolist()}, iters {one['iters'].tolist()}, path {np.asarray(one['path']).tolist()}")
    # neighbours in different states
    assert one["status"][who["none"]] == 0 and one["iters"][who["none"]] == 0 and one["path"][who["none"]] == 0
    if max_iter == 0:
        assert np.array_equal(one["status"], ref["status"])
        assert solved.sum() >= len(solved) - 1  # (all but the instance whose H is singular)
        if not warm:
            on_tableau = np.asarray(one["path"]) == 0
            assert one["iters"][who["many"]] >= MANY and one["iters"][who["many"]] == one["iters"][on_tableau].max() and on_tableau[who["many"]]
        if "routed" in who:
            assert one["path"][who["routed"]] == 2 and one["status"][who["routed"]] == 0  # off the tableau before its loop
        if "wrongsign" in who:
            # H is indefinite: the tableau's verdict inside its loop, confirmed by the Goldfarb-Idnani code's Cholesky
            # factorisation.  (That the verdict falls inside the loop and not in the initial sweeps -- both end here -- is what
            # the seed of the shape was searched for with a debug build: tests/golden/make_trip_paths.py --search.)
            assert one["path"][who["wrongsign"]] == 1 and one["status"][who["wrongsign"]] == 3
    else:
        assert (one["status"] == 1).any() and (one["status"] == 0).any()  # a capped group next to a converged one
    assert err < TOL
    for k in one:
        assert np.array_equal(np.asarray(one[k]).view(np.uint8), np.asarray(two[k]).view(np.uint8)), (k, "differs between two runs")
    if name == "emu":
        assert np.array_equal(np.ascontiguousarray(one["dq"]).view(np.uint64), recorded[f"{run}/dq_bits"]), "dq bits"
        for k in ("status", "iters", "path", "active"):
            if k in one:
                assert np.array_equal(np.asarray(one[k]), recorded[f"{run}/{k}"]), k


# ---------------------------------------------------------------------------------------------- Murty's least-index rule
@pytest.fixture(scope="module")
def emu_murty(built):
    import ctypes

    from pink_amd._lib import Desc, Problem, Result
    from tests.conftest import EmuSolver

    lib = ctypes.CDLL(built.build_emulator(variant="murty"))
    lib.pinkhip_emu_solve_host.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Problem), ctypes.POINTER(Result)]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
    return EmuSolver(lib)


MURTY_RUNS = tp.runs_murty()


@pytest.mark.parametrize("run,shape,max_iter,warm", MURTY_RUNS, ids=[r[0] for r in MURTY_RUNS])
def test_murty_run(emu_murty, recorded, run, shape, max_iter, warm):
    """The switch to the least index inside the split loop: the same bits as the parent's single loop, and the oracle's
    minimiser wherever both solve (the rule changes the path, not the point)."""
    from tests.test_warm_start import EmuWarm

    one = tp.execute(emu_murty, EmuWarm(emu_murty), shape, max_iter, warm)
    ref = tp.oracle(shape)
    solved = (ref["status"] == 0) & (one["status"] == 0)
    err = float(np.abs(one["dq"][solved] - ref["dq"][solved]).max())
    print(f"murty {run}: max|dq - dq_ref| = {err:.3e} over {int(solved.sum())} instances, status {one['status'].tolist()}, "
          f"iters {one['iters'].tolist()} (default rule: {recorded[run + '/iters'].tolist()}), path {np.asarray(one['path']).tolist()}")
    assert np.array_equal(one["status"], ref["status"])
    assert err < TOL
    assert np.array_equal(np.ascontiguousarray(one["dq"]).view(np.uint64), recorded[f"murty/{run}/dq_bits"]), "dq bits"
    for k in ("status", "iters", "path", "active"):
        if k in one:
            assert np.array_equal(np.asarray(one[k]), recorded[f"murty/{run}/{k}"]), k


def test_murty_rule_is_reached(recorded):
    """(of the fixture: with the rule after two trips the exchange counts are not the default rule's)"""
    differ = [r[0] for r in MURTY_RUNS if not np.array_equal(recorded[f"murty/{r[0]}/iters"], recorded[f"{r[0]}/iters"])]
    print("runs whose exchange counts change under the least-index rule:", differ)
    assert {"nv34_lead6", "nv50_a", "nv50_b", "nv30_warm"} <= set(differ)


# ---------------------------------------------------------------------------------------------- static guard: registers
LLVM = "/opt/rocm/lib/llvm/bin"
# the parent commit's figures: VGPRs, spilled VGPRs, spilled SGPRs, scratch bytes
PARENT_META = {"sweep_30_0_32.o": (168, 4, 0, 20), "wsweep_30_0_32.o": (168, 6, 0, 28)}


def _meta(path, tmp):
    """(vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size) of the one kernel of an object file."""
    local = os.path.join(tmp, os.path.basename(path))
    shutil.copy(path, local)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
    found = []
    for co in sorted(glob.glob(local + ".*gfx950*")):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .")[1:]:
            f = dict(re.findall(r"\.?(\w+):\s+(\S+)", "." + block))
            if "vgpr_count" in f:
                found.append(tuple(int(f.get(k, "0")) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")))
    assert len(found) == 1, found
    return found[0]


@pytest.mark.parametrize("obj", sorted(PARENT_META))
def test_no_more_registers_than_the_parent(built, tmp_path, obj):
    path = os.path.join(ROOT, "pink_amd", "csrc", "build", obj)
    if not os.path.exists(path):  # (a library that was copied in without its objects: one make target)
        subprocess.run(["make", os.path.join("build", obj)], cwd=os.path.dirname(os.path.dirname(path)), check=True, capture_output=True)
    now = _meta(path, str(tmp_path))
    print(f"{obj}: vgpr, spilled vgpr, spilled sgpr, scratch bytes = {now}, parent {PARENT_META[obj]}")
    assert all(n <= p for n, p in zip(now, PARENT_META[obj])), (now, PARENT_META[obj])
