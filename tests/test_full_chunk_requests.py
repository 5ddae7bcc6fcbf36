"""The stack + solve kernels request a full chunk of eight task rows from one scalar row pointer, inside one region of the
coordinate lanes, and a partial chunk row by row (pink_amd/csrc/ik_stack_rows.h: PINKHIP_STACK_FULL_CHUNKS): the same loads
from the same addresses.  The cases are those of tests/full_chunk_cases.py -- Kd = 3, 8, 9, 16, 17, 24 rows, B = 1, 3, 5,
weights as one vector and per instance, a zero-weight row (finite, and with a NaN) inside a full chunk, on <30, 0, 32> (nv =
30 and 26), its warm twin, <34, 0, 32> (nv = 33 and 34) and <40, 0, 64>:

  1. the CPU emulator reproduces, bit for bit, what the emulator of the parent commit -- which requested every row on its
     own -- returned (tests/golden/full_chunk_requests.npz, recorded by tests/golden/make_full_chunk_requests.py; the
     parent's hash is inside): dq as raw bits, status, iters, path;
  2. on both backends two runs are bit-equal;
  3. on the GPU the statuses are the recorded ones and dq is within the suite's 1e-10 of the recorded dq wherever the
     instance was solved.  (Emulator and GPU are not compared with each other bit for bit: their reciprocal seeds differ --
     as in tests/test_zero_weight_rows.py.  The GPU's bits against the parent's are compared on the headline batch:
     profiles/full_chunk_requests_ab.json.)"""
import ctypes
import os

import numpy as np
import pytest

from tests import full_chunk_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SWEEP = 3  # host_plan.h PlanKind
TOL = 1e-10  # the suite's bound between two solvers of one QP (tests/test_trip_paths.py)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(ROOT, "tests", "golden", "full_chunk_requests.npz"))


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    from tests.test_warm_start import EmuWarm

    if request.param == "emu":
        emu = request.getfixturevalue("emu")
        return "emu", emu, EmuWarm(emu)
    gpu = request.getfixturevalue("gpu_solver")
    return "gpu", gpu, gpu


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_fixture_names_its_parent(recorded):
    commit = str(recorded["parent_commit"])
    assert len(commit) == 40 and set(commit) <= set("0123456789abcdef")
    assert {k.rsplit("/", 1)[0] for k in recorded.files if "/" in k} == {fc.case_id(c) for c in fc.CASES}


def test_cases_reach_their_instantiations(emu):
    """(of the cases: the host plan sends every shape to the instantiation it is meant for)"""
    from pink_amd._lib import PackedArgs

    emu.lib.pinkhip_emu_plan_solve.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int * 6)]
    for shape in fc.SHAPES:
        for Kd in fc.KDS:
            a = PackedArgs(fc.build((shape, Kd, "vector"))["batch"])
            out = (ctypes.c_int * 6)()
            assert emu.lib.pinkhip_emu_plan_solve(ctypes.byref(a.desc), ctypes.byref(out)) == 0
            assert tuple(out[:4]) == (PLAN_SWEEP,) + fc.INSTANTIATION[shape.rsplit("_B", 1)[0]], (shape, Kd, tuple(out[:4]))


def test_recorded_cases_are_solved_and_the_nan_is_made(recorded):
    """(of the fixture: every finite case is solved in every instance, and the NaN in a zero-weight row reaches the result)"""
    for case in fc.CASES:
        st = recorded[f"{fc.case_id(case)}/status"]
        if case[2] == "zero_row_nan":
            assert st[-1] != 0 and (st[:-1] == 0).all(), (fc.case_id(case), st.tolist())
        else:
            assert (st == 0).all(), (fc.case_id(case), st.tolist())


@pytest.mark.parametrize("case", fc.CASES, ids=[fc.case_id(c) for c in fc.CASES])
def test_case(backend, recorded, case):
    name, solver, warm_api = backend
    run = fc.case_id(case)
    one = fc.execute(solver, warm_api, case)
    two = fc.execute(solver, warm_api, case)
    print(f"{name} {run}: status {one['status'].tolist()} iters {one['iters'].tolist()} path {np.asarray(one['path']).tolist()}")
    for k in one:  # (2)
        assert np.array_equal(_bits(one[k]), _bits(two[k])), (k, "differs between two runs")
    if name == "emu":  # (1)
        assert np.array_equal(np.ascontiguousarray(one["dq"]).view(np.uint64), recorded[f"{run}/dq_bits"]), "dq bits"
        for k in ("status", "iters", "path"):
            assert np.array_equal(np.asarray(one[k]), recorded[f"{run}/{k}"]), k
    else:  # (3)
        st = recorded[f"{run}/status"]
        assert np.array_equal(one["status"], st)
        ref = recorded[f"{run}/dq_bits"].view(np.float64)
        err = float(np.abs(one["dq"][st == 0] - ref[st == 0]).max()) if (st == 0).any() else 0.0
        print(f"   max|dq - dq_recorded| = {err:.3e}")
        assert err < TOL
