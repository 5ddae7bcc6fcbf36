"""The stack + solve kernels do not multiply a task row whose weight is exactly zero in every instance of the wave, if every
entry of the row is finite (pink_amd/csrc/ik_stack_rows.h: PINKHIP_STACK_SKIP_ZERO_ROWS; the argument why no bit of any
accumulator can change is in that header).  The cases are those of tests/zero_weight_cases.py:

  1. the CPU emulator reproduces, bit for bit, what the emulator of the parent commit -- which multiplied every row --
     returned (tests/golden/zero_weight_rows.npz, recorded by tests/golden/make_zero_weight_rows.py; the parent's hash is
     inside): dq as raw bits, status, iters, path;
  2. on both backends the finite patterns give, bit for bit, what the same batch gives with the zero-weight rows deleted
     (Kd smaller).  No task has a Levenberg-Marquardt term, so the chain of non-zero rows is the same in both.  One
     exception, in the parent commit as much as here: the entries of H and c among the two eliminated front columns of
     <34, 0, 32> are partial sums per lane, and a deletion that moves a surviving row to another lane of its chunk
     reassociates them (zero_weight_cases.deleted) -- those comparisons are held to the suite's 1e-10 and equal statuses;
  3. on both backends two runs are bit-equal and the statuses are the C oracle's (the finite patterns: what the oracle makes
     of a NaN is its own business);
  4. on the GPU the non-finite patterns -- a zero-weight row that holds inf or NaN, a zero-weight row whose error is NaN:
     rows that must take the ordinary path -- end with the statuses the emulator gave them.

Emulator and GPU are not compared with each other bit for bit: their reciprocal seeds differ."""
import ctypes
import os

import numpy as np
import pytest

from tests import zero_weight_cases as zw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SWEEP = 3  # host_plan.h PlanKind
TOL = 1e-10  # the suite's bound between two solvers of one QP (tests/test_trip_paths.py)


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(ROOT, "tests", "golden", "zero_weight_rows.npz"))


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
    assert {k.rsplit("/", 1)[0] for k in recorded.files if "/" in k} == {zw.case_id(c) for c in zw.CASES}


def test_cases_reach_their_instantiations(emu):
    """(of the cases: the host plan sends every shape to the instantiation it is meant for)"""
    from pink_amd._lib import PackedArgs

    emu.lib.pinkhip_emu_plan_solve.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int * 6)]
    for shape in zw.SHAPES:
        for Kd in zw.KDS:
            a = PackedArgs(zw.build((shape, Kd, "none"))["batch"])
            out = (ctypes.c_int * 6)()
            assert emu.lib.pinkhip_emu_plan_solve(ctypes.byref(a.desc), ctypes.byref(out)) == 0
            assert tuple(out[:4]) == (PLAN_SWEEP,) + zw.INSTANTIATION[shape.rsplit("_B", 1)[0]], (shape, Kd, tuple(out[:4]))


def test_recorded_nonfinite_cases_are_not_solved(recorded):
    """(of the fixture: the non-finite patterns do reach the result -- a skip that ignored them would return status 0)"""
    for case in zw.CASES:
        if case[2] in zw.NONFINITE_PATTERNS:
            st = recorded[f"{zw.case_id(case)}/status"]
            assert (st != 0).any(), (zw.case_id(case), st.tolist())


@pytest.mark.parametrize("case", zw.CASES, ids=[zw.case_id(c) for c in zw.CASES])
def test_case(backend, recorded, case):
    name, solver, warm_api = backend
    run = zw.case_id(case)
    one = zw.execute(solver, warm_api, case)
    two = zw.execute(solver, warm_api, case)
    print(f"{name} {run}: status {one['status'].tolist()} iters {one['iters'].tolist()} path {np.asarray(one['path']).tolist()}")
    for k in one:  # (3)
        assert np.array_equal(_bits(one[k]), _bits(two[k])), (k, "differs between two runs")
    if case[2] in zw.FINITE_PATTERNS:
        ref = zw.oracle(case)
        print(f"   oracle status {ref['status'].tolist()}")
        assert np.array_equal(one["status"], ref["status"])  # (3)
        for idx, batch, exact in zw.deleted(case):  # (2)
            short = zw.execute(solver, warm_api, case, batch)
            if exact:
                for k in one:
                    assert np.array_equal(_bits(np.asarray(one[k])[idx]), _bits(short[k])), (k, idx, "differs from the batch without the zero-weight rows")
            else:
                err = float(np.abs(one["dq"][idx] - short["dq"]).max())
                print(f"   instances {idx}: a surviving row changes its lane, max|dq - dq_deleted| = {err:.3e}")
                assert np.array_equal(one["status"][idx], short["status"]) and err < TOL
    elif name == "gpu":  # (4)
        assert np.array_equal(one["status"], recorded[f"{run}/status"])
    if name == "emu":  # (1)
        assert np.array_equal(np.ascontiguousarray(one["dq"]).view(np.uint64), recorded[f"{run}/dq_bits"]), "dq bits"
        for k in ("status", "iters", "path"):
            assert np.array_equal(np.asarray(one[k]), recorded[f"{run}/{k}"]), k
