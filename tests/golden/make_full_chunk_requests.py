#!/usr/bin/env python3
"""Records tests/golden/full_chunk_requests.npz: what the CPU wave emulator OF A GIVEN COMMIT returns for the cases of
tests/full_chunk_cases.py -- dq as raw bits, status, iters, path -- with that commit's hash inside.
tests/test_full_chunk_requests.py asserts that the emulator of the working tree reproduces them bit for bit: requesting a
full chunk of task rows from one scalar row pointer changes no bit of the result.

    # in a checkout of the commit to record, after `python __graft_entry__.py`:
    python tests/golden/make_full_chunk_requests.py --emulator tests/emu/libpinkemu.so --commit $(git rev-parse HEAD)

The batches come from tests/full_chunk_cases.py of THIS tree (plain NumPy on a seeded generator), the kernels from the
library named by --emulator.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emulator", required=True, help="libpinkemu.so of the commit to record")
    ap.add_argument("--commit", required=True, help="its hash")
    ap.add_argument("-o", default=os.path.join(ROOT, "tests", "golden", "full_chunk_requests.npz"))
    args = ap.parse_args()

    from pink_amd._lib import Desc, Problem, Result
    from tests import full_chunk_cases as fc
    from tests.conftest import EmuSolver
    from tests.test_warm_start import EmuWarm

    lib = ctypes.CDLL(os.path.abspath(args.emulator))
    lib.pinkhip_emu_solve_host.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Problem), ctypes.POINTER(Result)]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
    emu = EmuSolver(lib)
    out = {"parent_commit": np.array(args.commit)}
    for case in fc.CASES:
        r = fc.execute(emu, EmuWarm(emu), case)
        run = fc.case_id(case)
        out[f"{run}/dq_bits"] = np.ascontiguousarray(r["dq"]).view(np.uint64)
        for k in ("status", "iters", "path"):
            out[f"{run}/{k}"] = np.asarray(r[k])
        print(f"{run:40s} status {r['status'].tolist()} iters {r['iters'].tolist()} path {np.asarray(r['path']).tolist()}")
    np.savez_compressed(args.o, **out)
    print("wrote", args.o, os.path.getsize(args.o), "bytes")


if __name__ == "__main__":
    main()
