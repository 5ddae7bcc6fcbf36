#!/usr/bin/env python3
"""Records tests/golden/lane_masks.npz: what the CPU wave emulator OF A GIVEN COMMIT returns for the runs of
tests/lane_mask_cases.py -- dq as raw bits, status, iters, path and the warm kernels' active_out -- with that commit's hash
inside.  tests/test_lane_masks.py asserts that the emulator of the working tree reproduces them bit for bit: the lane-mask
form of the tableau kernels' predicates (pink_amd/csrc/wave.h: lane_pred) changes no arithmetic and no decision.

    # in a checkout of the commit to record, after `python __graft_entry__.py`:
    python tests/golden/make_lane_masks.py --emulator tests/emu/libpinkemu.so --commit $(git rev-parse HEAD)

The batches come from tests/lane_mask_cases.py of THIS tree (plain NumPy on a seeded generator), the kernels from the
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
    ap.add_argument("-o", default=os.path.join(ROOT, "tests", "golden", "lane_masks.npz"))
    args = ap.parse_args()

    from pink_amd._lib import Desc, Problem, Result
    from tests import lane_mask_cases as lm
    from tests.conftest import EmuSolver
    from tests.test_warm_start import EmuWarm

    lib = ctypes.CDLL(os.path.abspath(args.emulator))
    lib.pinkhip_emu_solve_host.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Problem), ctypes.POINTER(Result)]
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
    emu = EmuSolver(lib)
    out = {"parent_commit": np.array(args.commit)}
    for run, shape, max_iter, warm in lm.runs():
        r = lm.execute(emu, EmuWarm(emu), shape, max_iter, warm)
        out[f"{run}/dq_bits"] = np.ascontiguousarray(r["dq"]).view(np.uint64)
        for k in ("status", "iters", "path", "active"):
            if k in r:
                out[f"{run}/{k}"] = np.asarray(r[k])
        print(f"{run:24s} status {r['status'].tolist()} iters {r['iters'].tolist()} path {np.asarray(r['path']).tolist()}")
    np.savez_compressed(args.o, **out)
    print("wrote", args.o, os.path.getsize(args.o), "bytes")


if __name__ == "__main__":
    main()
