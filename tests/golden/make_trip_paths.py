#!/usr/bin/env python3
"""Records tests/golden/trip_paths.npz: what the CPU wave emulator OF A GIVEN COMMIT returns for the runs of
tests/trip_path_cases.py -- dq as raw bits, status, iters, path and the warm kernels' active_out -- with that commit's hash
inside.  tests/test_trip_paths.py asserts that the emulator of the working tree reproduces them bit for bit: splitting the
box-only tableau loop into ordinary and closing trips changes no arithmetic and no decision.

    # in a checkout of the commit to record, after `python __graft_entry__.py`:
    python tests/golden/make_trip_paths.py --emulator tests/emu/libpinkemu.so --murty-emulator tests/emu/libpinkemu_murty.so \
        --commit $(git rev-parse HEAD)

The batches come from tests/trip_path_cases.py of THIS tree (plain NumPy on a seeded generator), the kernels from the
library named by --emulator.

    python tests/golden/make_trip_paths.py --search --emulator <debug library>

finds the seeds of SHAPES: per shape the first seed whose "many" instance makes the most exchanges of its batch, at least
twice the cap of the capped runs, and whose "wrongsign" instance reaches the verdict on a pivot of the wrong sign inside the
tableau loop.  That needs an emulator that says why a group left the tableau, built from emu/ as
__graft_entry__.build_emulator does with -DPINKHIP_SWEEP_DEBUG_WHY -DPINKHIP_SWEEP_NO_HANDOVER added: status 4 and
iters = it + 1000 * (2 + 10 * 3) with it > 0 is "status 3 (not positive definite) set after `it` exchanges"; a non-positive
pivot of the initial sweeps has it = 0.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def search(emu, tp):
    for name, (nv, lead, B, roles, _) in tp.SHAPES.items():
        who = {r: b for b, r in roles.items()}
        for seed in range(400):
            built = tp.make(name, seed)
            r = tp.execute(emu, None, name, 0, False, built)
            its = r["iters"] % 1000
            # the "many" instance makes the most exchanges of its batch, and at least twice the cap of the capped runs
            if its[who["many"]] < 2 * tp.SMALL_CAP or its[who["many"]] < its.max():
                continue
            if "wrongsign" in who:
                b = who["wrongsign"]
                if not (r["status"][b] == 4 and r["iters"][b] // 1000 == 32 and its[b] > 0):
                    continue
            print(f"{name}: seed {seed}: status {r['status'].tolist()} iters {r['iters'].tolist()}")
            break
        else:
            print(f"{name}: no seed below 400")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emulator", required=True, help="libpinkemu.so of the commit to record")
    ap.add_argument("--commit", help="its hash")
    ap.add_argument("--murty-emulator", help="libpinkemu_murty.so of the same commit (__graft_entry__.EMU_VARIANTS; on a commit "
                                             "without it: the g++ lines of build_emulator with that flag added)")
    ap.add_argument("--search", action="store_true", help="find the seeds of the wrong-sign instances (debug emulator)")
    ap.add_argument("-o", default=os.path.join(ROOT, "tests", "golden", "trip_paths.npz"))
    args = ap.parse_args()

    from pink_amd._lib import Desc, Problem, Result
    from tests import trip_path_cases as tp
    from tests.conftest import EmuSolver
    from tests.test_warm_start import EmuWarm

    def load(path):
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.pinkhip_emu_solve_host.argtypes = [ctypes.POINTER(Desc), ctypes.POINTER(Problem), ctypes.POINTER(Result)]
        lib.pinkhip_emu_last_error.restype = ctypes.c_char_p
        return EmuSolver(lib)

    emu = load(args.emulator)
    if args.search:
        return search(emu, tp)
    assert args.commit, "--commit: the hash of the commit whose emulator this is"
    out = {"parent_commit": np.array(args.commit)}
    assert args.murty_emulator, "--murty-emulator: the same commit's emulator with Murty's rule after two trips"
    murty = load(args.murty_emulator)
    todo = [("", emu, r) for r in tp.runs()] + [("murty/", murty, r) for r in tp.runs_murty()]
    for prefix, api, (run, shape, max_iter, warm) in todo:
        r = tp.execute(api, EmuWarm(api), shape, max_iter, warm)
        run = prefix + run
        out[f"{run}/dq_bits"] = np.ascontiguousarray(r["dq"]).view(np.uint64)
        for k in ("status", "iters", "path", "active"):
            if k in r:
                out[f"{run}/{k}"] = np.asarray(r[k])
        print(f"{run:24s} status {r['status'].tolist()} iters {r['iters'].tolist()} path {np.asarray(r['path']).tolist()}")
    np.savez_compressed(args.o, **out)
    print("wrote", args.o, os.path.getsize(args.o), "bytes")


if __name__ == "__main__":
    main()
