"""The C-ABI library: it loads, exports what include/pinkhip.h declares, validates
descriptors, and refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from pink_amd import _lib
from pink_amd._lib import PackedArgs, PinkHipError
from tests.cases import config_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(built):
    header = open(os.path.join(ROOT, "include", "pinkhip.h")).read()
    declared = sorted(set(re.findall(r"\b(pinkhip_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    assert sorted(_lib.ABI_SYMBOLS) == declared
    lib = _lib.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pinkhip_version() == 112


def test_struct_layouts_match_the_header(built):
    # pinkhip_desc: 8 + 6*4 + 5*8 + 4(+4 pad) + 2*8 + 2*8 + 2*4
    assert ctypes.sizeof(_lib.Desc) == 8 + 24 + 40 + 8 + 16 + 16 + 8 + 8  # (+ n_free_lead and its padding, round 6)
    assert ctypes.sizeof(_lib.Problem) == 64 and ctypes.sizeof(_lib.Result) == 24
    assert ctypes.sizeof(_lib.DeviceInfo) == 4 * 4 + 2 * 8 + 128 + 64


def test_no_gpu_means_loud_failure(built):
    lib = _lib.load_library()
    n = ctypes.c_int(-1)
    rc = lib.pinkhip_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible here")
    from pink_amd.batch_solver import BatchSolver

    with pytest.raises(PinkHipError) as ei:
        BatchSolver(0)
    assert ei.value.code == -4  # PINKHIP_E_NODEVICE


def test_descriptor_validation(emu):
    def err(mutate):
        batch, _ = config_case("ur5", "tight", "dense", 2)  # fresh arrays: mutations must not leak
        a = PackedArgs(batch)
        mutate(a)
        dq = np.zeros((2, 6)); st = np.zeros(2, np.int32)
        r = _lib.Result(); r.dq, r.status = dq.ctypes.data, st.ctypes.data
        p = a.host_problem()
        rc = emu.lib.pinkhip_emu_solve_host(ctypes.byref(a.desc), ctypes.byref(p), ctypes.byref(r))
        return rc, emu.lib.pinkhip_emu_last_error().decode()

    assert err(lambda a: None)[0] == 0
    for mut, word in [
        (lambda a: setattr(a.desc, "nv", 65), "nv"),
        (lambda a: setattr(a.desc, "md", 65), "md"),
        (lambda a: setattr(a.desc, "n_eq", 1), "n_eq"),
        (lambda a: setattr(a.desc, "dt", 0.0), "dt"),
        (lambda a: setattr(a.desc, "K", 13), "task_rows"),
        (lambda a: setattr(a.desc, "Kd", 5), "Kd"),
        (lambda a: a.task_kind.__setitem__(0, 1), "dense task"),
        (lambda a: a.task_col0.__setitem__(1, 3), "exceeds"),
    ]:
        rc, msg = err(mut)
        assert rc == -1 and re.search(word, msg), (rc, msg)


def test_host_plan_invariants(tmp_path):
    """emu/host_plan_check.cpp, built with the address and undefined-behaviour sanitizers and run as a child process:
    whatever host_plan.h plans for nv = 1..64 x md x n_free_lead x B x PINKHIP_SOLVER, cold and warm, and for the whole-step
    kernel, holds the problem, covers B, is an entry of its X-macro table and fits the LDS; the warm refusals are refused."""
    import subprocess

    exe = str(tmp_path / "host_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wno-psabi", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "emu", "host_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "checks passed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def _print_objects(*args):
    import subprocess

    out = subprocess.run(["make", "-s", "print-objects", *args], cwd=os.path.join(ROOT, "pink_amd", "csrc"), capture_output=True, text=True, check=True)
    return out.stdout.split()


def test_makefile_builds_every_instantiation_of_the_dispatch_table():
    """dispatch.h (PINKHIP_FAMILIES and its tables) is the single source of the instantiations; the Makefile has to compile
    one object per entry of every family or the link fails only on the GPU box.  It derives them with the preprocessor
    (`make print-objects`): held here to the tables as written, and to the development rule for three DEV builds."""
    src = open(os.path.join(ROOT, "pink_amd", "csrc", "dispatch.h")).read()

    def table(name):
        t = src[src.rindex(f"#define {name}(X)"):]  # (the real tables follow the development ones)
        t = t[:re.search(r"\n(?!\s*X\()", t).start()]  # the define and its continuation lines
        return re.findall(r"X\((\d+), (\d+), (\d+)\)", t)

    families = re.findall(r"^\s*F\((PLAN_\w+), ([01]), (\w+), (\w+), (PINKHIP_\w+_TABLE)\)", src, re.M)
    by_prefix = {prefix: table(tab) for _, _, prefix, _, tab in families}
    assert sorted(by_prefix) == sorted(["rdense", "rpairs", "rollout", "wrollout", "sweepx", "sweep", "wsweep", "packed", "pdense"]) and len(families) == 9
    objs = _print_objects()
    want = [f"{prefix}_{nv}_{md}_{w}.o" for prefix, t in by_prefix.items() for nv, md, w in t]
    assert len(objs) == len(set(objs)) and sorted(objs) == sorted(want + ["pinkhip.o"])
    # the whole-step kernels are started first, each family from its largest entry
    assert objs[0] == "rdense_56_8_64.o" and objs[-1] == "pinkhip.o" and objs.index("rollout_56_0_64.o") < objs.index("sweep_64_0_64.o") < objs.index("sweep_8_0_16.o")

    pairs = [(nv, w) for nv, md, w in by_prefix["packed"]]
    assert by_prefix["pdense"] == by_prefix["packed"] and all(md == "0" for _, md, _ in by_prefix["packed"]) and len(pairs) >= 11
    for nv, w in pairs:
        assert int(w) >= int(nv) and int(nv) % 2 == 0 and 64 % int(w) == 0
    # the whole-control-step kernel: a subset of the table (groups of whole 16-lane rows), one unit each
    rpairs = [(nv, w) for nv, md, w in by_prefix["rollout"]]
    assert all(md == "0" for _, md, _ in by_prefix["rollout"]) and len(rpairs) >= 10
    assert set(rpairs) <= set(pairs) and all(int(w) >= 16 for _, w in rpairs)
    # the sweep-tableau kernel: one unit per (NV, MD, W) of PINKHIP_SWEEP_TABLE, NV + MD tableau rows on W lanes
    triples, dense, virtual = by_prefix["sweep"], by_prefix["rdense"], by_prefix["sweepx"]
    assert len(triples) >= 20 and len(dense) >= 4 and len(virtual) >= 3
    # ... and with virtual dense rows (ik_sweepx.h): NV coordinates on W lanes, MD rows in a second role of the first MD lanes
    for nv, md, w in virtual:
        assert int(nv) <= int(w) and 1 <= int(md) <= 16 and int(nv) % 2 == 0 and int(w) in (16, 32, 64)
    # (the sphere-pair kernels are whole-step kernels with dense rows: held to the same rule)
    for nv, md, w in triples + dense + by_prefix["rpairs"]:
        # one lane per tableau row, or (whole-step kernel only) virtual dense rows in an instantiated shape
        # ... or (round 6, box-only stack + solve kernel) at most two leading coordinates eliminated before the solve: NV - W
        eliminated = int(md) == 0 and 0 < int(nv) - int(w) <= 2 and (nv, md, w) in triples
        assert (int(nv) + int(md) <= int(w) or (nv, md, w) in virtual or eliminated) and int(nv) % 2 == 0 and int(w) in (16, 32, 64)
    assert all(int(md) > 0 for _, md, _ in dense + by_prefix["rpairs"]) and set(by_prefix["rpairs"]) <= set(dense) and len(by_prefix["rpairs"]) >= 3
    # the warm-start twins: box-only, each the twin of an entry of the cold table
    assert set(by_prefix["wsweep"]) <= set(triples) and set(by_prefix["wrollout"]) <= set(by_prefix["rollout"])
    assert all(md == "0" for _, md, _ in by_prefix["wsweep"] + by_prefix["wrollout"]) and len(by_prefix["wsweep"]) >= 5 and len(by_prefix["wrollout"]) >= 4

    # development builds: one instantiation per family that can hold it (the PINKHIP_DEV_NV block of dispatch.h)
    assert sorted(_print_objects("DEV=1")) == sorted(
        ["packed_30_0_32.o", "pdense_30_0_32.o", "rollout_30_0_32.o", "sweep_30_0_32.o", "wsweep_30_0_32.o", "wrollout_30_0_32.o", "pinkhip.o"])
    assert sorted(_print_objects("DEV=1", "DEVNV=50", "DEVMD=6", "DEVW=64")) == sorted(
        ["packed_50_0_64.o", "pdense_50_0_64.o", "rollout_50_0_64.o", "sweep_50_6_64.o", "sweepx_50_6_64.o", "rdense_50_6_64.o", "pinkhip.o"])
    # (more coordinates than lanes: front coordinates eliminated in the tableau kernels, the others hold all of them on 64 lanes)
    assert sorted(_print_objects("DEV=1", "DEVNV=34", "DEVW=32")) == sorted(
        ["packed_34_0_64.o", "pdense_34_0_64.o", "rollout_34_0_64.o", "sweep_34_0_32.o", "wsweep_34_0_32.o", "wrollout_34_0_64.o", "pinkhip.o"])


def test_emulator_has_a_lane_entry_for_every_table_entry(emu):
    """Every entry of every family of PINKHIP_FAMILIES has a registered lane entry in the emulator (a missing one used to
    surface only when some parity case happened to plan it), and the emulator was compiled with the tables `make` builds."""
    emu.lib.pinkhip_emu_table_text.restype = ctypes.c_char_p
    rows = [ln.split() for ln in emu.lib.pinkhip_emu_table_text().decode().splitlines()]
    assert len(rows) >= 81 and all(len(r) == 7 for r in rows)
    assert [r for r in rows if r[6] != "1"] == []
    assert sorted(f"{r[0]}_{r[3]}_{r[4]}_{r[5]}.o" for r in rows) == sorted(o for o in _print_objects() if o != "pinkhip.o")
    assert {r[0]: r[2] for r in rows}["pdense"] == "1" and sum(r[2] == "1" for r in rows) == sum(r[0] == "packed" for r in rows)


def test_headline_kernel_has_no_register_spills(built):
    """Code-generation guard: the fully unrolled register-resident tableau is fragile under the register allocator
    (a second back edge in the active-set loop once cost 145 register moves per trip and 41 spilled registers: 0.74 ->
    1.12 ms per 65 536).  The headline instantiation must keep its rows in registers."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_meta.py"),
                          os.path.join(ROOT, "pink_amd", "csrc", "build", "sweep_30_0_32.o")], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-objdump / llvm-readelf not available: " + out.stderr[-200:])
    row = [ln for ln in out.stdout.splitlines() if "ik_solve_sweep_kernel<30, 0, 32>" in ln]
    assert row, out.stdout
    f = row[0].split()
    vgpr, vspill = int(f[-7]), int(f[-4])
    # (the dozen spilled registers belong to the hand-over to the Goldfarb-Idnani code at the end of the kernel, which
    # runs for groups whose result failed its certificate; the tableau loop itself has none: checked in the ISA when
    # the hand-over was added, 0.667 -> 0.680 ms with the certificate's extra closing trip)
    assert vspill <= 16 and vgpr <= 168, row[0]


def test_tableau_rows_stay_in_registers(built):
    """Round 5: the tableau rows of the 32- and 64-lane kernels live in 1024-bit VGPR tuples so that a column of a
    run-time index is a register read (TabRegs, csrc/ik_common.h).  When the optimiser gets to rewrite "load the tuple,
    extract element p" as a scalar load at a run-time address, the tuples never become registers and the kernel reads its
    tableau from SCRATCH memory -- correct results, a fraction of the speed, silently (it happened to the ik_sweepx.h
    instantiations and to a 512-bit last tuple while this was written).  A tuple in memory shows as a private segment of
    hundreds of bytes that no spilled register accounts for."""
    import glob
    import subprocess
    import sys

    objs = sorted(glob.glob(os.path.join(ROOT, "pink_amd", "csrc", "build", "sweep_*.o")) + glob.glob(os.path.join(ROOT, "pink_amd", "csrc", "build", "sweepx_*.o"))
                  + glob.glob(os.path.join(ROOT, "pink_amd", "csrc", "build", "rollout_*.o")) + glob.glob(os.path.join(ROOT, "pink_amd", "csrc", "build", "rdense_*.o")))
    assert len(objs) >= 30
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_meta.py")] + objs, capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-objdump / llvm-readelf not available: " + out.stderr[-200:])
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("ik_")]
    assert len(rows) >= 30, out.stdout[-2000:]
    # private segment beyond what the spilled registers account for (4 bytes each): an array or a tuple kept in memory
    excess = lambda f: int(f[-2]) - 4 * int(f[-4])  # noqa: E731  (columns: ... vspill sspill scratch lds)
    worst = max(rows, key=excess)
    assert excess(worst) < 128, " ".join(worst)  # (one 1024-bit tuple per lane is 128 bytes)


def test_no_device_function_is_called(built):
    """Everything that touches the dynamic LDS has to be inlined into its kernel: as a *called* function the body of
    the sweep-tableau kernel reached the LDS through the per-kernel offset table LLVM builds for that case and faulted on
    the first access (the largest instantiations, once the hand-over to the Goldfarb-Idnani code made the body too big
    for the inliner).  No code object of the library may contain a call."""
    import glob
    import shutil
    import subprocess
    import tempfile

    llvm = "/opt/rocm/lib/llvm/bin"
    lib = os.path.join(ROOT, "pink_amd", "csrc", "libpinkhip.so")
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
        objects = sorted(glob.glob(local + ".*gfx950*"))
        assert objects
        from concurrent.futures import ThreadPoolExecutor

        def calls(co):  # (awk keeps the pipe small: the disassembly of one code object is tens of megabytes)
            out = subprocess.run(f"{llvm}/llvm-objdump -d {co} | awk '/s_swappc/{{c++}} /v_/{{v++}} END{{print c+0, v+0}}'",
                                 shell=True, capture_output=True, text=True).stdout.split()
            return int(out[0]), int(out[1])

        with ThreadPoolExecutor(max_workers=os.cpu_count() or 4) as pool:
            counts = list(pool.map(calls, objects))
        assert sum(v for _, v in counts) > 100000  # (the disassembler did run)
        assert all(c == 0 for c, _ in counts), [(os.path.basename(o), c) for o, (c, _) in zip(objects, counts) if c]
