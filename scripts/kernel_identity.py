#!/usr/bin/env python3
"""Is the device code of two builds of the library the same?  Per object of build directory A and its counterpart of
B (names may differ where a refactor renamed objects: --rename): sha256 of the gfx950 code object's .text, the
metadata row of every kernel (scripts/kernel_meta.py) -- and the set of kernel names of the two libraries.

    python scripts/kernel_identity.py A/build A/libpinkhip.so B/build B/libpinkhip.so [--rename RULE] [--per-kernel OBJ] [-o out.json]

--per-kernel OBJ (e.g. pinkhip.o): for an object whose .text differs because kernels were ADDED to it, compare kernel by
kernel -- the instruction text of every kernel symbol of A's object (llvm-objdump -d, addresses dropped) against the
symbol of the same name in B's; the report gains "per_kernel": how many of A's kernels are instruction for instruction
the same, which differ, which are new in B.  Kernels that differ count as a difference; new ones do not.

RULE "legacy": B names objects <prefix>_<NV>_<MD>_<W>.o where A has packed_<NV>_<W>_<DENSE>.o / rollout_<NV>_<W>.o /
wrollout_<NV>_<W>.o.  Exit status 1 when anything differs.
"""
import argparse
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_meta import LLVM, kernels  # noqa: E402

META = ("name", "vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def device_text(path):
    """sha256 of the .text of every gfx950 code object bundled in `path`, and the metadata rows of its kernels"""
    digests = []
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(path))
        shutil.copy(path, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
        for co in sorted(glob.glob(local + ".*gfx950*")):
            subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, co + ".text"], check=True)
            digests.append(hashlib.sha256(open(co + ".text", "rb").read()).hexdigest())
    rows = sorted([k.get(f, "0") for f in META] for k in kernels(path))
    return {"text_sha256": digests, "kernels": rows}


def kernel_disassembly(path):
    """{kernel symbol: sha256 of its instruction text} of the first gfx950 code object bundled in `path`"""
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(path))
        shutil.copy(path, local)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", local], check=True, capture_output=True)
        co = sorted(glob.glob(local + ".*gfx950*"))[0]
        out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for ln in out.splitlines():
        if ln.endswith(">:") and "<" in ln:
            cur = ln.split("<", 1)[1][:-2]
            res[cur] = []
        elif cur and ln.strip():
            res[cur].append(ln.split("//")[0].strip())  # (the address of the instruction is in the trailing comment)
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in res.items()}


def per_kernel(obj_a, obj_b):
    a, b = kernel_disassembly(obj_a), kernel_disassembly(obj_b)
    return {"kernels_of_a": len(a), "of_them_with_identical_disassembly": sum(1 for k in a if b.get(k) == a[k]),
            "differing": sorted(k for k in a if k in b and a[k] != b[k]), "missing_in_b": sorted(k for k in a if k not in b),
            "new_kernels": sorted(k for k in b if k not in a)}


def legacy(name):
    m = re.fullmatch(r"packed_(\d+)_(\d+)_([01])\.o", name)
    if m:
        return f"{'pdense' if m.group(3) == '1' else 'packed'}_{m.group(1)}_0_{m.group(2)}.o"
    m = re.fullmatch(r"(w?rollout)_(\d+)_(\d+)\.o", name)
    return f"{m.group(1)}_{m.group(2)}_0_{m.group(3)}.o" if m else name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("build_a"), ap.add_argument("lib_a"), ap.add_argument("build_b"), ap.add_argument("lib_b")
    ap.add_argument("--rename", choices=["legacy"])
    ap.add_argument("--per-kernel", metavar="OBJ", help="compare this object of A kernel by kernel with its counterpart of B")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    names_a = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.build_a, "*.o")))
    names_b = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.build_b, "*.o")))
    pair = {n: (legacy(n) if a.rename else n) for n in names_a}
    with ThreadPoolExecutor(len(os.sched_getaffinity(0))) as pool:
        da = dict(zip(names_a, pool.map(device_text, [os.path.join(a.build_a, n) for n in names_a])))
        db = dict(zip(names_b, pool.map(device_text, [os.path.join(a.build_b, n) for n in names_b])))
    lib_names = [sorted(k.get("name", "?") for k in kernels(lib)) for lib in (a.lib_a, a.lib_b)]
    report = {"objects": [], "unmatched_a": sorted(n for n in names_a if pair[n] not in db), "unmatched_b": sorted(set(names_b) - set(pair.values())),
              "library_kernel_names": {"a": len(lib_names[0]), "b": len(lib_names[1]), "equal": lib_names[0] == lib_names[1]}}
    for n in names_a:
        if pair[n] in db:
            x, y = da[n], db[pair[n]]
            report["objects"].append({"a": n, "b": pair[n], "text_sha256_a": x["text_sha256"], "text_sha256_b": y["text_sha256"],
                                      "n_kernels": len(x["kernels"]), "text_equal": x["text_sha256"] == y["text_sha256"] and bool(x["text_sha256"]),
                                      "metadata_equal": x["kernels"] == y["kernels"]})
    bad = [o for o in report["objects"] if not (o["text_equal"] and o["metadata_equal"])]
    report["identical"] = not bad and not report["unmatched_a"] and not report["unmatched_b"] and report["library_kernel_names"]["equal"]
    if a.per_kernel:
        pk = per_kernel(os.path.join(a.build_a, a.per_kernel), os.path.join(a.build_b, pair.get(a.per_kernel, a.per_kernel)))
        report["per_kernel"] = dict(object=a.per_kernel, **pk)
        print(f"{a.per_kernel}: {pk['of_them_with_identical_disassembly']} of {pk['kernels_of_a']} kernels identical, differing {pk['differing']}, "
              f"missing {pk['missing_in_b']}, new {pk['new_kernels']}")
        # with the object looked at kernel by kernel, it counts as different only if a kernel of A changed or vanished
        others = [o for o in bad if o["a"] != a.per_kernel]
        report["identical_but_for_new_kernels"] = (not others and not pk["differing"] and not pk["missing_in_b"]
                                                   and not report["unmatched_a"] and not report["unmatched_b"])
    print(f"{len(report['objects'])} objects compared, {len(bad)} differ; unmatched {report['unmatched_a']} / {report['unmatched_b']}; "
          f"library kernel names: {report['library_kernel_names']}")
    for o in bad:
        print("DIFFERS", o["a"], o["b"], "text" if not o["text_equal"] else "", "metadata" if not o["metadata_equal"] else "")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0 if report.get("identical_but_for_new_kernels", report["identical"]) else 1


if __name__ == "__main__":
    sys.exit(main())
