#!/usr/bin/env python3
"""Same device code, per kernel: compares the gfx950 code objects of two source trees.

    tools/kernel_identity.py PARENT_TREE BRANCH_TREE [-j JOBS]

For each tree, every unit of the Makefile's KERNEL_OBJS and PREP_OBJS is compiled with the flags of the Makefile's rule
for its list (PREP_OBJS: without -ffp-contract=off) plus --cuda-device-only, the gfx950 object is unbundled and disassembled.  The comparison is per kernel symbol and ACROSS
files (a kernel may have moved to another unit): the two symbol sets, and for each symbol the sequence of instruction
encodings and the resources of its kernel descriptor (VGPRs, SGPRs, LDS, scratch).  Needs no GPU.  Exit status 0 iff
the sets are equal and every kernel is identical; a kernel that differs is shown side by side, instruction by
instruction, with its instruction counts and resources.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
CSRC = os.path.join("matrixfactorizationsgd.java_amd", "csrc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(cmd, cwd=None):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.exit(f"{' '.join(cmd)} failed:\n{p.stdout}")
    return p.stdout


def make_var(csrc, name):
    return run(["make", "-s", "-C", csrc, f"print-{name}"]).split()


def disassemble(csrc, unit, flags, hipcc, work):
    """One unit -> ({kernel symbol: [(encoding, text)]}, {kernel symbol: {resource: value}})."""
    bundle, obj = os.path.join(work, unit + ".bundle"), os.path.join(work, unit + ".gfx950.o")
    run([hipcc, *flags, "--cuda-device-only", "-c", unit + ".hip", "-o", bundle], cwd=csrc)
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
         f"--input={bundle}", f"--output={obj}"])
    code, sym = {}, None
    for line in run([os.path.join(LLVM, "llvm-objdump"), "-d", obj]).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            code[sym] = []
            continue
        m = re.match(r"^\s+(.*?)\s*// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)", line)
        if m and sym is not None:
            code[sym].append((m.group(2).strip(), " ".join(m.group(1).split())))
    # amdhsa.kernels: one record per kernel, "  - .key: value" opening it and "    .key: value" continuing it
    res, rec = {}, None
    for line in run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj]).splitlines():
        m = re.match(r"^  (- |  )(\.[a-z_]+):\s+(\S+)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            rec = {}
        if rec is None:
            continue
        if m.group(2) == ".name":
            res[m.group(3).strip("'\"")] = rec
        elif m.group(2) in RESOURCES:
            rec[m.group(2)] = m.group(3)
    kernels = {s: c for s, c in code.items() if s in res}  # (leaves out local labels and device functions)
    return unit, kernels, {s: dict(sorted(res[s].items())) for s in kernels}


def tree_kernels(tree, jobs, work):
    csrc = os.path.join(tree, CSRC)
    cxx = make_var(csrc, "CXXFLAGS")
    # the Makefile's two lists of device units and what its rule for each adds to CXXFLAGS
    lists = (("KERNEL_OBJS", make_var(csrc, "HIPFLAGS")), ("PREP_OBJS", ["--offload-arch=" + make_var(csrc, "ARCH")[0]]))
    units = [(o[:-2], cxx + extra) for name, extra in lists for o in make_var(csrc, name)]
    hipcc = make_var(csrc, "HIPCC")[0]
    os.makedirs(work, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(lambda uf: disassemble(csrc, uf[0], uf[1], hipcc, work), units))


def merge(units):
    code, res, where = {}, {}, {}
    for unit, k, r in units:
        for sym in k:
            # a library's kernel template (rocPRIM's) that several units instantiate is compared per unit: each unit
            # compiles its own copy, under its own flags
            s = f"{sym} [{unit}.hip]" if "rocprim" in sym else sym
            if s in code:
                sys.exit(f"kernel {s} is in two units: {where[s]}.hip and {unit}.hip")
            code[s], res[s], where[s] = k[sym], r[sym], unit
    return code, res, where


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(2) as ex:
        fa = ex.submit(tree_kernels, a.parent, max(1, a.jobs // 2), os.path.join(tmp, "parent"))
        fb = ex.submit(tree_kernels, a.branch, max(1, a.jobs - a.jobs // 2), os.path.join(tmp, "branch"))
        (ca, ra, wa), (cb, rb, wb) = merge(fa.result()), merge(fb.result())
    bad = 0
    for s in sorted(set(ca) - set(cb)):
        print(f"ONLY IN PARENT ({wa[s]}.hip): {s}")
        bad += 1
    for s in sorted(set(cb) - set(ca)):
        print(f"ONLY IN BRANCH ({wb[s]}.hip): {s}")
        bad += 1
    same = 0
    for s in sorted(set(ca) & set(cb)):
        ea, eb = [e for e, _ in ca[s]], [e for e, _ in cb[s]]
        if ea == eb and ra[s] == rb[s]:
            same += 1
            continue
        bad += 1
        print(f"DIFFERS: {s}\n  parent {wa[s]}.hip: {len(ea)} instructions, {ra[s]}\n"
              f"  branch {wb[s]}.hip: {len(eb)} instructions, {rb[s]}")
        if len(ea) == len(eb):
            for x, (p, b) in enumerate(zip(ca[s], cb[s])):
                if p[0] != b[0]:
                    print(f"    [{x}] {p[1]}  |  {b[1]}")
    per_unit = {}
    for s in cb:
        per_unit[wb[s]] = per_unit.get(wb[s], 0) + 1
    print(f"parent: {len(ca)} kernels; branch: {len(cb)} kernels "
          f"({', '.join(f'{u}.hip {n}' for u, n in sorted(per_unit.items()))}); identical: {same}; not: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
