#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel?

    python profiles/kernel_isa_diff.py <tree A> <tree B> [--keep DIR]

Compiles acm_kernels.hip, acm_kernels_f32.hip and acm_parse.hip of both trees with the flags of tests/test_isa_invariants.py
(-O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S), the two kernel files once more with -DACM_TUNING=1, drops comments, .file,
.loc, .ident and debug sections, and compares per kernel: the instruction stream, the kernel descriptor (.amdhsa_* lines: register
counts, LDS size ...) and the metadata record of the kernel.  Kernels are paired by name; a name only one tree has is paired with the
other tree's kernel of the same position in the file and reported as renamed.  Symbol names inside a body are compared after the
same renaming.  Exit status 0: every kernel identical.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

UNITS = [("acm_kernels.hip", []), ("acm_kernels_f32.hip", []), ("acm_parse.hip", []),
         ("acm_kernels.hip", ["-DACM_TUNING=1"]), ("acm_kernels_f32.hip", ["-DACM_TUNING=1"])]


def compile_unit(tree, unit, flags, out):
    if not os.path.exists(out):
        csrc = os.path.join(tree, "libacm_amd", "csrc")
        subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", os.path.join(tree, "include"), "-I", csrc] +
                       flags + [os.path.join(csrc, unit), "-o", out], check=True)
    with open(out) as f:
        return f.read()


def kernels_of(asm):
    """{name: (body lines, descriptor lines)} in file order, and the metadata record per kernel"""
    lines = []
    in_debug = False
    for ln in asm.splitlines():
        s = ln.strip()
        if s.startswith(".section"):
            in_debug = ".debug" in s
        if in_debug or not s or s.startswith((";", "//", ".file", ".loc", ".ident", ".cfi_")):
            continue
        lines.append(re.sub(r"\s*;.*$", "", ln).rstrip())
    out, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(\w+):$", ln)
        if m and not ln.startswith((".L", "$")) and name is None and ("acm_" in ln):
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(ln)
            if ln.strip().startswith(".end_amdhsa_kernel"):
                out[name] = body
                name = None
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", asm, re.M | re.S):
        rec = m.group(0)
        n = re.search(r"^\s+\.name:\s+(\S+)", rec, re.M)
        if n:
            meta[n.group(1)] = [x for x in rec.splitlines() if ".symbol:" not in x and ".name:" not in x]
    return out, meta


def compare(a_asm, b_asm, label, report):
    ka, ma = kernels_of(a_asm)
    kb, mb = kernels_of(b_asm)
    na, nb = list(ka), list(kb)
    if len(na) != len(nb):
        report.append("%s: %d kernels against %d" % (label, len(na), len(nb)))
        return False
    rename = {x: y for x, y in zip(na, nb) if x != y}
    if set(na) - set(nb) != set(rename):
        report.append("%s: the kernels both trees have are not in the same order" % label)
        return False
    ok = True
    pat = re.compile("|".join(re.escape(k) for k in sorted(rename, key=len, reverse=True))) if rename else None
    for x, y in zip(na, nb):
        body = [pat.sub(lambda m: rename[m.group(0)], ln) for ln in ka[x]] if pat else ka[x]
        if body != kb[y] or ma.get(x) != mb.get(y):
            ok = False
            report.append("%s: DIFFERENT %s" % (label, x))
    for x, y in rename.items():
        report.append("%s: renamed %s -> %s" % (label, x, y))
    report.append("%s: %d kernels, %s" % (label, len(na), "identical" if ok else "NOT identical"))
    return ok


def main():
    a, b = sys.argv[1], sys.argv[2]
    keep = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--keep" else "/tmp/kernel_isa_diff"
    jobs = []
    for side, tree in (("a", a), ("b", b)):
        os.makedirs(os.path.join(keep, side), exist_ok=True)
        for unit, flags in UNITS:
            jobs.append((tree, unit, flags, os.path.join(keep, side, unit.replace(".hip", "") + (".tuning" if flags else "") + ".s")))
    with ThreadPoolExecutor(max_workers=5) as ex:
        asm = list(ex.map(lambda j: compile_unit(*j), jobs))
    report, ok = [], True
    for k, (unit, flags) in enumerate(UNITS):
        ok &= compare(asm[k], asm[k + len(UNITS)], unit + (" " + flags[0] if flags else ""), report)
    print("\n".join(report))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
