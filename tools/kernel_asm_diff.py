#!/usr/bin/env python3
"""Same kernels, same instructions? Compares the gfx950 kernels of two sets of HIP units (CPU only, no GPU needed).

    tools/kernel_asm_diff.py --old old/knn.hip --new csrc/knn.hip csrc/knn_ring16.hip ...

Every .hip file is compiled with the flags of csrc/Makefile plus --cuda-device-only -S (a .s file is taken as it is). The assembly
is cut per kernel symbol; `;` comments and blank lines go, .LBB<n>_ labels become .LBB_ (the number counts the functions of the
unit). Passes when both sides hold the same mangled kernel names and every kernel's body and .amdhsa_ descriptor block
(registers, LDS, scratch) are equal; otherwise names the kernels that differ, with the size of their diff, and exits 1."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "point-cloud-donkey_amd", "csrc")


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch)
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    return [hipcc] + flags.split()


def assembly(path, tmp):
    if path.endswith(".s"):
        return open(path).read()
    out = os.path.join(tmp, "%d.s" % len(os.listdir(tmp)))
    subprocess.check_call(makefile_flags() + ["--cuda-device-only", "-S", path, "-o", out])
    return open(out).read()


def kernels(text):
    """{mangled name: (body lines, descriptor lines)} of one unit's assembly"""
    lines = []
    for ln in text.split("\n"):
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()
        if ln:
            lines.append(ln)
    names = [ln.split()[1] for ln in lines if ln.startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        b0 = lines.index(name + ":") + 1
        d0 = lines.index(".amdhsa_kernel " + name) + 1
        b1 = d0 - 1                                    # the body ends where the descriptor's section begins
        while lines[b1 - 1].startswith((".section", ".p2align")):
            b1 -= 1
        d1 = lines.index(".end_amdhsa_kernel", d0)
        out[name] = (lines[b0:b1], lines[d0:d1])
    return out


def collect(paths, tmp):
    allk = {}
    for p in paths:
        for name, k in kernels(assembly(p, tmp)).items():
            if name in allk:
                sys.exit("kernel defined twice: %s (again in %s)" % (name, p))
            allk[name] = k
    return allk


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True, help=".hip or .s files of the earlier state")
    ap.add_argument("--new", nargs="+", required=True, help=".hip or .s files of the new state")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = collect(a.old, tmp), collect(a.new, tmp)
    bad = 0
    for name in sorted(set(old) - set(new)):
        print("only old:", name); bad += 1
    for name in sorted(set(new) - set(old)):
        print("only new:", name); bad += 1
    n_ins = 0
    for name in sorted(set(old) & set(new)):
        n_ins += len(old[name][0])
        for what, o, n in (("body", old[name][0], new[name][0]), ("descriptor", old[name][1], new[name][1])):
            if o != n:
                d = [x for x in difflib.unified_diff(o, n, lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
                print("differs: %s %s, %d of %d lines" % (name, what, len(d), len(o)))
                bad += 1
    print("%d kernels old, %d new, %d in both (%d body lines): %s" % (len(old), len(new), len(set(old) & set(new)), n_ins,
                                                                     "identical" if not bad else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
