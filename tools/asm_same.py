#!/usr/bin/env python3
"""Compare the device assembly of kernels between two builds of one translation unit.

    hipcc ... --cuda-device-only -S a.hip -o before.s ; (the same of the changed tree) -o after.s
    python3 tools/asm_same.py before.s after.s diag_viterbi_kernel

For every kernel whose symbol contains the given substring: the text between its label and its
.Lfunc_end (the instructions and the .amdhsa_kernel descriptor block: registers, LDS, scratch) must be
the same in both files once the function-local label numbers (.LBB<n>_, .Lfunc_end<n>) are normalised.
Prints one line per kernel and exits 1 if any differs or is missing after.  Kernels only the second
file has are listed, not counted.
"""
import re
import sys


def kernels(path, needle):
    text = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(text):
        m = re.match(r"^(\S+):\s*(;.*)?$", text[i])
        if m and needle in m.group(1) and not m.group(1).startswith("."):
            body = []
            i += 1
            while i < len(text) and not text[i].startswith(".Lfunc_end"):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"(BB|\.Lfunc_begin|\.Lfunc_end)\d+", r"\1", text[i])))
                i += 1
            out[m.group(1)] = body
        i += 1
    return out


def main():
    a, b = kernels(sys.argv[1], sys.argv[3]), kernels(sys.argv[2], sys.argv[3])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{'only after ' if name not in a else 'only before'} {name}")
            bad += name in a
            continue
        same = a[name] == b[name]
        print(f"{'same  ' if same else 'DIFFER'} {len(a[name]):6d} lines  {name}")
        bad += not same
    print(f"{len(set(a) & set(b))} kernels compared, {bad} differ or are missing")
    return 1 if bad or not (set(a) & set(b)) else 0


if __name__ == "__main__":
    sys.exit(main())
