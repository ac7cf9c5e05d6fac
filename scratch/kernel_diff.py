#!/usr/bin/env python3
"""kernel_diff.py BUILD_A BUILD_B — are the kernels of two builds the same machine code?

For every *.o of each build directory: every kernel of its gfx950 code object, hashed as bow_amd/csrc/kernel_sha.py hashes the
benched one (machine code + kernel descriptor, entry offset zeroed).  Kernels are matched by mangled symbol ACROSS objects, so
one that moved to another translation unit still matches.  Prints the objects with their kernel counts, every symbol that is
missing from B, new in B or different, and the verdict; exit status 1 unless the two sets are identical.  What a refactor of
device code that must not change an instruction is checked with (host objects differ; cmp of two .o files says nothing)."""
import glob
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bow_amd", "csrc"))
from kernel_sha import all_kernel_identities   # noqa: E402


def build_kernels(build_dir):
    """({symbol: (sha, code_bytes, object)}, {object: kernels}) over the directory's objects"""
    kernels, per_object = {}, {}
    for path in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        obj = os.path.basename(path)
        ids = all_kernel_identities(path)
        per_object[obj] = len(ids)
        for sym, k in ids.items():
            assert sym not in kernels, "%s is defined by %s and %s" % (sym, kernels[sym][2], obj)
            kernels[sym] = (k["sha"], k["code_bytes"], obj)
    return kernels, per_object


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    (a, objs_a), (b, objs_b) = build_kernels(argv[1]), build_kernels(argv[2])
    print("object                     kernels A  kernels B")
    for obj in sorted(set(objs_a) | set(objs_b)):
        if objs_a.get(obj, 0) or objs_b.get(obj, 0):
            print("%-26s %9s  %9s" % (obj, objs_a.get(obj, "-"), objs_b.get(obj, "-")))
    print("%-26s %9d  %9d" % ("total", len(a), len(b)))
    missing = sorted(set(a) - set(b))
    new = sorted(set(b) - set(a))
    moved = sorted(s for s in set(a) & set(b) if a[s][2] != b[s][2])
    different = sorted(s for s in set(a) & set(b) if a[s][:2] != b[s][:2])
    for s in moved:
        print("moved      %s: %s -> %s" % (s, a[s][2], b[s][2]))
    for s in missing:
        print("MISSING    %s (%s)" % (s, a[s][2]))
    for s in new:
        print("NEW        %s (%s)" % (s, b[s][2]))
    for s in different:
        print("DIFFERENT  %s: %s %d bytes (%s) -> %s %d bytes (%s)" % ((s,) + a[s] + b[s]))
    bad = len(missing) + len(new) + len(different)
    print("%d kernels in A, %d in B: %d moved to another object, %d missing, %d new, %d different - %s"
          % (len(a), len(b), len(moved), len(missing), len(new), len(different), "IDENTICAL" if bad == 0 else "NOT identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
