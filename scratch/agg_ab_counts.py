"""Compares the work two builds put on the GPU for the same script: calls per HIP API name and dispatches per kernel name, from two
`rocprofv3 --hip-trace --kernel-trace --stats --output-format csv -d <dir>` runs.

    python scratch/agg_ab_counts.py <dir of build A> <dir of build B>      (exit code 1 when a count differs)
"""
import csv
import glob
import sys


def counts(root, suffix):
    out = {}
    for path in glob.glob(root + "/**/*" + suffix, recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
    return out


bad = 0
for what, suffix in (("HIP API", "hip_api_stats.csv"), ("kernel", "kernel_stats.csv")):
    a, b = counts(sys.argv[1], suffix), counts(sys.argv[2], suffix)
    assert a and b, "no %s under one of the directories" % suffix
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)}
    print("%s: %d names, %d calls in A, %d in B, %d names differ" % (what, len(set(a) | set(b)), sum(a.values()), sum(b.values()), len(diff)))
    if what == "HIP API":
        for k in ("hipLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipMemcpyAsync", "hipMemsetAsync", "hipStreamSynchronize", "hipEventRecord", "hipMalloc"):
            if k in a or k in b:
                print("   %-26s %8d %8d" % (k, a.get(k, 0), b.get(k, 0)))
    for k, v in diff.items():
        print("   DIFFERS %s: %d against %d" % (k, v[0], v[1]))
    bad += len(diff)
sys.exit(1 if bad else 0)
