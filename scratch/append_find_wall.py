"""Wall time of AppendBows and Bow.FindNext on the device at 1e8 rows, device-resident, every output allocated ONCE outside the timed
region (the ctypes arguments are built outside it too), each next to its comparator in the same run:
    bowgpu_append of two pieces of rows/2 (Int64 + Float64 with 30 % nulls)   vs  bowgpu_diff over the same two columns of the result
    the same frame as pieces of 4096 rows and as pieces of 1000 rows         over the two-piece time (no bar fixed in advance)
    bowgpu_find_next, Int64: hit at row 0, at row n-1, absent                 vs  bowgpu_is_col_sorted on the same column (one full read);
                                                                                  the row-0 case also against a call at 1000 rows
One process; run it under a time limit:
    timeout -k 10 600 python scratch/append_find_wall.py [rows [section]]
Per-kernel times come from a profiler run of one section, e.g. rocprofv3 --kernel-trace --stats -d DIR -- python scratch/append_find_wall.py 1e8 append
Warm-up call, then REPS timed calls: median and min .. max.  "Not slower" means: the median is within the comparator's min .. max."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ONLY = sys.argv[2] if len(sys.argv) > 2 else None      # append / find
REPS = 5
print("device: %s   rows: %d" % (capi.device_name(), n))
rng = np.random.default_rng(7)


def timeit(fn, reps=REPS):
    fn(); capi.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    return wall[len(wall) // 2], wall[0], wall[-1]


def show(label, t):
    print("  %-58s median %8.3f ms   (min %.3f .. max %.3f)" % ((label,) + t))


def verdict(what, ours, theirs_median, theirs_max):
    ok = ours[0] <= theirs_max
    print("  -> %s: %.3f ms against %.3f ms (max %.3f): %s" % (what, ours[0], theirs_median, theirs_max, "WITHIN" if ok else "MISSED"))


def device_col(values, valid=None):
    n_ = len(values)
    typ = capi.INT64 if values.dtype == np.int64 else capi.FLOAT64
    v = capi.DeviceBuffer.from_numpy(values)
    if valid is None:
        return capi.Column(v, None, typ, 0, n_, 0)
    b = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(valid, bitorder="little"), np.zeros(8, np.uint8)]))
    return capi.Column(v, b, typ, 0, n_, int(n_ - valid.sum()))


def pieces_of(cols, rows):
    """the frame as pieces of `rows` rows (the last one short): slices of the same buffers by Arrow offset; null_count -1 where there
    is a bitmap.  Returns the ctypes arguments of bowgpu_append (built once) and what keeps them alive"""
    cuts = list(range(0, n, rows)) + [n]
    flat = (capi.Col * (len(cols) * (len(cuts) - 1)))()
    ptrs = (C.POINTER(capi.Col) * (len(cuts) - 1))()
    base = [c.c() for c in cols]
    stride = C.sizeof(capi.Col) * len(cols)
    for f in range(len(cuts) - 1):
        for i, b in enumerate(base):
            s = flat[f * len(cols) + i]
            s.values, s.validity, s.type, s.residency = b.values, b.validity, b.type, b.residency
            s.offset, s.length, s.null_count = cuts[f], cuts[f + 1] - cuts[f], (-1 if b.validity else 0)
        ptrs[f] = C.cast(C.addressof(flat) + f * stride, C.POINTER(capi.Col))
    return ptrs, len(cuts) - 1, flat


if not ONLY or ONLY == "append":
    print("\nAppendBows: Int64 + Float64 with 30 %% nulls, %d rows in all (8 B read and 8 B written per row and column)" % n)
    valid = rng.random(n) >= 0.3
    cols = [device_col(np.arange(n, dtype=np.int64)), device_col(rng.standard_normal(n), valid)]
    nulls = int(n - valid.sum())
    del valid
    outs = [capi.OutColumn(n, capi.DEVICE) for _ in range(2)]
    outs_d = [capi.OutColumn(n, capi.DEVICE) for _ in range(2)]
    oarr = (capi.Out * 2)(outs[0].c(), outs[1].c())
    unchanged = C.c_int32(0)
    times = {}
    for label, rows in (("two pieces", (n + 1) // 2), ("pieces of 4096 rows", 4096), ("pieces of 1000 rows", 1000)):
        ptrs, k, keep = pieces_of(cols, rows)

        def append():
            capi.check(capi.lib().bowgpu_append(ptrs, k, 2, oarr, C.byref(unchanged)))

        times[label] = timeit(append)
        assert (oarr[0].length, oarr[1].length, oarr[0].null_count, oarr[1].null_count) == (n, n, 0, nulls)
        assert capi.checksum64(outs[0].values, n) == capi.checksum64(cols[0].values, n)      # the frame itself comes back
        assert capi.checksum64(outs[1].validity, n // 64) == capi.checksum64(cols[1].validity, n // 64)
        show("bowgpu_append, %s (%d)" % (label, k), times[label])
        del ptrs, keep
    for o, a in zip(outs, oarr):
        o.absorb(a)
    appended = [capi.out_as_column(o) for o in outs]
    d = timeit(lambda: capi.diff(appended, outs=outs_d))
    show("bowgpu_diff over the two columns of the appended frame", d)
    two = times["two pieces"]
    print("  append, two pieces: %.2f TB/s by 16 B per row and column over the wall time" % (2 * 16 * n / (two[0] * 1e-3) / 1e12))
    verdict("Append (two pieces) not slower than Diff", two, d[0], d[2])
    for label in ("pieces of 4096 rows", "pieces of 1000 rows"):
        print("  -> %s: %.2fx the two-piece time%s" % (label, times[label][0] / two[0], "" if times[label][0] <= 1.25 * two[0] else "  (above 1.25x)"))
    del cols, outs, outs_d, appended

if not ONLY or ONLY == "find":
    print("\nBow.FindNext: one Int64 column without nulls, %d rows" % n)
    vals = np.arange(n, dtype=np.int64) * 2
    col = device_col(vals)
    small = device_col(vals[:1000].copy())
    del vals
    first = timeit(lambda: capi.find_next(col, 0))
    last = timeit(lambda: capi.find_next(col, 2 * (n - 1)))
    absent = timeit(lambda: capi.find_next(col, 1))
    assert (capi.find_next(col, 0), capi.find_next(col, 2 * (n - 1)), capi.find_next(col, 1)) == (0, n - 1, -1)
    s = timeit(lambda: capi.is_col_sorted(col))
    tiny = timeit(lambda: capi.find_next(small, 1998))
    show("bowgpu_find_next, hit at row 0", first)
    show("bowgpu_find_next, hit at row n-1", last)
    show("bowgpu_find_next, absent", absent)
    show("bowgpu_is_col_sorted (one full read)", s)
    show("bowgpu_find_next at 1000 rows, device-resident", tiny)
    print("  find, absent: %.2f TB/s by 8 B per row over the wall time" % (8 * n / (absent[0] * 1e-3) / 1e12))
    verdict("FindNext (absent) within IsColSorted", absent, s[0], s[2])
    verdict("FindNext (last row) within IsColSorted", last, s[0], s[2])
    verdict("FindNext (row 0) under twice a 1000-row call", first, 2 * tiny[0], 2 * tiny[0])
