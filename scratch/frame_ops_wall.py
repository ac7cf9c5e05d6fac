"""Wall time of Bow.Diff, Bow.DropNils and Bow.Distinct on the device at 1e8 rows, device-resident, every output allocated ONCE outside
the timed region, each next to its comparator in the same run:
    bowgpu_diff of one Float64 column with 30 % nulls         vs  bowgpu_fill (FillPrevious) of the same column
    bowgpu_drop_nils of a three-column frame, p = 0.01 / 0.5   vs  bowgpu_filter over an Int64 predicate column that selects the same rows
    bowgpu_distinct, 1000 values shuffled                      vs  bowgpu_argsort + bowgpu_take, + one bowgpu_compact of a one-column frame
    bowgpu_distinct, a sorted timestamp column                 vs  bowgpu_is_col_sorted + that compaction
One process; run it under a time limit:
    timeout -k 10 900 python scratch/frame_ops_wall.py [rows [section]]
Per-kernel times come from a profiler run of one section, e.g. rocprofv3 --kernel-trace --stats -d DIR -- python scratch/frame_ops_wall.py 1e8 diff
Warm-up call, then REPS timed calls: median and min .. max.  "Not slower" means: the median is within the comparator's min .. max."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ONLY = sys.argv[2] if len(sys.argv) > 2 else None      # diff / drop / distinct
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


def same(a, b, k):
    assert (a.length, a.null_count) == (b.length, b.null_count)
    assert capi.checksum64(a.values, k) == capi.checksum64(b.values, k)
    assert capi.checksum64(a.validity, k // 64, 0) == capi.checksum64(b.validity, k // 64, 0)


if not ONLY or ONLY == "diff":
    print("\nBow.Diff: one Float64 column, 30 % nulls (8 B read and 8 B written per row)")
    col = device_col(rng.standard_normal(n), rng.random(n) >= 0.3)
    out_d, out_f = capi.OutColumn(n, capi.DEVICE), capi.OutColumn(n, capi.DEVICE)

    def fill_previous():
        o, c, u = out_f.c(), col.c(), C.c_int32(0)
        capi.check(capi.lib().bowgpu_fill(C.byref(c), capi.FILL["Previous"], C.byref(o), C.byref(u)))

    d = timeit(lambda: capi.diff([col], outs=[out_d]))
    f = timeit(fill_previous)
    show("bowgpu_diff", d)
    show("bowgpu_fill (FillPrevious)", f)
    print("  diff: %.2f TB/s by 16 B/row + the bitmaps over the wall time" % ((16 * n + n // 4) / (d[0] * 1e-3) / 1e12))
    verdict("Diff not slower than FillPrevious", d, f[0], f[2])
    del col, out_d, out_f

if not ONLY or ONLY == "drop":
    ts = device_col(np.arange(n, dtype=np.int64))
    v1 = device_col(rng.standard_normal(n))
    outs = [capi.OutColumn(n, capi.DEVICE) for _ in range(3)]
    outs_f = [capi.OutColumn(n, capi.DEVICE) for _ in range(3)]
    for p in (0.01, 0.5):
        valid = rng.random(n) >= p
        k = int(valid.sum())
        v2 = device_col(rng.standard_normal(n), valid)
        key = device_col(np.where(valid, 7, 3).astype(np.int64))
        del valid
        preds = [(0, np.array([7], np.int64))]
        print("\nBow.DropNils: Int64 + Float64 + Float64 with nulls, null density %.2f: %d of %d rows kept" % (p, k, n))

        def drop():
            _, _, count, contiguous = capi.drop_nils([ts, v1, v2], [2], outs=outs)
            assert count == k and not contiguous

        def filt():
            _, _, count, contiguous = capi.filter([key, v1, v2], preds, outs=outs_f)
            assert count == k and not contiguous

        d = timeit(drop)
        f = timeit(filt)
        m = timeit(lambda: capi.valid_mask([ts, v1, v2], [2], want_mask=False))
        for a, b in zip(outs[1:], outs_f[1:]):
            same(a, b, k)
        show("bowgpu_drop_nils", d)
        show("  its mask pass alone (bowgpu_valid_mask, numbers only)", m)
        show("bowgpu_filter, Int64 predicate column, the same rows", f)
        verdict("DropNils not slower than Filter", d, f[0], f[2])
        del v2, key
    del ts, v1, outs, outs_f

if not ONLY or ONLY == "distinct":
    for label, keys in (("1000 distinct Int64 values, shuffled", rng.integers(0, 1000, n) * 7919 - 4000),
                        ("a sorted timestamp column of a long-format frame (10 rows per timestamp)", np.arange(n, dtype=np.int64) // 10 * 1000)):
        print("\nBow.Distinct: %s" % label)
        s = np.sort(keys)
        flags = np.ones(n, bool)
        flags[:-1] = s[1:] != s[:-1]
        nd = int(flags.sum())
        col, sorted_col = device_col(keys), device_col(s)
        mask = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(flags, bitorder="little"), np.zeros(8, np.uint8)]))
        is_sorted = bool((keys[1:] >= keys[:-1]).all())
        del keys, s, flags
        out, out_t, out_c = capi.OutColumn(nd, capi.DEVICE), capi.OutColumn(n, capi.DEVICE), capi.OutColumn(nd, capi.DEVICE)
        perm = capi.DeviceBuffer(n * 8)

        def distinct():
            _, got = capi.distinct(col, out=out)
            assert got == nd

        def argsort():
            c, sflag = col.c(), C.c_int32(0)
            capi.check(capi.lib().bowgpu_argsort(C.byref(c), C.c_void_p(perm.ptr), capi.DEVICE, C.byref(sflag)))
            assert bool(sflag.value) == is_sorted

        def compact():
            _, _, count, contiguous = capi.compact([sorted_col], mask, outs=[out_c])
            assert count == nd and not contiguous

        d = timeit(distinct)
        c_ = timeit(compact)
        same(out, out_c, nd)
        show("bowgpu_distinct (%d values)" % nd, d)
        if is_sorted:
            i = timeit(lambda: capi.is_col_sorted(col))
            show("bowgpu_is_col_sorted", i)
            show("bowgpu_compact of the one-column frame by the group flags", c_)
            verdict("Distinct within is_col_sorted + compact", d, i[0] + c_[0], i[2] + c_[2])
        else:
            a = timeit(argsort)
            t = timeit(lambda: capi.take(col, perm, n, out=out_t))
            show("bowgpu_argsort (device-resident permutation)", a)
            show("bowgpu_take through it", t)
            show("bowgpu_compact of the one-column frame by the group flags", c_)
            verdict("Distinct within argsort + take + compact", d, a[0] + t[0] + c_[0], a[2] + t[2] + c_[2])
        del col, sorted_col, mask, out, out_t, out_c, perm
