"""Wall and kernel time of Bow.SortByCol on the device at 1e8 rows (Int64 key + one Float64 column, device-resident, outputs
allocated ONCE outside the timed region) for three input orders, next to the only alternative a device-resident frame has:
(a) bowgpu_memcpy_d2h + bowgpu_memcpy_h2d of the same two columns (the bare round trip, no host sort counted) and
(b) np.argsort(kind="stable") + two takes on the host.  One process; run it under a time limit:
    timeout -k 10 900 python scratch/sort_wall.py [rows]
Warm-up call, then REPS timed calls: min and median."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = 5
L = capi.lib()
print("device: %s   rows: %d   host cores available: %d" % (capi.device_name(), n, len(os.sched_getaffinity(0))))


def timeit(fn, reps=REPS):
    fn(); capi.synchronize()
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3); kern.append(capi.last_kernel_ms())
    wall.sort(); kern.sort()
    return wall[0], wall[len(wall) // 2], kern[0], kern[len(kern) // 2]


def orders(rng):
    yield "uniform shuffle", rng.permutation(n)
    blocks = n // 4096
    p = np.arange(n, dtype=np.int64)
    p[:blocks * 4096] = (rng.permuted(np.arange(blocks * 4096, dtype=np.int64).reshape(blocks, 4096) % 4096, axis=1) +
                         (np.arange(blocks, dtype=np.int64) * 4096)[:, None]).ravel()
    yield "shuffled inside 4096-row blocks", p
    yield "reversed", np.arange(n - 1, -1, -1, dtype=np.int64)


ts, val = capi.gen_dense(0, n, seed=42)          # ts[i] = i
outs = [capi.OutColumn(n, capi.DEVICE) for _ in range(2)]
take_out = capi.OutColumn(n, capi.DEVICE)
perm_dev = capi.DeviceBuffer(n * 8)
results = {}
for label, perm in orders(np.random.default_rng(7)):
    d_perm = capi.DeviceBuffer.from_numpy(perm.astype(np.int64))
    del perm
    s_ts = capi.out_as_column(capi.take(ts, d_perm, n, out_residency=capi.DEVICE))
    s_val = capi.out_as_column(capi.take(val, d_perm, n, out_residency=capi.DEVICE))
    d_perm.free()
    cols = [s_ts, s_val]

    def argsort():
        c = s_ts.c(); s = C.c_int32(0)
        capi.check(L.bowgpu_argsort(C.byref(c), C.c_void_p(perm_dev.ptr), capi.DEVICE, C.byref(s)))
        assert not s.value

    def gather():
        capi.take(s_val, perm_dev, n, out=take_out)

    def sort_by_col():
        _, unchanged = capi.sort_by_col(cols, 0, outs=outs)
        assert not unchanged

    a = timeit(argsort)
    name = capi.last_kernel_instance()
    passes = int(name.split("<")[1].split()[0])
    g = timeit(gather)
    s = timeit(sort_by_col)
    assert capi.checksum64(outs[0].values, n) == capi.checksum64(ts.values, n) and capi.checksum64(outs[1].values, n) == capi.checksum64(val.values, n)
    model = (8 + 24 * passes + 20 * 2) * n          # B: one key read, 12 B read + 12 B written per pass, (4 + 8 + 8) B per gathered column
    print("\n%s: %d radix passes run, %d skipped" % (label, passes, 8 - passes))
    print("  argsort       wall min %.2f / median %.2f ms   kernels min %.2f / median %.2f ms   (passes alone: %.2f TB/s by 24 B/row/pass)"
          % (a + (24 * passes * n / (a[2] * 1e-3) / 1e12,)))
    print("  gather/column wall min %.2f / median %.2f ms   kernels min %.2f / median %.2f ms   (%.2f TB/s by 20 B/row: random 8-byte reads)"
          % (g + (20 * n / (g[2] * 1e-3) / 1e12,)))
    print("  sort_by_col   wall min %.2f / median %.2f ms   kernels min %.2f / median %.2f ms   model %.1f GB moved -> %.2f TB/s (peak 8)"
          % (s + (model / 1e9, model / (s[2] * 1e-3) / 1e12)))
    results[label] = s
    if label == "uniform shuffle":
        keep = cols
    else:
        del cols, s_ts, s_val

# (a) the round trip the feature replaces: both columns to the host and back, nothing done to them there
s_ts, s_val = keep
h = [np.empty(n, np.int64), np.empty(n, np.float64)]
back = [capi.DeviceBuffer(n * 8) for _ in range(2)]


def round_trip():
    for col, harr, dbuf in zip((s_ts, s_val), h, back):
        capi.check(L.bowgpu_memcpy_d2h(harr.ctypes.data_as(C.c_void_p), C.c_void_p(col.values.ptr), C.c_int64(n * 8)))
        capi.check(L.bowgpu_memcpy_h2d(C.c_void_p(dbuf.ptr), harr.ctypes.data_as(C.c_void_p), C.c_int64(n * 8)))


rt = timeit(round_trip, 3)
print("\n(a) bowgpu_memcpy_d2h + bowgpu_memcpy_h2d of the two columns (%.1f GB over the host link): wall min %.2f / median %.2f ms = %.1f GB/s"
      % (32 * n / 1e9, rt[0], rt[1], 32 * n / (rt[0] * 1e-3) / 1e9))
print("    (the same bytes at the link's 63 GB/s specification: %.2f ms)" % (32 * n / 63e9 * 1e3))
# (b) the host sort between the two copies
t0 = time.perf_counter()
p = np.argsort(h[0], kind="stable")
t1 = time.perf_counter()
sorted_ts, sorted_val = h[0][p], h[1][p]
t2 = time.perf_counter()
assert sorted_ts[0] == 0 and sorted_ts[-1] == n - 1
print("(b) host: np.argsort(kind='stable') %.0f ms + two takes %.0f ms (numpy, one core of %d)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, len(os.sched_getaffinity(0))))
s = results["uniform shuffle"]
print("\nsort_by_col (uniform shuffle) wall median %.2f ms  vs  (a) %.2f ms: %s, %.1fx" % (s[1], rt[1], "FASTER than the bare round trip" if s[1] < rt[1] else "NOT faster than the bare round trip", rt[1] / s[1]))
