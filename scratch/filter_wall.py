"""Wall and kernel time of Bow.Filter on the device at 1e8 rows: a frame of one Int64 predicate column and two Float64 value columns
(one of them with nulls), device-resident, outputs allocated ONCE outside the timed region, for four selections, next to the only
route a device-resident frame had before: bowgpu_take per column over a device-resident list of the same rows (the list prepared
outside the clock).  One process; run it under a time limit:
    timeout -k 10 900 python scratch/filter_wall.py [rows [selection]]
Per-kernel times come from a profiler run of one selection, e.g. rocprofv3 --kernel-trace --stats -d DIR -- python scratch/filter_wall.py 1e8 0.50
Warm-up call, then REPS timed calls: min and median.  TB/s by the algorithmic bytes: the predicate column and the bitmap (written once,
read once), the kept rows of every column read and written."""
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ONLY = sys.argv[2] if len(sys.argv) > 2 else None      # run the selections whose label contains this (a profiler run of one of them)
REPS = 5
print("device: %s   rows: %d   frame: Int64 predicate column + Float64 + Float64 with nulls" % (capi.device_name(), n))


def timeit(fn, reps=REPS):
    fn(); capi.synchronize()
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3); kern.append(capi.last_kernel_ms())
    wall.sort(); kern.sort()
    return wall[0], wall[len(wall) // 2], kern[0], kern[len(kern) // 2]


def selections(rng):
    for p in (0.01, 0.5, 0.99):
        yield "random p = %.2f" % p, rng.random(n) < p
    keep = np.zeros(n, bool)   # 1 % of the rows in runs of 4096 (not aligned with the kernel's tiles)
    for b in rng.choice(n // 4096 - 1, max(n // 4096 // 100, 1), replace=False):
        keep[b * 4096 + 1234:(b + 1) * 4096 + 1234] = True
    yield "clustered: 1 % in 4096-row runs", keep


_, v1 = capi.gen_dense(0, n, seed=42)
_, v2 = capi.gen_sparse(0, n, seed=43)
v2.null_count = n - int(np.unpackbits(v2.validity.to_numpy(np.uint8, (n + 7) // 8), bitorder="little")[:n].sum())
outs = [capi.OutColumn(n, capi.DEVICE) for _ in range(3)]
take_outs = [capi.OutColumn(n, capi.DEVICE) for _ in range(3)]
rows = []
verdict = None
for label, keep in selections(np.random.default_rng(7)):
    if ONLY and ONLY not in label:
        continue
    k = int(keep.sum())
    key = capi.Column(capi.DeviceBuffer.from_numpy(np.where(keep, 7, 3).astype(np.int64)), None, capi.INT64, 0, n, 0)
    idx = capi.DeviceBuffer.from_numpy(np.flatnonzero(keep).astype(np.int64))
    del keep
    cols = [key, v1, v2]
    preds = [(0, np.array([7], np.int64))]

    def one_call():
        _, _, count, contiguous = capi.filter(cols, preds, outs=outs)
        assert count == k and not contiguous

    def mask_only():
        capi.filter_mask(cols[:1], preds, out_residency=capi.DEVICE)

    def take_route():
        for c, o in zip(cols, take_outs):
            capi.take(c, idx, k, out=o)

    f = timeit(one_call)
    m = timeit(mask_only)
    t = timeit(take_route)
    for a, b in zip(outs, take_outs):   # the two routes produced the same columns
        assert (a.length, a.null_count) == (b.length, b.null_count)
        assert capi.checksum64(a.values, k) == capi.checksum64(b.values, k)
        assert capi.checksum64(a.validity, k // 64, 0) == capi.checksum64(b.validity, k // 64, 0)
    model = 8 * n + 2 * (n // 8) + 2 * 3 * 8 * k
    print("\n%s: %d of %d rows kept" % (label, k, n))
    print("  bowgpu_filter          wall min %.3f / median %.3f ms" % f[:2])
    print("    pass 1 filter_mask_kernel + stats     min %.3f / median %.3f ms   (device events; %.2f TB/s by 8 B/row + the bitmap)"
          % (m[2], m[3], (8 * n + n // 8) / (m[3] * 1e-3) / 1e12))
    print("    pass 2 scan + filter_scatter_kernel   min %.3f / median %.3f ms   (device events from the scan to the scatter launch)" % f[2:])
    print("    algorithmic bytes %.2f GB -> %.2f TB/s over the two event intervals, %.2f TB/s over the wall time"
          % (model / 1e9, model / ((m[3] + f[3]) * 1e-3) / 1e12, model / (f[1] * 1e-3) / 1e12))
    print("  bowgpu_take x 3 columns wall min %.3f / median %.3f ms   (indices prepared outside the clock)" % t[:2])
    print("  filter / take, wall medians: %.2fx" % (t[1] / f[1]))
    if label == "random p = 0.50":
        verdict = (f[1], t[1])
    del key, idx

if verdict is None:
    sys.exit(0)
f, t = verdict
print("\nselectivity 0.5: bowgpu_filter wall median %.3f ms  vs  bowgpu_take per column %.3f ms: %s" %
      (f, t, "FASTER than the take route" if f < t else "NOT faster than the take route"))
