"""Wall and kernel time of Bow.Convert on the device (bowgpu_convert) at 1e8 rows, 30 % nulls, for the nine (source, target) pairs of
Int64, Float64 and Boolean: device-resident input and output, outputs and ctypes arguments built ONCE outside the timed region.  The
comparator, in the same run, is bowgpu_diff of the Float64 column: a streaming pass that reads and writes about 16.25 B/row.  What
bytes moved lead one to expect: an 8-byte -> 8-byte pair moves Diff's bytes and takes about Diff's time; 8-byte -> Boolean and
Boolean -> 8-byte move about 8.4 B/row and take no longer than Diff; Boolean -> Boolean is a bitmap copy.  One process; run it under
a time limit:
    timeout -k 10 600 python scratch/convert_wall.py [rows]
Warm-up call, then REPS timed calls: wall median with the spread (min .. max), kernel median."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = 5
L = capi.lib()
I, F, B = capi.INT64, capi.FLOAT64, capi.BOOLEAN
NAMES = {I: "Int64", F: "Float64", B: "Boolean"}
print("device: %s   rows: %d   nulls: 30 %%   reps: %d" % (capi.device_name(), n, REPS))


def timeit(fn):
    fn(); capi.synchronize()
    wall, kern = [], []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3); kern.append(capi.last_kernel_ms())
    wall.sort(); kern.sort()
    return wall[0], wall[REPS // 2], wall[-1], kern[REPS // 2]


rng = np.random.default_rng(5)
nb = (n + 7) // 8
values = capi.DeviceBuffer.from_numpy(np.round(rng.standard_normal(n) * 1000.0, 1))     # Float64; read as Int64 the same bytes are arbitrary integers
bits = capi.DeviceBuffer.from_numpy(rng.integers(0, 256, nb + 8, dtype=np.uint8))       # a Boolean column's value bits
valid = np.packbits(rng.random(n) >= 0.3, bitorder="little")
nulls = int(n - np.unpackbits(valid, bitorder="little")[:n].sum())
validity = capi.DeviceBuffer.from_numpy(np.concatenate([valid, np.zeros(8, np.uint8)]))
del valid
sources = {t: capi.Column(bits if t == B else values, validity, t, 0, n, nulls) for t in (I, F, B)}
out = capi.OutColumn(n, capi.DEVICE)                                                    # 8 n bytes: holds a Boolean output's n / 8 too
oarr = (capi.Out * 1)(out.c())


def bytes_per_row(a, b):
    return (0.125 if a == B else 8.0) + 0.125 + (0.125 if b == B else 8.0) + 0.125        # source + its validity, target + its validity


carr = capi._cols([sources[F]])
diff_out = (capi.Out * 1)(out.c())
d = timeit(lambda: capi.check(L.bowgpu_diff(carr, 1, None, 0, diff_out)))
assert diff_out[0].length == n
print("\nbowgpu_diff Float64 (comparator, 16.25 B/row): wall median %.3f ms (min %.3f .. max %.3f)   kernel median %.3f ms = %.2f TB/s"
      % (d[1], d[0], d[2], d[3], 16.25 * n / (d[3] * 1e-3) / 1e12))
print("\n%-20s %10s %22s %12s %8s %8s   %s" % ("pair", "wall med", "(min .. max) ms", "kernel med", "B/row", "TB/s", "expectation"))
missed = []
for a in (I, F, B):
    for b in (I, F, B):
        carr = capi._cols([sources[a]])
        tarr = (C.c_int32 * 1)(b)
        r = timeit(lambda: capi.check(L.bowgpu_convert(carr, tarr, 1, oarr)))
        assert (oarr[0].length, oarr[0].type, oarr[0].null_count) == (n, b, nulls) and capi.last_kernel_name() == "convert_kernel"
        bpr = bytes_per_row(a, b)
        if a != B and b != B:
            want, ok = "about Diff's time (within 15 %)", r[1] <= 1.15 * d[1]
        elif a == B and b == B:
            want, ok = "a bitmap copy: far below Diff", r[1] <= 0.25 * d[1]
        else:
            want, ok = "no longer than Diff", r[1] <= d[1]
        if not ok:
            missed.append("%s -> %s" % (NAMES[a], NAMES[b]))
        print("%-20s %10.3f %22s %12.3f %8.2f %8.2f   %s: %s" % ("%s -> %s" % (NAMES[a], NAMES[b]), r[1], "(%.3f .. %.3f)" % (r[0], r[2]), r[3], bpr,
                                                              bpr * n / (r[3] * 1e-3) / 1e12, want, "met" if ok else "MISSED"))
print("\nexpectations MISSED: %s" % (", ".join(missed) + " (kernel to look at: convert_kernel, bow_amd/csrc/convert.hip)" if missed else "none"))
