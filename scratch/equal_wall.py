"""Wall time of bowgpu_equal and bowgpu_valid_row on the device at 1e8 rows, device-resident, 30 % nulls, the ctypes arguments built
outside the timed region, the comparator in the same run and alternating with the call it is compared to:
    (a) bowgpu_equal of two equal Float64 columns with bitmaps (2 x 8.125 B read per row, nothing written), both modes
                                                                      vs  bowgpu_diff of one such column (the same 16.25 B per row, partly written)
    (b) the same with the only difference at row 0 and at row n - 1  (the early leave: row 0 should cost about a call's overhead)
    (c) a three-column Int64 / Float64 / Boolean frame against its copy
    (d) bowgpu_valid_row from the last row backwards over a column whose only valid row is row 0 (n / 8 B read), and over one that is valid
        at the start row
One process; run it under a time limit:
    timeout -k 10 600 python scratch/equal_wall.py [rows [output file]]
Warm-up call, then REPS timed calls: median and min .. max.  "Not slower" means: the median is within the comparator's min .. max.
The report goes to the output file (default profiles/equal_wall_1e8.txt) and to stdout."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else "profiles/equal_wall_1e8.txt"
REPS = 5
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def timeit(*fns, reps=REPS):
    """the calls alternate: one warm-up each, then reps rounds of one timed call each.  -> (median, min, max) per call"""
    for fn in fns:
        fn(); capi.synchronize()
    wall = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); capi.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return [(sorted(w)[len(w) // 2], min(w), max(w)) for w in wall]


def show(label, t):
    say("  %-66s median %8.3f ms   (min %.3f .. max %.3f)" % ((label,) + t))


def device_col(values, valid, typ):
    v = capi.DeviceBuffer.from_numpy(values)
    if valid is None:
        return capi.Column(v, None, typ, 0, n, 0)
    b = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(valid, bitorder="little"), np.zeros(8, np.uint8)]))
    return capi.Column(v, b, typ, 0, n, int(n - valid.sum()))


def poke(col, row, value):
    """one 8-byte value of a device-resident column"""
    v = np.array([value], np.float64)
    capi.check(capi.lib().bowgpu_memcpy_h2d(C.c_void_p(col.values.ptr + 8 * row), v.ctypes.data_as(C.c_void_p), C.c_int64(8)))


def equal_call(left, right, mode):
    l, r, info = capi._cols(left), capi._cols(right), capi.EqualInfo()

    def call():
        capi.check(capi.lib().bowgpu_equal(l, r, len(left), mode, C.byref(info)))
    return call, info


def valid_row_call(col, start, direction):
    c, row = capi._cols([col]), C.c_int64(0)

    def call():
        capi.check(capi.lib().bowgpu_valid_row(c, 1, C.c_int64(start), direction, C.byref(row)))
    return call, row


say("device: %s   rows: %d" % (capi.device_name(), n))
rng = np.random.default_rng(7)
vals = rng.standard_normal(n)
valid = rng.random(n) >= 0.3
row_a = int(np.flatnonzero(valid)[0])       # the first and the last valid row: where (b) plants its difference
row_z = int(np.flatnonzero(valid)[-1])
left, right = device_col(vals, valid, capi.FLOAT64), device_col(vals, valid, capi.FLOAT64)

say("\n(a) Equal of two equal Float64 columns with bitmaps, 30 % nulls (16.25 B read per row)  vs  Diff of one (16.25 B per row, partly written)")
out_d = [capi.OutColumn(n, capi.DEVICE)]
go, info_go = equal_call([left], [right], capi.EQUAL_GO)
bits, info_bits = equal_call([left], [right], capi.EQUAL_BITS)
t_go, t_bits, t_diff = timeit(go, bits, lambda: capi.diff([left], outs=out_d))
assert (info_go.equal, info_go.first_row, info_go.first_col) == (1, -1, -1) and info_bits.equal == 1
show("bowgpu_equal, BOWGPU_EQUAL_GO, equal", t_go)
show("bowgpu_equal, BOWGPU_EQUAL_BITS, equal", t_bits)
show("bowgpu_diff of one such column", t_diff)
say("  equal: %.2f TB/s by 16.25 B per row over the wall time" % (16.25 * n / (t_go[0] * 1e-3) / 1e12))
say("  -> Equal not slower than Diff: %.3f ms against %.3f ms (min %.3f .. max %.3f), ratio %.2f: %s"
    % (t_go[0], t_diff[0], t_diff[1], t_diff[2], t_go[0] / t_diff[0], "MET" if t_go[0] <= t_diff[2] else "MISSED"))
del out_d

say("\n(b) the same, the only difference at one row")
small_l, small_r = capi.Column.from_list([1.0] * 1000, "float64").to_device(), capi.Column.from_list([1.0] * 1000, "float64").to_device()
tiny, _ = equal_call([small_l], [small_r], capi.EQUAL_GO)
for label, row in (("the first valid row (%d)" % row_a, row_a), ("the last valid row (%d)" % row_z, row_z)):
    poke(right, row, vals[row] + 1.0)
    t_one, t_tiny = timeit(go, tiny)
    assert (info_go.equal, info_go.first_row, info_go.first_col) == (0, row, 0)
    show("bowgpu_equal, difference at " + label, t_one)
    show("bowgpu_equal of two 1000-row columns (a call's overhead)", t_tiny)
    poke(right, row, vals[row])
del small_l, small_r

say("\n(c) a three-column frame, Int64 / Float64 / Boolean, each with a bitmap (2 x 16.375 B read per row), against its copy")
ints = np.arange(n, dtype=np.int64)
flags = np.packbits(rng.random(n) < 0.5, bitorder="little")
flags = np.concatenate([flags, np.zeros(8, np.uint8)])
frames = [[device_col(ints, valid, capi.INT64), left if k == 0 else right, device_col(flags, valid, capi.BOOLEAN)] for k in range(2)]
del ints, flags
three, info3 = equal_call(frames[0], frames[1], capi.EQUAL_GO)
(t_three,) = timeit(three)
assert info3.equal == 1
show("bowgpu_equal, three columns, equal", t_three)
say("  %.2f TB/s by 32.75 B per row over the wall time" % (32.75 * n / (t_three[0] * 1e-3) / 1e12))
del frames, left, right, vals

say("\n(d) valid_row from the last row backwards, one column")
only0 = np.zeros(n, bool)
only0[0] = True
far = device_col(np.zeros(8, np.float64), only0, capi.FLOAT64)         # (bitmaps alone are read)
near = device_col(np.zeros(8, np.float64), valid | (np.arange(n) == n - 1), capi.FLOAT64)
call_far, row_far = valid_row_call(far, n - 1, -1)
call_near, row_near = valid_row_call(near, n - 1, -1)
t_far, t_near = timeit(call_far, call_near)
assert (row_far.value, row_near.value) == (0, n - 1)
show("bowgpu_valid_row, the only valid row is row 0 (n / 8 B read)", t_far)
show("bowgpu_valid_row, valid at the start row", t_near)
say("  far: %.2f TB/s by 1/8 B per row over the wall time" % (n / 8 / (t_far[0] * 1e-3) / 1e12))

with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
