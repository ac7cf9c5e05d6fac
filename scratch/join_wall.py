"""Wall time of Bow.OuterJoin / InnerJoin on the device (bowgpu_join), frames device-resident, every output allocated ONCE and the
ctypes arguments built outside the timed region, each comparator timed in the same run:
  (a) two sorted series of `rows` rows - Int64 key + one Float64 column with 30 % nulls, half the instants shared - OuterJoin and InnerJoin
        vs 1: bowgpu_memcpy_d2h + bowgpu_memcpy_h2d of the four columns and the two bitmaps: today's only route for a device-resident
              frame, with no host join counted.  The join is expected to beat it.
        vs 2: bowgpu_sort_by_col over a frame of the OUTER join's size and width (key reversed, so that it is moved): a call that moves
              comparable bytes.  No bar; the ratio is reported.
  (b) the same with the right frame's rows shuffled: the difference to (a) is the argsort - next to bowgpu_argsort alone on that key
  (c) rows/10 left rows against 1000 distinct right keys, every left row matching one right row: the probe under lane divergence
One process; run it under a time limit:
    timeout -k 10 900 python scratch/join_wall.py [rows [section [outfile [commit]]]]      # section: a / b / c / all
It prints what it measures and writes the same lines to outfile (default profiles/join_wall_<rows>.txt, e.g. join_wall_1e8.txt), headed
by the commit (the argument, else git rev-parse HEAD).  The dominant kernel comes from a profiler run of one section in a run of its
own: rocprofv3 --kernel-trace --stats -d DIR -- python scratch/join_wall.py 1e8 a /dev/null
Warm-up call, then REPS timed calls: wall median with min .. max."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ONLY = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "all" else None
OUTFILE = sys.argv[3] if len(sys.argv) > 3 else "profiles/join_wall_%s.txt" % ("%.0e" % n).replace("e+0", "e").replace("e+", "e")
REPS = 5
L = capi.lib()
INNER, OUTER = capi.JOIN_INNER, capi.JOIN_OUTER
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def commit():
    if len(sys.argv) > 4:
        return sys.argv[4]
    p = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True)
    return p.stdout.strip() if p.returncode == 0 else "unknown (no git history next to this tree)"


def timeit(fn, reps=REPS):
    fn(); capi.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    return wall[len(wall) // 2], wall[0], wall[-1]


def show(label, t):
    say("  %-74s median %9.3f ms   (min %.3f .. max %.3f)" % ((label,) + t))


def device_col(values, valid=None):
    typ = capi.INT64 if values.dtype == np.int64 else capi.FLOAT64
    v = capi.DeviceBuffer.from_numpy(values)
    if valid is None:
        return capi.Column(v, None, typ, 0, len(values), 0)
    b = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(valid, bitorder="little"), np.zeros(8, np.uint8)]))
    return capi.Column(v, b, typ, 0, len(values), int(len(values) - valid.sum()))


def series(key, rng, order=None):
    """key + one Float64 column with 30 % nulls, the rows in `order`"""
    val, valid = rng.standard_normal(len(key)), rng.random(len(key)) >= 0.3
    if order is not None:
        key, val, valid = key[order], val[order], valid[order]
    return [device_col(key), device_col(val, valid)]


class Join:
    """one bowgpu_join call with everything but the call built beforehand; the count call sizes the outputs"""

    def __init__(self, left, right, kind):
        self.rows, self.pairs = capi.join_rows(left[0], right[0], kind, count_only=True)[2:]
        self.outs = [capi.OutColumn(self.rows, capi.DEVICE) for _ in range(len(left) + len(right) - 1)]
        self.oarr = (capi.Out * len(self.outs))(*[o.c() for o in self.outs])
        self.l, self.r, self.nl, self.nr, self.kind = capi._cols(left), capi._cols(right), len(left), len(right), kind
        self.got = C.c_int64(0)

    def __call__(self):
        capi.check(L.bowgpu_join(self.l, self.nl, 0, self.r, self.nr, 0, self.kind, self.oarr, C.byref(self.got)))

    def free(self):
        for o in self.outs:
            o.values.free()
            o.validity.free()


def timed_join(label, left, right, kind, want_rows=None):
    j = Join(left, right, kind)
    t = timeit(j)
    assert j.got.value == j.rows and (want_rows is None or j.rows == want_rows), (j.got.value, j.rows, want_rows)
    show("%s: %d rows, %d pairs" % (label, j.rows, j.pairs), t)
    j.free()
    return t, j.rows


say("commit: %s" % commit())
say("device: %s   rows per series: %d   wall median of %d after a warm-up" % (capi.device_name(), n, REPS))
rng = np.random.default_rng(7)
lkey, rkey = np.arange(n, dtype=np.int64) * 2, np.arange(n, dtype=np.int64) * 4      # the right instants below 2n are the left's: n/2 shared
shared = (n + 1) // 2

if not ONLY or ONLY in ("a", "b"):
    left = series(lkey, rng)

if not ONLY or ONLY == "a":
    say("\n(a) two sorted series, Int64 key + Float64 with 30 % nulls, half the instants shared")
    right = series(rkey, rng)
    outer, out_rows = timed_join("bowgpu_join OUTER", left, right, OUTER, 2 * n - shared)
    inner, _ = timed_join("bowgpu_join INNER", left, right, INNER, shared)
    # comparator 1: the four columns and the two bitmaps to the host and back
    cols = left + right
    parts = [(c.values.ptr, c.length * 8) for c in cols] + [(c.validity.ptr, (c.length + 7) // 8) for c in cols if c.validity is not None]
    host = [np.empty(nbytes, np.uint8) for _, nbytes in parts]
    back = [capi.DeviceBuffer(nbytes) for _, nbytes in parts]

    def round_trip():
        for (ptr, nbytes), h, d in zip(parts, host, back):
            capi.check(L.bowgpu_memcpy_d2h(h.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_int64(nbytes)))
            capi.check(L.bowgpu_memcpy_h2d(C.c_void_p(d.ptr), h.ctypes.data_as(C.c_void_p), C.c_int64(nbytes)))

    rt = timeit(round_trip)
    moved = 2 * sum(nbytes for _, nbytes in parts)
    show("1: memcpy_d2h + memcpy_h2d of the four columns (%.1f GB over the host link)" % (moved / 1e9), rt)
    for d in back:
        d.free()
    del host, back
    # comparator 2: a frame of the outer join's size and width through bowgpu_sort_by_col
    frame = [device_col(np.arange(out_rows - 1, -1, -1, dtype=np.int64))] + \
            [device_col(rng.standard_normal(out_rows), rng.random(out_rows) >= 0.3) for _ in range(2)]
    souts = [capi.OutColumn(out_rows, capi.DEVICE) for _ in range(3)]

    def sort_by_col():
        _, unchanged = capi.sort_by_col(frame, 0, outs=souts)
        assert not unchanged

    sb = timeit(sort_by_col)
    show("2: bowgpu_sort_by_col, %d rows x 3 columns, key reversed" % out_rows, sb)
    for kind, t in (("OUTER", outer), ("INNER", inner)):
        say("  -> %s against 1: %.3f ms against %.3f ms (min %.3f): %s, %.1fx" %
            (kind, t[0], rt[0], rt[1], "FASTER than the bare round trip" if t[0] < rt[1] else "NOT faster than the bare round trip", rt[0] / t[0]))
    say("  -> OUTER against 2: %.2fx bowgpu_sort_by_col's wall time (no bar)" % (outer[0] / sb[0]))
    for c in frame + right:
        c.values.free()
    for o in souts:
        o.values.free()
        o.validity.free()
    del frame, souts, right

if not ONLY or ONLY == "b":
    say("\n(b) the same, the right frame's rows shuffled")
    right = series(rkey, rng, rng.permutation(n))
    outer_b, _ = timed_join("bowgpu_join OUTER", left, right, OUTER, 2 * n - shared)
    inner_b, _ = timed_join("bowgpu_join INNER", left, right, INNER, shared)
    perm = capi.DeviceBuffer(n * 8)

    def argsort():
        c = right[0].c(); s = C.c_int32(0)
        capi.check(L.bowgpu_argsort(C.byref(c), C.c_void_p(perm.ptr), capi.DEVICE, C.byref(s)))
        assert not s.value

    a = timeit(argsort)
    show("bowgpu_argsort of the shuffled right key alone (int64 permutation out)", a)
    if not ONLY:
        say("  -> OUTER: (b) - (a) = %.3f ms, INNER: %.3f ms, against the argsort's %.3f ms" % (outer_b[0] - outer[0], inner_b[0] - inner[0], a[0]))
    del right, perm

if not ONLY or ONLY == "c":
    m = max(n // 10, 1)
    say("\n(c) %d left rows against 1000 distinct right keys, every left row matching one right row" % m)
    left_c = series(rng.integers(0, 1000, m).astype(np.int64), rng)
    right_c = series(rng.permutation(1000).astype(np.int64), rng)
    timed_join("bowgpu_join OUTER", left_c, right_c, OUTER)
    timed_join("bowgpu_join INNER", left_c, right_c, INNER, m)
    sorted_left = series(np.sort(rng.integers(0, 1000, m)).astype(np.int64), rng)
    timed_join("bowgpu_join INNER, the left key in order (neighbouring lanes alike)", sorted_left, right_c, INNER, m)

with open(OUTFILE, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written: %s" % OUTFILE)
