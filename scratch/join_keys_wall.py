"""Wall time of Bow.OuterJoin / InnerJoin on TWO common columns on the device (bowgpu_join_keys), frames device-resident, every output
allocated ONCE and the ctypes arguments built outside the timed region, each comparator timed in the same run.
Shape: L = R = rows / 2; keys (time, series id) - time ascends, 16 series per instant; one Float64 column with 30 % nulls per frame; the
right frame holds every second instant of the left's and as many beyond (half the tuples shared, each matching once).
  (a) both frames in order
  (b) the right frame's rows shuffled
        vs 1: bowgpu_join on key 0 (time) alone over the same frames - 16 right rows per shared left row, so it also moves 16x the rows
        vs 2: bowgpu_argsort of an (L + R)-row Int64 column (shuffled: all passes of its active digits)
        vs 3: bowgpu_join on ONE combined key time * 16 + series id in place of the time column: the one-key join with the two-key
              join's own pair list (its result is one column wider: the series id of the right frame is no key there)
Expectation (reasoned, not measured): a two-key join costs the one-key join of the same pair list (3) plus about two such argsorts (each
skipping the digits that are the same in every key, and none where the concatenated key is in order) plus the rank passes' traffic:
8 B read + 4 B written per row and key for the rank, 8 B written for the pack.
One process; run it under a time limit:
    timeout -k 10 900 python scratch/join_keys_wall.py [rows [section [outfile [commit]]]]      # section: a / b / all
It prints what it measures and writes the same lines to outfile (default profiles/join_keys_wall_<rows>.txt, e.g.
join_keys_wall_1e8.txt), headed by the commit (the argument, else git rev-parse HEAD).
Warm-up call, then REPS timed calls: wall median with min .. max."""
import ctypes as C
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
n = total // 2
ONLY = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "all" else None
OUTFILE = sys.argv[3] if len(sys.argv) > 3 else "profiles/join_keys_wall_%s.txt" % ("%.0e" % total).replace("e+0", "e").replace("e+", "e")
REPS = 5
SERIES = 16
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
    say("  %-78s median %9.3f ms   (min %.3f .. max %.3f)" % ((label,) + t))


def device_col(values, valid=None):
    typ = capi.INT64 if values.dtype == np.int64 else capi.FLOAT64
    v = capi.DeviceBuffer.from_numpy(values)
    if valid is None:
        return capi.Column(v, None, typ, 0, len(values), 0)
    b = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(valid, bitorder="little"), np.zeros(8, np.uint8)]))
    return capi.Column(v, b, typ, 0, len(values), int(len(values) - valid.sum()))


def frame(t, s, rng, order=None):
    """time, series id, one Float64 column with 30 % nulls, the rows in `order`"""
    val, valid = rng.standard_normal(len(t)), rng.random(len(t)) >= 0.3
    if order is not None:
        t, s, val, valid = t[order], s[order], val[order], valid[order]
    return [device_col(t), device_col(s), device_col(val, valid)]


def free(cols):
    for c in cols:
        c.values.free()
        if c.validity is not None:
            c.validity.free()


class Join:
    """one bowgpu_join_keys / bowgpu_join call with everything but the call built beforehand; the count call sizes the outputs"""

    def __init__(self, left, right, kind, keys):
        lk, rk = [left[k] for k in keys], [right[k] for k in keys]
        self.rows, self.pairs = capi.join_keys_rows(lk, rk, kind, count_only=True)[2:]
        self.outs = [capi.OutColumn(self.rows, capi.DEVICE) for _ in range(len(left) + len(right) - len(keys))]
        self.oarr = (capi.Out * len(self.outs))(*[o.c() for o in self.outs])
        self.l, self.r, self.nl, self.nr, self.kind = capi._cols(left), capi._cols(right), len(left), len(right), kind
        self.keys, self.nk = (C.c_int32 * len(keys))(*keys), len(keys)
        self.got = C.c_int64(0)

    def __call__(self):
        if self.nk == 1:
            capi.check(L.bowgpu_join(self.l, self.nl, self.keys[0], self.r, self.nr, self.keys[0], self.kind, self.oarr, C.byref(self.got)))
        else:
            capi.check(L.bowgpu_join_keys(self.l, self.nl, self.keys, self.r, self.nr, self.keys, self.nk, self.kind, self.oarr, C.byref(self.got)))

    def free(self):
        for o in self.outs:
            o.values.free()
            o.validity.free()


def timed_join(label, left, right, kind, keys, want_rows=None):
    j = Join(left, right, kind, keys)
    t = timeit(j)
    assert j.got.value == j.rows and (want_rows is None or j.rows == want_rows), (j.got.value, j.rows, want_rows)
    show("%s: %d rows, %d pairs" % (label, j.rows, j.pairs), t)
    j.free()
    return t, j.rows


say("commit: %s" % commit())
say("device: %s   L = R = %d rows, %d series per instant   wall median of %d after a warm-up" % (capi.device_name(), n, SERIES, REPS))
rng = np.random.default_rng(7)
row = np.arange(n, dtype=np.int64)
lt, ls = row // SERIES, row % SERIES
rt, rs = (row // SERIES) * 2, row % SERIES      # every second instant of the left's, and as many beyond: half the tuples shared
shared = int(np.count_nonzero(rt < lt[-1] + 1))
left = frame(lt, ls, rng)
argsort_key = capi.DeviceBuffer.from_numpy(rng.permutation(2 * n).astype(np.int64))
perm = capi.DeviceBuffer(2 * n * 8)


def argsort():
    c = capi.Column(argsort_key, None, capi.INT64, 0, 2 * n, 0).c()
    s = C.c_int32(0)
    capi.check(L.bowgpu_argsort(C.byref(c), C.c_void_p(perm.ptr), capi.DEVICE, C.byref(s)))
    assert not s.value


for section, title, order in (("a", "both frames in order", None), ("b", "the right frame's rows shuffled", "shuffle")):
    if ONLY and ONLY != section:
        continue
    say("\n(%s) %s" % (section, title))
    order_rows = rng.permutation(n) if order else None
    right = frame(rt, rs, rng, order_rows)
    two_o, _ = timed_join("bowgpu_join_keys (time, series) OUTER", left, right, OUTER, [0, 1], 2 * n - shared)
    two_i, _ = timed_join("bowgpu_join_keys (time, series) INNER", left, right, INNER, [0, 1], shared)
    one_o, rows_one = timed_join("1: bowgpu_join on time alone OUTER", left, right, OUTER, [0])
    one_i, _ = timed_join("1: bowgpu_join on time alone INNER", left, right, INNER, [0])
    lc, rc = [device_col(lt * SERIES + ls)] + left[1:], [device_col((rt * SERIES + rs)[order_rows] if order_rows is not None else rt * SERIES + rs)] + right[1:]
    cmb_o, _ = timed_join("3: bowgpu_join on time * 16 + series OUTER", lc, rc, OUTER, [0], 2 * n - shared)
    cmb_i, _ = timed_join("3: bowgpu_join on time * 16 + series INNER", lc, rc, INNER, [0], shared)
    free([lc[0], rc[0]])
    a = timeit(argsort)
    show("2: bowgpu_argsort of a shuffled Int64 column of L + R = %d rows (int64 permutation out)" % (2 * n), a)
    for kind, two, one in (("OUTER", two_o, cmb_o), ("INNER", two_i, cmb_i)):
        say("  -> %s: two keys %.3f ms = the combined key (3) %.3f ms %+.3f ms; the difference is %.2f such argsorts (2)" %
            (kind, two[0], one[0], two[0] - one[0], (two[0] - one[0]) / a[0]))
    say("  -> two keys OUTER against 2 x argsort: %.2fx" % (two_o[0] / (2 * a[0])))
    free(right)

with open(OUTFILE, "w") as f:
    f.write("\n".join(lines) + "\n")
print("written: %s" % OUTFILE)
