"""The cells of the Rolling.Aggregate route table (tests/agg_route_table.json): which calls they are and how one is run.

Shared by tests/test_gpu_agg_route_table.py, which executes every cell and compares it with the table, and by
scratch/agg_route_table.py, which writes the table (and dumps routes + output checksums for an A/B of two libraries).

A cell = (column kind, rows per window, variant, reducer set).  ts = arange(n), interval = rows, n = rows * K with n >= 65536, so
every window holds exactly `rows` rows and n / W == rows: the call's average window length is the cell's."""
import zlib

import numpy as np

from bow_amd import capi

# both sides of every window-length threshold of common.h and agg_pass.cpp job_run
ROWS = (2, 3, 5, 11, 12, 16, 17, 47, 48, 63, 64, 127, 128, 129, 176, 177, 200, 201, 255, 256, 511, 512, 1000)
ROWS_VARIANTS = (4, 12, 64, 128, 144, 192, 256, 1000)   # the lengths that also run under every variant below
COLUMNS = ("f64", "f64_nulls", "i64")
REDUCER_SETS = (
    ("Sum", "ArithmeticMean"),
    ("Count", "NumRows"),
    ("Min", "Max"),
    ("First", "Last"),
    ("Sum", "Min", "Max"),
    ("WeightedAverageStep",),
    ("IntegralTrapezoid",),
    ("IntegralStep", "WeightedAverageLinear"),
    ("Sum", "Min", "WeightedAverageStep"),
    ("Min", "Last"),
)
ROUTE_VARIANTS = ("NO_SIMPLE", "FORCE_GENERAL", "NO_LONG_ONLY", "LONG_CLASSIC", "LONG_STREAM_ALL", "TW_ROWS", "TW_F64", "QUEUE_HOST",
                  "QUEUE_DEVICE", "SIMPLE_SMALL_LIST", "SIMPLE_LARGE_LIST")
VARIANTS = ("inclusive", "strict", "plan") + ROUTE_VARIANTS
# two calls of a handful of giant windows over 2^23 rows: the bisection form and, just below it, the streaming form
BIG_N = 1 << 23
BIG_INTERVALS = (1 << 22, (BIG_N + 2) // 3)

MAX_AGGS = 1 + max(len(s) for s in REDUCER_SETS)


def rows_n(rows):
    return rows * -(-65536 // rows)


def groups():
    """(column kind, rows per window or 'big') - one test each"""
    return [(col, rows) for col in COLUMNS for rows in sorted(set(ROWS) | set(ROWS_VARIANTS))] + [(col, "big") for col in COLUMNS]


def group_shapes(rows):
    """[(key suffix, n, interval, variants)] of a group"""
    if rows == "big":
        return [("big%d" % i, BIG_N, iv, ("default",)) for i, iv in enumerate(BIG_INTERVALS)]
    variants = (("default",) if rows in ROWS else ()) + (VARIANTS if rows in ROWS_VARIANTS else ())
    return [(str(rows), rows_n(rows), rows, variants)]


def keys_of(col, rows):
    return ["%s|%s|%s" % (col, suffix, v) for suffix, _n, _iv, variants in group_shapes(rows) for v in variants]


class Data:
    """the three columns on the device, uploaded once; calls take a prefix of them"""

    def __init__(self, n_max):
        rng = np.random.default_rng(20260)
        self.n_max = n_max
        self.ts = capi.DeviceBuffer.from_numpy(np.arange(n_max, dtype=np.int64))
        f = rng.standard_normal(n_max)
        self.valid = rng.random(n_max) > 0.3
        self.f64 = capi.DeviceBuffer.from_numpy(f)
        self.i64 = capi.DeviceBuffer.from_numpy(rng.integers(-1000, 1000, n_max, dtype=np.int64))
        self.bits = capi.DeviceBuffer.from_numpy(np.concatenate([np.packbits(self.valid, bitorder="little"), np.zeros(8, np.uint8)]))
        self.outs = {}

    def cols(self, col, n):
        ts = capi.Column(self.ts, None, capi.INT64, 0, n)
        if col == "f64":
            return [ts, capi.Column(self.f64, None, capi.FLOAT64, 0, n)]
        if col == "i64":
            return [ts, capi.Column(self.i64, None, capi.INT64, 0, n)]
        return [ts, capi.Column(self.f64, self.bits, capi.FLOAT64, 0, n, int(n - self.valid[:n].sum()))]

    def out_cols(self, W):
        if W not in self.outs:
            self.outs[W] = [capi.OutColumn(W, capi.DEVICE) for _ in range(MAX_AGGS)]
        return self.outs[W]


def run_cell(data, col, n, interval, variant, reducers, names, detail=False):
    """one call -> the cell's code: name index * 6 + (long_windows: 0 none, 1 all, 2 some) * 2 + (slow rows > 0); a declined
    call: minus its error code.  detail=True: also a string with the instantiation, the null counts and checksums of the outputs."""
    aggs = [("WindowStart", 0)] + [(k, 1) for k in reducers]
    cols = data.cols(col, n)
    W = -(-n // interval)
    outs = data.out_cols(W)[:len(aggs)]
    kw = {}
    mask = 0
    if variant == "inclusive":
        kw["inclusive"] = True
    elif variant == "strict":
        kw["strict_order"] = True
    elif variant == "plan":
        kw["plan"] = capi.plan_windows_ex(cols[0], interval, 0)
    elif variant != "default":
        mask = getattr(capi, "ROUTE_" + variant)
    try:
        with capi.route(mask):
            outs, info = capi.rolling_aggregate(cols, 0, interval, aggs, outs=outs, **kw)
    except capi.BowGpuError as e:
        return (-e.code, "error: %s" % e.message) if detail else -e.code
    assert info.num_windows == W, (info.num_windows, W)
    name = capi.last_kernel_name()
    if name not in names:
        names.append(name)
    lw = 0 if info.long_windows == 0 else 1 if info.long_windows == info.num_windows else 2
    code = names.index(name) * 6 + lw * 2 + (1 if capi.last_call_slow_rows() > 0 else 0)
    if not detail:
        return code
    parts = [capi.last_kernel_instance()]
    nb = (W + 7) // 8
    for o in outs:
        vx, vs = capi.checksum64(o.values, W)
        bx, bs = capi.checksum64(o.validity, nb // 8) if nb >= 8 else (0, 0)
        tail = zlib.crc32(o.validity.to_numpy(np.uint8, nb - nb // 8 * 8, nb // 8 * 8).tobytes()) if nb % 8 else 0
        parts.append("%d:%d:%016x%016x:%016x%016x%08x" % (o.type, o.null_count, vx, vs, bx, bs, tail))
    return code, " ".join(parts)
