"""Seeded cases for the paths that serve an INTERVAL COLUMN WITH NULLS (bow_amd/csrc/ts_nulls.hip, aggregate_api.cpp run_aggregate_null_ts,
interp_null_ts.cpp): what tests/test_gpu_null_ts_fuzz.py pushes through the device and tests/test_null_ts_cases_cpu.py checks
without one.  No GPU is needed to draw a case or to build its oracle columns; Case.ccols() alone touches the device, and only for a
device-resident case.

Over the hand-picked shapes of test_gpu_aggregate.py / test_gpu_callers.py a case adds: the interval column - like every value
column - at an Arrow offset of 0 .. 69 rows inside longer buffers whose bits and values outside the column are random, row counts on
the edges of a wavefront's keep word and of the tiles, null runs that are i.i.d., short, longer than the near walk of the neighbour
index (2048 bits) or than one of its blocks (4096), runs that begin or end on a 32 / 64 / 4096-bit edge of the offset bitmap, a null
last row, arbitrary bits in the timestamps of null rows, one to three value columns of either type with or without validity, every
reducer the path serves with Factor chains, reducer lists that split into batches, nanosecond-scale timestamps."""
import numpy as np

from bow_amd import capi
from oracle import pyoracle as orc
from test_gpu_aggregate import ALL_AGGS, TIME_AGGS
from test_gpu_fuzz import rand_col, rand_ts

AGG_SIZES = [1, 2, 63, 64, 65, 127, 129, 511, 512, 513, 639, 641, 1023, 1025, 2047, 2049, 4095, 4097, 5000, 40_000]
INTERP_SIZES = [63, 64, 65, 127, 129, 511, 512, 513, 639, 641, 700]
AGG_CASES, INTERP_CASES, CHAIN_CASES = 30, 30, 20      # per seed
LINEAR = ("IntegralTrapezoid", "WeightedAverageLinear")   # the two reducers that ask for inclusive windows (aggregation.go:183-185)
MAX_AGGS_PER_LAUNCH = 16                                # bow_amd/csrc/common.h kMaxAggs: a longer reducer list runs as several batches


def prev_row(ts0):
    return (float(ts0 - 3), True, 42.5, True, 42)


# ------------------------------------------------------------------ predicates over (ts, tvalid) of the column's own rows
def prev_valid(tvalid):
    """index of the nearest row at or before i whose timestamp is valid, -1 if none"""
    return np.maximum.accumulate(np.where(tvalid, np.arange(len(tvalid)), -1))


def next_valid(tvalid):
    """index of the nearest row at or behind i whose timestamp is valid, n if none"""
    n = len(tvalid)
    return np.minimum.accumulate(np.where(tvalid, np.arange(n), n)[::-1])[::-1]


def rows_on_a_start_with_a_null_behind(ts, tvalid, s0, interval):
    """bool per row: the rows ts_nulls.hip singles out after an inclusive iteration - on a window start (not window 0's), the first
    with that timestamp, the next row's timestamp null (the next window begins at `rowIndex - 1`, rolling.go:214-218).
    The timestamps of null rows are never looked at."""
    n = len(ts)
    hit = np.zeros(n, bool)
    if n < 2:
        return hit
    t = np.where(tvalid, ts, s0)                     # (a null row's timestamp may hold anything)
    hit[:-1] = tvalid[:-1] & ~tvalid[1:] & (t[:-1] >= s0 + interval) & ((t[:-1] - s0) % interval == 0)
    pp = np.concatenate(([-1], prev_valid(tvalid)[:-1]))
    hit &= (pp < 0) | (t[np.maximum(pp, 0)] < t)
    return hit


def outside_inclusive_interpolate(ts, tvalid, s0, interval):
    """the two shapes inclusive Interpolate over an interval column with nulls leaves to the reference (BOWGPU_ERR_TS_NULLS, interp_null_ts.cpp
    interp_null_ts): a row as above that sits on -1 - interpolateWindow's "no first value", interpolation.go:119-127 - or whose next
    valid timestamp equals its own (the next window then has its start and adds no row)"""
    n = len(ts)
    quirk = rows_on_a_start_with_a_null_behind(ts, tvalid, s0, interval)
    if not quirk.any():
        return False
    t = np.where(tvalid, ts, s0)
    nb = np.concatenate((next_valid(tvalid)[1:], [n]))       # next valid row BEHIND row i
    return bool((quirk & ((t == -1) | ((nb < n) & (t[np.minimum(nb, n - 1)] == t)))).any())


def longest_null_run(tvalid):
    if tvalid.all():
        return 0
    edges = np.flatnonzero(np.diff(np.concatenate(([1], tvalid.astype(np.int8), [1]))))
    return int((edges[1::2] - edges[::2]).max())


# ------------------------------------------------------------------ the interval column's validity
VALIDITY_MODES = ("iid", "runs", "long-run", "edge-runs", "ends-only")


def interval_validity(rng, n, pad, mode=None, null_last=None, past_near=False, frac=None):
    """(bool[n], mode): row 0 valid; the last row null in about 5 % of the draws (null_last: forced).  past_near: the long run is
    longer than 2048 rows for sure; frac: the null fraction of mode "iid"."""
    if mode is None:
        mode = VALIDITY_MODES[int(rng.choice(5, p=[0.35, 0.2, 0.15, 0.2, 0.1]))]
    if mode == "long-run" and n < 2100:
        mode = "runs"
    tv = np.ones(n, bool)
    if mode == "iid":
        tv = rng.random(n) >= (frac if frac is not None else [0.01, 0.05, 0.3, 0.9][int(rng.integers(0, 4))])
    elif mode == "runs":
        i = int(rng.integers(0, 40))
        while i < n:
            run = int(rng.integers(1, 71))
            tv[i:i + run] = False
            i += run + int(rng.integers(1, 120))
    elif mode == "long-run":
        # longer than prev_valid_near's 64 words (2048 bits), or than a 4096-bit block of the neighbour index - by a few rows either way
        run = int(rng.integers(2049 if past_near else 2040, 2061)) if (n < 4200 or rng.random() < 0.5) else int(rng.integers(4090, 4101))
        a = int(rng.integers(1, n - run))
        tv = rng.random(n) >= 0.02
        tv[a:a + run] = False
    elif mode == "edge-runs":
        tv = rng.random(n) >= 0.03
        for _ in range(int(rng.integers(1, 5))):
            step = int([32, 64, 64, 4096][int(rng.integers(0, 4))])
            first = (-pad) % step or step                       # the first row behind row 0 whose bit (pad + i) opens a word (a block)
            if first >= n:
                step = 32
                first = (-pad) % step or step
            if first >= n:
                break
            edge = first + step * int(rng.integers(0, (n - 1 - first) // step + 1))
            run = int(rng.integers(1, 200)) if rng.random() < 0.7 else int(rng.integers(1, 3))
            if rng.random() < 0.5:
                tv[edge:edge + run] = False                      # begins on the edge
            else:
                tv[max(edge - run, 0):edge] = False              # ends right in front of it
            if rng.random() < 0.5 and 0 < edge < n:
                tv[edge if rng.random() < 0.5 else edge - 1] = True   # ... with a valid row right on / in front of the edge
    else:
        tv[:] = False
    tv[0] = True
    if null_last is None:
        null_last = rng.random() < 0.05
    if n > 1:
        tv[-1] = not null_last
    return tv, mode


class Case:
    """one frame: the interval column (column 0) and `raw` value columns, all `pad` rows into longer buffers"""

    def __init__(self, ts, tvalid, pad, raw, rng, device, scramble):
        n = len(ts)
        self.n, self.pad, self.raw, self.device, self.tvalid = n, pad, raw, device, tvalid
        tot = pad + n + int(rng.integers(0, 9))
        buf = rng.integers(-2 ** 62, 2 ** 62, tot).astype(np.int64)
        ts = ts.copy()
        if scramble:                                             # a null slot's value is undefined in Arrow: nothing may depend on it
            nul = ~tvalid
            ts[nul] = rng.integers(-2 ** 62, 2 ** 62, int(nul.sum()))
        buf[pad:pad + n] = ts
        bits = rng.random(tot) < 0.5
        bits[pad:pad + n] = tvalid
        self.ts, self.ts_buf, self.tbm = ts, buf, np.packbits(bits, bitorder="little")

    def ocols(self):
        out = [orc.Column(self.ts_buf, self.tbm, orc.INT64, offset=self.pad, length=self.n)]
        for v, bm, typ, off in self.raw:
            out.append(orc.Column(v, bm, typ, offset=off, length=self.n))
        return out

    def ccols(self):
        out = [capi.Column(self.ts_buf, self.tbm, capi.INT64, self.pad, self.n, -1)]
        for v, bm, typ, off in self.raw:
            out.append(capi.Column(v, bm, typ, off, self.n, -1 if bm is not None else 0))
        return [c.to_device() for c in out] if self.device else out

    def plan(self):
        """(s0, W) of the frame's window grid for self.interval / self.offset"""
        return orc.plan_windows(self.ocols()[0], self.interval, self.offset)

    def a5_rows(self):
        s0, _W = self.plan()
        return int(rows_on_a_start_with_a_null_behind(self.ts, self.tvalid, s0, self.interval).sum())

    def outside(self):
        s0, _W = self.plan()
        return outside_inclusive_interpolate(self.ts, self.tvalid, s0, self.interval)


def value_cols(rng, n, pad, ncols):
    raw = []
    for _ in range(ncols):
        v, bm, typ, off = rand_col(rng, n, pad)
        if bm is not None and rng.random() < 0.2:                # (rand_col leaves one column in six without validity: a third in all)
            bm = None
        raw.append((v, bm, typ, off))
    return raw


def draw_pad(rng):
    return int(rng.integers(1, 70)) if rng.random() < 0.5 else 0


# ------------------------------------------------------------------ Rolling.Aggregate
def aggregate_cases(seed, cases=AGG_CASES):
    """Case objects with .interval .offset .aggs .inclusive (Options.Inclusive) .inclusive_call (... or a reducer implies it) .label.
    The first five cases of a seed are made to hold what chance would leave out of some seeds: a null run past 2048 / 4096 rows, a
    null last row, a reducer list that splits into batches, nanosecond-scale timestamps, and an inclusive call over small steps and
    a small interval with 30 % nulls - rows on window starts with a null behind them by the hundred."""
    rng = np.random.default_rng(11_000 + seed)
    for case in range(cases):
        rich = case == 4
        if case == 0:
            n = int([4097, 5000, 40_000][int(rng.integers(0, 3))])
        elif rich:
            n = int([2049, 4097, 5000][int(rng.integers(0, 3))])
        else:
            n = int(AGG_SIZES[int(rng.integers(0, len(AGG_SIZES)))]) if rng.random() < 0.8 else int(rng.integers(1, 3000))
        ts = rand_ts(rng, n)
        interval = int([1, 2, 3, 7, 10, 64, 100, 1000, 12345, 10 ** 6][int(rng.integers(0, 10))])
        if rich:
            ts = np.cumsum(rng.integers(0, 4, n)).astype(np.int64) + int(rng.integers(-2000, 2000))
            interval = int([1, 2, 3, 5][int(rng.integers(0, 4))])
        while (int(ts[-1]) - int(ts[0])) // interval > 1_500_000:
            interval *= 10  # keep the number of windows (output slots) reasonable
        ns = case == 3 or (rng.random() < 0.3 and not rich)
        if ns:
            # the same shape at nanosecond scale: rows span far more than 2^32 from the first window (magic_div over large intervals)
            scale = int(10 ** rng.integers(5, 10)) + int(rng.integers(0, 3))
            ts = ts * scale + int(rng.integers(-2, 3)) * 1_500_000_000_000_000_000 // 2
            interval *= scale
            if interval >= 2 ** 32 and rng.random() < 0.7:
                interval = int(rng.integers(1, 2 ** 32 - 1))
                while (int(ts[-1]) - int(ts[0])) // interval > 1_500_000:
                    interval = min(interval * 10, 2 ** 62)
        offset = int(rng.integers(-3 * interval, 3 * interval + 1))
        pad = draw_pad(rng)
        tvalid, vmode = interval_validity(rng, n, pad, mode="long-run" if case == 0 else "iid" if rich else None,
                                          null_last=True if case == 1 else False if rich else None, past_near=case == 0, frac=0.3 if rich else None)
        ncols = int(rng.integers(1, 4))
        c = Case(ts, tvalid, pad, value_cols(rng, n, pad, ncols), rng, device=bool(rng.random() < 0.4), scramble=bool(rng.random() < 0.5))
        linear = rich or rng.random() < 0.5
        kinds = list(ALL_AGGS) + [k for k in TIME_AGGS if linear or k not in LINEAR]
        na = int(rng.integers(17, 21)) if (case == 2 or rng.random() < 0.1) else int(rng.integers(1, 9))
        aggs = [("WindowStart", 0)]
        for _ in range(na):
            k = kinds[int(rng.integers(0, len(kinds)))]
            col = 0 if k == "WindowStart" else int(rng.integers(0 if rng.random() < 0.15 else 1, ncols + 1))
            if rng.random() < 0.25:
                aggs.append((k, col, [float(rng.choice([0.5, -1.0, 2.0, 0.1, 1e3])) for _ in range(int(rng.integers(1, 3)))]))
            else:
                aggs.append((k, col))
        c.interval, c.offset, c.aggs, c.ns, c.vmode = interval, offset, aggs, ns, vmode
        c.inclusive = bool(rng.random() < 0.4) or rich
        c.inclusive_call = c.inclusive or any(a[0] in LINEAR for a in aggs)
        c.planned = bool(rng.random() < 0.25)
        c.label = "seed=%d case=%d n=%d I=%d off=%d pad=%d %s incl=%d dev=%d" % (seed, case, n, interval, offset, pad, vmode, c.inclusive, c.device)
        yield c


# ------------------------------------------------------------------ Rolling.Interpolate, and Interpolate -> Aggregate as one call
def _interpolate_case(rng, seed, case, tag):
    # (sizes are bounded by the ORACLE: like the reference's GetPrevFloat64s walks it is cubic on all-null columns)
    n = int(rng.integers(1, 500)) if rng.random() < 0.7 else int(INTERP_SIZES[int(rng.integers(0, len(INTERP_SIZES)))])
    ts = rand_ts(rng, n)
    interval = int([1, 2, 5, 10, 64, 100, 1000][int(rng.integers(0, 7))])
    inclusive = bool(rng.random() < 0.4)
    rich = case < 2     # an inclusive call over small ascending steps and a small interval, 30 % nulls: SURVEY A.5 rows by the dozen
    if rich:
        n = int(rng.integers(400, 701))
        ts = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
        interval, inclusive = int(rng.integers(1, 4)), True
    if inclusive:
        # the domain interp_null_ts.cpp states for inclusive Interpolate: non-negative timestamps, 0 <= offset < interval, 0 <= s0 <= ts[0],
        # a span far below 2^31
        offset = int(rng.integers(0, interval))
        ts = ts - min(int(ts[0]), 0) + int(rng.integers(0, 50))
        if ts[0] < offset:
            ts = ts + offset
    else:
        offset = int(rng.integers(-2 * interval, 2 * interval + 1))
    pad = draw_pad(rng)
    tvalid, vmode = interval_validity(rng, n, pad, mode="iid" if rich else None, null_last=False if rich else None, frac=0.3 if rich else None)
    ncols = int(rng.integers(1, 4))
    raw = value_cols(rng, n, pad, ncols)
    windows = (int(ts[tvalid].max()) - int(ts[0])) // interval + 1
    for j, (v, bm, typ, off) in enumerate(raw):
        # (the oracle's neighbour walks are cubic on an all-null column: such a column under thousands of windows loses its bitmap)
        if bm is not None and windows * n * n > 50_000_000 and not np.unpackbits(bm, bitorder="little")[pad:pad + n].any():
            raw[j] = (v, None, typ, off)
    c = Case(ts, tvalid, pad, raw, rng, device=bool(rng.random() < 0.4), scramble=bool(rng.random() < 0.5))
    ip = [{"kind": "WindowStart", "col": 0}]
    for j in range(ncols):
        ip.append({"kind": ["Linear", "StepPrevious", "None"][int(rng.integers(0, 3))], "col": 1 + j})
        if rng.random() < 0.3:
            ip[-1]["prev"] = prev_row(int(ts[0]))
    c.interval, c.offset, c.inclusive, c.interps, c.vmode, c.ncols = interval, offset, inclusive, ip, vmode, ncols
    c.label = "%s seed=%d case=%d n=%d I=%d off=%d pad=%d %s incl=%d dev=%d %s" % (tag, seed, case, n, interval, offset, pad, vmode, inclusive, c.device,
                                                                                 [i_["kind"] for i_ in ip[1:]])
    return c


def interpolate_cases(seed, cases=INTERP_CASES):
    """Case objects with .interval .offset .inclusive .interps .label"""
    rng = np.random.default_rng(12_000 + seed)
    for case in range(cases):
        yield _interpolate_case(rng, seed, case, "interp")


def chain_cases(seed, cases=CHAIN_CASES):
    """Interpolate cases with .aggs on top: r.Interpolate(...).Aggregate(...) as one call (Options.Inclusive holds for both halves)"""
    rng = np.random.default_rng(13_000 + seed)
    for case in range(cases):
        c = _interpolate_case(rng, seed, case, "chain")
        kinds = list(rng.choice(ALL_AGGS[1:], size=int(rng.integers(1, 7))))
        aggs = [("WindowStart", 0)] + [(str(k), int(rng.integers(0 if k in ("Count", "NumRows") else 1, c.ncols + 1))) for k in kinds]
        if rng.random() < 0.3:
            i = int(rng.integers(1, len(aggs)))
            aggs[i] = aggs[i] + ([float(rng.choice([2.0, -1.0, 0.5, 1e3]))],)
        c.aggs = aggs
        c.label += " %s" % [a[0] for a in aggs]
        yield c
