"""GPU parity for the callers either side of Rolling.Aggregate (SURVEY §8 a16-a18 + f2):
Rolling.Interpolate, Bow.FillLinear / IsColSorted, window bounds (the iterator), whole-frame
Aggregate — golden vectors of the reference's tests plus seeded comparisons with the oracle."""
import numpy as np
import pytest

import whole_model as wm
from bow_amd import capi
from interp_model import TRIP, next_valid, plan as model_plan, prev_valid, trip_figures
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

T = {"float64": capi.FLOAT64, "int64": capi.INT64}


def same_list(a, b):
    assert len(a) == len(b), (a, b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or x == y), (a, b)


def _interps(spec):
    out = []
    for i, s in enumerate(spec):
        if s.startswith("Const:"):
            out.append({"kind": "Const", "col": i, "const": float(s.split(":")[1])})
        else:
            out.append({"kind": s, "col": i})
    return out


def both_interp_kernels(fn):
    """runs fn() under both Interpolate kernels - interp_wave3_kernel (the product's, for the usual shapes) and the workgroup kernel that
    serves the rest (capi.ROUTE_INTERP_TILE: the one kept second implementation) - checks that they agree bit for bit, returns the
    first result"""
    res = []
    for _label, mask in capi.INTERP_ROUTES:
        with capi.route(mask):
            res.append(fn())
    # ... and under the product kernel with device-resident outputs: bitmaps that reach the end of their last word are written in place
    # (no zeroing launch in front, the null counts summed from per-trip partials), a capacity of exactly the rows goes through the
    # working copies unless it happens to end on a word
    for padded in (True, False):
        with capi.interp_outputs(capi.DEVICE, padded):
            res.append(fn())
    a = res[0]
    for b in res[1:]:
        if isinstance(a, list) and a and isinstance(a[0], list):   # one list of columns per shard
            a_cols, b_cols = [c for sh in a for c in sh], [c for sh in b for c in sh]
        else:
            a_cols, b_cols = list(a), list(b)
        assert len(a_cols) == len(b_cols)
        for x, y in zip(a_cols, b_cols):
            assert x.length == y.length and x.null_count == y.null_count
            xv, xb = x.host_arrays()
            yv, yb = y.host_arrays()
            assert np.array_equal(xv.view(np.uint64), yv.view(np.uint64)) and np.array_equal(xb, yb)
    return a


def cmp_out(name, got, want):
    assert got.length == want.length, (name, got.length, want.length)
    gm, wm = got.valid_mask(), want.valid_mask()
    assert np.array_equal(gm, wm), (name, np.flatnonzero(gm != wm)[:10])
    gv, _ = got.host_arrays()
    wv = want.values[:want.length]
    gb_, wb_ = gv.view(np.uint64)[gm], wv.view(np.uint64)[wm]
    diff = gb_ != wb_
    if diff.any() and gv.dtype == np.float64:  # generated NaNs: hardware-default payload (see test_gpu_aggregate.compare)
        diff &= ~(np.isnan(gv[gm]) & np.isnan(wv[wm].view(np.float64)))
    assert not diff.any(), (name, np.flatnonzero(diff)[:10])
    assert got.null_count == int((~wm).sum()), name


# ------------------------------------------------------------------ Interpolate
def test_golden_interpolate(golden):
    for v in golden["interpolate"]:
        cols = [capi.Column.from_list(v["time"], "int64"), capi.Column.from_list(v["value"], "float64")]
        outs = capi.rolling_interpolate(cols, 0, v["interval"], _interps(v["interps"]), offset=v["offset"])
        same_list(outs[0].to_list(), v["expect_time"])
        same_list(outs[1].to_list(), v["expect_value"])


def test_interpolate_errors():
    cols = [capi.Column.from_list([10, 13], "int64"), capi.Column.from_list([1.0, 1.3], "float64")]
    with pytest.raises(capi.BowGpuError) as e:  # rolling/interpolation_test.go:37-47
        capi.rolling_interpolate(cols, 0, 2, [{"kind": "Const", "col": 1, "const": 9.9}])
    assert e.value.code == -5
    with pytest.raises(capi.BowGpuError) as e:  # WindowStart accepts Int64 only (windowstart.go:9)
        capi.rolling_interpolate(cols, 0, 2, [{"kind": "WindowStart", "col": 0}, {"kind": "WindowStart", "col": 1}])
    assert e.value.code == -7 and e.value.message == "accepts types [int64], got type float64"


@pytest.mark.parametrize("vtype", ["f64", "i64"])
def test_interpolate_random_vs_oracle(vtype):
    rng = np.random.default_rng(3)
    for n, interval, offset in [(1, 5, 0), (50, 3, 1), (5000, 10, 0), (60_000, 100, 7), (60_000, 7, 0)]:
        ts = np.cumsum(rng.integers(1, 20, n)).astype(np.int64) - 500
        if vtype == "f64":
            vals = np.round(rng.standard_normal(n) * 100, 2)
        else:
            vals = rng.integers(-1000, 1000, n).astype(np.int64)
        valid = rng.random(n) >= 0.3
        bm = np.packbits(valid, bitorder="little")
        typ = capi.FLOAT64 if vtype == "f64" else capi.INT64
        for kind in ["Linear", "StepPrevious", "None"]:
            for prev in [None, (float(ts[0] - 3), True, 42.5, True, 42)]:
                ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
                if prev is not None:
                    ip[1]["prev"] = prev
                got = both_interp_kernels(lambda: capi.rolling_interpolate([capi.Column(ts), capi.Column(vals, bm, typ, 0, n, -1)], 0, interval, ip,
                                                                           offset=offset))
                want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, typ)], 0, interval, ip, offset=offset)
                cmp_out("ts %s" % kind, got[0], want[0])
                cmp_out("val %s n=%d prev=%s" % (kind, n, prev is not None), got[1], want[1])


@pytest.mark.parametrize("vtype", ["f64", "i64"])
def test_interpolate_in_one_pass_without_a_count(vtype):
    """bowgpu_rolling_interpolate_fill on its own, without a preceding _count: the caller sizes the buffers (rows + windows at most), the
    call sets their length.  Inclusive windows take ONE pass over the rows (n_out = n + W - e0 needs no count; the fill kernel checks
    the order of the interval column itself); exclusive windows make their own count pass first (a look-back inside the fill kernel
    was measured slower: interpolate_api.cpp).  Equal to the oracle bit for bit; a buffer that is too small is an error that names the
    size, never a write past its end; an unsorted column is declined."""
    rng = np.random.default_rng(2604)
    typ = capi.FLOAT64 if vtype == "f64" else capi.INT64
    shapes = [(1, 5, 0), (700, 3, 1), (5000, 10, 0), (60_000, 100, 7), (60_000, 7, 0), (300_000, 4, 0), (300_000, 1000, 13)]
    for n, interval, offset in shapes:
        ts = np.cumsum(rng.integers(0, 20, n)).astype(np.int64) + 500
        if n > 1000:
            ts[n // 2:] += 20_000 * interval  # a long run of empty windows in the middle
            ts[n // 3: n // 3 + 2000] = ts[n // 3] - (ts[n // 3] % interval) + offset % interval   # rows sitting exactly on a window start, duplicated
            ts = np.sort(ts)
        vals = np.round(rng.standard_normal(n) * 100, 2) if vtype == "f64" else rng.integers(-1000, 1000, n).astype(np.int64)
        bm = np.packbits(rng.random(n) >= 0.3, bitorder="little")
        for kind in ("Linear", "StepPrevious"):
            ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
            for inclusive in (False, True):
                cols = [capi.Column(ts), capi.Column(vals, bm, typ, 0, n, -1)]
                want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, typ)], 0, interval, ip, offset=offset, inclusive=inclusive)
                for res in (capi.HOST, capi.DEVICE):
                    got = capi.rolling_interpolate_onepass(cols, 0, interval, ip, offset=offset, inclusive=inclusive, out_residency=res)
                    cmp_out("one pass ts %s n=%d I=%d incl=%s" % (kind, n, interval, inclusive), got[0], want[0])
                    cmp_out("one pass val %s n=%d I=%d incl=%s" % (kind, n, interval, inclusive), got[1], want[1])
                # buffers of exactly the right size, and one slot short
                exact = capi.rolling_interpolate_onepass(cols, 0, interval, ip, offset=offset, inclusive=inclusive, capacity=want[0].length)
                cmp_out("one pass exact capacity", exact[1], want[1])
                if want[0].length > n:
                    with pytest.raises(capi.BowGpuError) as e:
                        capi.rolling_interpolate_onepass(cols, 0, interval, ip, offset=offset, inclusive=inclusive, capacity=want[0].length - 1)
                    assert e.value.code == -10 and str(want[0].length) in e.value.message, e.value.message
    # not ascending: declined by the fill kernel's own check (there is no count pass to notice)
    ts = np.arange(100_000, dtype=np.int64) * 3
    ts[77_777] = 5
    vals = rng.standard_normal(100_000)
    for inclusive in (False, True):
        with pytest.raises(capi.BowGpuError) as e:
            capi.rolling_interpolate_onepass([capi.Column(ts), capi.Column(vals, None, capi.FLOAT64)], 0, 10,
                                             [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}], inclusive=inclusive)
        assert e.value.code == -14
    # ... and with the disorder at the END of the column: the one-pass row count comes from the first and the last timestamp alone, so
    # it is tiny here and nearly every trip also fails the "fits the counted range" check - the answer is still the decline (-14: the
    # caller keeps the reference's path), not the argument error of a column that changed between _count and _fill (-10)
    for tail in (1, 700):
        ts = np.arange(100_000, dtype=np.int64) * 3 + 100
        ts[-tail:] = 105
        for inclusive in (False, True):
            with pytest.raises(capi.BowGpuError) as e:
                capi.rolling_interpolate_onepass([capi.Column(ts), capi.Column(vals, None, capi.FLOAT64)], 0, 10,
                                                 [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}], inclusive=inclusive)
            assert e.value.code == -14, (tail, inclusive, e.value.code, e.value.message)


def test_interpolate_neighbour_points_thousands_of_null_rows_away():
    """interp_wave3_kernel looks a synthetic row's neighbour points up without the neighbour index (round 5: a walk over at most 64
    validity words; the index cost three launches per column and call); a point further away raises status[7] and the call is repeated
    with the index built.  Runs of 2500 .. 3000 nulls in front of, behind and across window starts (the ORACLE, like the reference's
    GetPrevFloat64s walks, is quadratic in the run length: sizes stay small), both interpolators that look for neighbours, both kernels."""
    rng = np.random.default_rng(41)
    n = 60_000
    ts = np.arange(n, dtype=np.int64) * 3 + 1        # (no row on a window start: every window gets a synthetic row)
    vals = np.round(rng.standard_normal(n) * 100, 2)
    valid = rng.random(n) >= 0.2
    for a, b in ((10_000, 13_000), (30_000, 32_500), (45_000, 45_700), (n - 2_600, n)):
        valid[a:b] = False
    valid[:2_500] = False                             # ... and no previous point at all for the first windows
    bm = np.packbits(valid, bitorder="little")
    for kind in ("Linear", "StepPrevious"):
        ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
        for interval, offset in ((60, 0), (3000, 7)):
            got = both_interp_kernels(lambda: capi.rolling_interpolate([capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)], 0, interval, ip, offset=offset))
            want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip, offset=offset)
            cmp_out("far neighbours ts %s I=%d" % (kind, interval), got[0], want[0])
            cmp_out("far neighbours val %s I=%d" % (kind, interval), got[1], want[1])
            one = capi.rolling_interpolate_onepass([capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)], 0, interval, ip, offset=offset, inclusive=True)
            want_i = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip, offset=offset, inclusive=True)
            cmp_out("far neighbours, inclusive one pass %s I=%d" % (kind, interval), one[1], want_i[1])


@pytest.mark.parametrize("base_ts", [0, 1_700_000_000_000, -(1 << 40), (1 << 52)])
def test_interpolate_frames_spanning_more_than_2_31(base_ts):
    """millisecond / microsecond timestamps: the frame spans far more than 2^31 from its first window start (round 2's wave kernels
    declined that: every row had to lie within 2^31 of s0).  interp_wave3_kernel's arithmetic is relative to each 512-row trip;
    a single trip that spans more (a gap of 3e9 inside it) is redone by the workgroup kernel.  All kernels bit for bit + the oracle."""
    rng = np.random.default_rng(17)
    n = 40_000
    step = rng.integers(1, 200_000, n)
    for with_jump in (False, True):
        st = step.copy()
        if with_jump:
            st[n // 2] = 3_000_000_000
        ts = np.cumsum(st).astype(np.int64) + base_ts
        assert int(ts[-1]) - int(ts[0]) > (1 << 31)
        vals = np.round(rng.standard_normal(n) * 100, 2)
        valid = rng.random(n) >= 0.3
        bm = np.packbits(valid, bitorder="little")
        for interval, offset in ((60_000, 0), (1_000_000, 7), (10_000_000, -3)):
            if with_jump and interval < 1_000_000:
                continue       # (millions of empty windows behind the jump: covered by the empty-window-runs test at a friendlier size)
            for kind in ("Linear", "StepPrevious"):
                ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
                got = both_interp_kernels(lambda: capi.rolling_interpolate([capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)], 0,
                                                                           interval, ip, offset=offset))
                want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip, offset=offset)
                cmp_out("wide ts %s I=%d jump=%s" % (kind, interval, with_jump), got[0], want[0])
                cmp_out("wide val %s I=%d jump=%s" % (kind, interval, with_jump), got[1], want[1])
                # INCLUSIVE windows on the same frames: only interp_wave3_kernel's trip-relative form takes a frame wider than 2^31.
                # Without the jump it equals the oracle; with it (one trip spans 3e9) there is no second kernel for inclusive
                # windows: the call must be declined, never answered with the exclusive layout
                cols = [capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)]
                below_s0 = capi.plan_windows(cols[0], interval, offset)[0] > int(ts[0])   # negative timestamps: Go's truncating division
                if with_jump or below_s0:                                                 # (rows below s0 + inclusive windows: declined as before)
                    with pytest.raises(capi.BowGpuError) as ei:
                        capi.rolling_interpolate(cols, 0, interval, ip, offset=offset, inclusive=True)
                    assert ei.value.code == -9   # BOWGPU_ERR_UNSUPPORTED
                else:
                    goti = capi.rolling_interpolate(cols, 0, interval, ip, offset=offset, inclusive=True)
                    wanti = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip,
                                            offset=offset, inclusive=True)
                    cmp_out("wide inclusive ts %s I=%d" % (kind, interval), goti[0], wanti[0])
                    cmp_out("wide inclusive val %s I=%d" % (kind, interval), goti[1], wanti[1])


def test_interpolate_empty_window_runs_and_the_minus_one_sentinel():
    # (1) long runs of empty windows (thousands of synthetic rows in front of one row, more than a tile stages in LDS);
    # (2) the reference's sentinel: an EMPTY window whose start is -1 gets no synthetic row, because "no first value" is
    #     encoded as -1 and compares equal to the window start (interpolation.go:119-125)
    rng = np.random.default_rng(12)
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}, {"kind": "StepPrevious", "col": 2}]

    def check(ts, interval, offset):
        n = len(ts)
        v1 = np.round(rng.standard_normal(n) * 10, 1)
        v2 = rng.integers(-50, 50, n).astype(np.int64)
        m1, m2 = rng.random(n) >= 0.3, rng.random(n) >= 0.3
        b1, b2 = np.packbits(m1, bitorder="little"), np.packbits(m2, bitorder="little")
        got = both_interp_kernels(lambda: capi.rolling_interpolate(
            [capi.Column(ts), capi.Column(v1, b1, capi.FLOAT64, 0, n, -1), capi.Column(v2, b2, capi.INT64, 0, n, -1)], 0, interval, ip, offset=offset))
        want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(v1, b1, orc.FLOAT64), orc.Column(v2, b2, orc.INT64)],
                               0, interval, ip, offset=offset)
        for c in range(3):
            cmp_out("col %d I=%d off=%d" % (c, interval, offset), got[c], want[c])
        return got[0].length - n

    step = rng.integers(1, 4, 30_000)
    step[rng.random(30_000) < 0.003] = rng.integers(5_000, 60_000)
    added = check(np.cumsum(step).astype(np.int64) - 1_000_000, 7, 2)
    assert added > 100_000
    # window starts = 4 (mod 5): ..., -6, -1, 4, ...; the window [-1, 4) is empty in the first two, not in the third
    assert check(np.array([-11, -9, 6, 7], dtype=np.int64), 5, 4) == 2      # windows -11, -6 (exact / synthetic), NOT -1, then 4
    # s0 = -1 above ts[0] = -3 (Go's truncating division) and window 0 = [-1, 4) has no row of its own: the row
    # below s0 belongs to no window and is dropped; window 0 gets no synthetic row either (sentinel); window 1 gets one (4)
    assert check(np.array([-3, 6, 7], dtype=np.int64), 5, 4) == 0
    assert check(np.array([-8, -7, 4, 9], dtype=np.int64), 5, 4) == -1      # -8, -7 dropped; synthetic -6; none for -1; 4 exact
    assert check(np.array([-8, -7, -3, 4, 9], dtype=np.int64), 5, 4) == 1   # window 0 has -3: nothing dropped
    assert check(np.array([-3, -2], dtype=np.int64), 5, 4) == -2            # no window at all => empty result
    check(np.array([-11, -9, 0, 6, 7], dtype=np.int64), 5, 4)
    check(np.array([-1, 3, 4, 9, 30], dtype=np.int64), 5, 4)                # -1 is an exact head
    # rows below s0 (Go's truncating division) with s0 = -1
    check(np.array([-3, -2, 8, 9], dtype=np.int64), 5, 4)
    check(np.array([-3, -2, 0, 8, 9], dtype=np.int64), 5, 4)


@pytest.mark.parametrize("inclusive", [False, True])
def test_interpolate_trips_with_more_outputs_than_the_stage_holds(inclusive):
    """512-row trips that produce more than 768 rows with few enough runs for interp_wave3_kernel's list: its UNSTAGED form - outputs
    stored from the lanes, validity bits ORed into the bitmap.  With the bitmaps written in place (device-resident outputs whose
    capacity reaches the end of the last word; round 5) nobody zeroes them beforehand: such a trip zeroes the words it owns itself.
    Every variant of both_interp_kernels - working copies, in place, the workgroup kernel for exclusive windows - gives the
    oracle's rows, and so does a second call into the SAME dirty output buffers."""
    rng = np.random.default_rng(77)
    interval, rows_per_window, nwin = 100, 8, 2_500
    starts = np.cumsum(rng.integers(6, 16, nwin)) * interval              # 5 .. 14 empty windows in front of every window with rows
    offs = np.sort(rng.integers(1, interval, (nwin, rows_per_window)), axis=1)
    ts = (starts[:, None] + offs).reshape(-1).astype(np.int64)
    assert np.all(np.diff(ts) >= 0)
    n = len(ts)
    vals = np.round(rng.standard_normal(n) * 10, 1)
    valid = rng.random(n) >= 0.3
    bm = np.packbits(valid, bitorder="little")
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
    want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip, inclusive=inclusive)
    assert want[0].length > 2 * n      # ~1.3 synthetic rows per row: ~1200 outputs per trip
    cols = [capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)]
    if inclusive:
        res = []
        for resid, padded in ((capi.HOST, True), (capi.DEVICE, True), (capi.DEVICE, False)):
            with capi.interp_outputs(resid, padded):
                res.append(capi.rolling_interpolate(cols, 0, interval, ip, inclusive=True))
    else:
        res = [both_interp_kernels(lambda: capi.rolling_interpolate(cols, 0, interval, ip))]
    for got in res:
        for c in range(2):
            cmp_out("col %d" % c, got[c], want[c])
    # the same output buffers again, full of the first call's bits
    dcols = [c_.to_device() for c_ in cols]
    outs = None
    for _ in range(2):
        outs = capi.rolling_interpolate_onepass(dcols, 0, interval, ip, inclusive=inclusive, out_residency=capi.DEVICE,
                                                capacity=(want[0].length + 511) // 512 * 512, outs=outs)
        for c in range(2):
            cmp_out("again, col %d" % c, outs[c], want[c])


def test_interpolate_a_wide_bow():
    """a Bow of 21 columns (the tile kernel takes 8 per launch; interpolation.go:98-161 loops over any number)"""
    rng = np.random.default_rng(23)
    n = 3000
    ts = np.cumsum(rng.integers(1, 9, n)).astype(np.int64)
    ccols, ocols, ip = [capi.Column(ts, None, capi.INT64)], [orc.Column(ts, None, orc.INT64)], [{"kind": "WindowStart", "col": 0}]
    for j in range(1, 21):
        as_int = j % 4 == 0
        v = rng.integers(-50, 50, n).astype(np.int64) if as_int else np.round(rng.standard_normal(n), 2)
        bm = None if j % 5 == 0 else np.packbits(rng.random(n) > 0.3, bitorder="little")
        typ = capi.INT64 if as_int else capi.FLOAT64
        ccols.append(capi.Column(v, bm, typ, 0, n, -1 if bm is not None else 0))
        ocols.append(orc.Column(v, bm, typ))
        ip.append({"kind": ["Linear", "StepPrevious", "None"][j % 3], "col": j})
    got = both_interp_kernels(lambda: capi.rolling_interpolate(ccols, 0, 10, ip, offset=3))
    want = orc.interpolate(ocols, 0, 10, ip, offset=3)
    assert len(got) == 21
    for j, (g, w) in enumerate(zip(got, want)):
        cmp_out("wide bow column %d" % j, g, w)


def test_interpolate_across_long_null_runs():
    # runs of nulls longer than a 4096-bit block of the neighbour index, with irregular ts: Linear / StepPrevious at every
    # window start inside a run reach the same two far-away neighbours.  (Sizes are bounded by the ORACLE: like the reference's
    # GetPrevFloat64s it is quadratic in the run length per window.)
    rng = np.random.default_rng(5)
    n = 40_000
    ts = np.cumsum(rng.integers(1, 20, n)).astype(np.int64)
    vals = np.round(rng.standard_normal(n) * 100, 2)
    valid = rng.random(n) >= 0.3
    valid[2_000:7_000] = False      # crosses the block boundaries at bits 4096 (and 8192 with the Arrow offset below)
    valid[20_470:24_600] = False    # starts just before bit 20480 = 5 * 4096
    valid[:7] = False
    valid[-9:] = False
    bm = np.packbits(valid, bitorder="little")
    for off in (0, 1500):
        m = n - off
        for kind in ("Linear", "StepPrevious"):
            ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
            got = both_interp_kernels(lambda: capi.rolling_interpolate(
                [capi.Column(ts, None, capi.INT64, off, m, 0), capi.Column(vals, bm, capi.FLOAT64, off, m, -1)], 0, 1000, ip, offset=3))
            want = orc.interpolate([orc.Column(ts, None, orc.INT64, offset=off, length=m),
                                    orc.Column(vals, bm, orc.FLOAT64, offset=off, length=m)], 0, 1000, ip, offset=3)
            cmp_out("ts " + kind, got[0], want[0])
            cmp_out("val " + kind, got[1], want[1])


def test_interpolate_then_mean_sparse_generator():
    # configs[2]: irregular ts, 30 % nulls, Linear fill then rolling mean - both stages on the device
    n = 300_000
    ts_d, val_d = capi.gen_sparse(0, n, seed=11)
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
    filled = capi.rolling_interpolate([ts_d, val_d], 0, 100, ip, out_residency=capi.DEVICE)
    ts_o, val_o, bm_o = orc.gen_sparse(0, n, seed=11)
    want = orc.interpolate([orc.Column(ts_o, None, orc.INT64), orc.Column(val_o, bm_o, orc.FLOAT64)], 0, 100, ip)
    cmp_out("ts", filled[0], want[0])
    cmp_out("val", filled[1], want[1])
    m = filled[0].length
    cols2 = [capi.Column(filled[0].values, None, capi.INT64, 0, m, 0), capi.Column(filled[1].values, filled[1].validity, capi.FLOAT64, 0, m, -1)]
    aggs = [("WindowStart", 0), ("ArithmeticMean", 1), ("Count", 1)]
    outs, _ = capi.rolling_aggregate(cols2, 0, 100, aggs)
    exp, _ = orc.aggregate([want[0], want[1]], 0, 100, aggs)
    for (k, _), g, w in zip(aggs, outs, exp):
        cmp_out(k, g, w)


# ------------------------------------------------------------------ FillLinear / IsColSorted
def test_golden_fill_linear(golden):
    names = ["a", "b", "c", "d", "e"]
    for v in golden["fill_linear"]:
        cols = [capi.Column.from_list([None if x is None else (float(x) if v["type"] == "float64" else x)
                                       for x in golden["fill_bow"][n]], v["type"]) for n in names]
        ref, fill = names.index(v["ref"]), names.index(v["fill"])
        if v.get("error"):
            with pytest.raises(capi.BowGpuError) as e:
                capi.fill_linear(cols, ref, fill)
            assert e.value.code == -8
            continue
        out, unchanged = capi.fill_linear(cols, ref, fill)
        assert not unchanged and out.type == T[v["type"]]
        same_list(out.to_list(), v["expect"])
    m = golden["fill_linear_meta"]
    cols = [capi.Column.from_list(m["ref"], m["ref_type"]), capi.Column.from_list(m["fill"], m["fill_type"])]
    out, _ = capi.fill_linear(cols, 0, 1)
    same_list(out.to_list(), m["expect"])


@pytest.mark.parametrize("ftype", ["f64", "i64"])
@pytest.mark.parametrize("desc", [False, True])
def test_fill_linear_random_vs_oracle(ftype, desc):
    rng = np.random.default_rng(17)
    n = 100_000
    ref = np.cumsum(rng.integers(0, 5, n)).astype(np.float64) * 0.5
    if desc:
        ref = ref[::-1].copy()
    ref_valid = rng.random(n) >= 0.1
    fill = np.round(rng.standard_normal(n) * 1000, 1) if ftype == "f64" else rng.integers(-10**6, 10**6, n).astype(np.int64)
    fill_valid = rng.random(n) >= 0.4
    fill_valid[:3] = False  # leading nulls have no previous value
    rb, fb = np.packbits(ref_valid, bitorder="little"), np.packbits(fill_valid, bitorder="little")
    ftyp = capi.FLOAT64 if ftype == "f64" else capi.INT64
    want, wu = orc.fill_linear([orc.Column(ref, rb, orc.FLOAT64), orc.Column(fill, fb, ftyp)], 0, 1)
    for resid, cap in ((capi.DEVICE, None), (capi.DEVICE, (n + 511) // 512 * 512)):   # (device-resident outputs: exact capacity, padded = bitmap in place)
        got, unchanged = capi.fill_linear([capi.Column(ref, rb, capi.FLOAT64, 0, n, -1), capi.Column(fill, fb, ftyp, 0, n, -1)], 0, 1,
                                          out_residency=resid, capacity=cap)
        assert unchanged == wu
        cmp_out("FillLinear, device-resident output", got, want)
    got, unchanged = capi.fill_linear([capi.Column(ref, rb, capi.FLOAT64, 0, n, -1), capi.Column(fill, fb, ftyp, 0, n, -1)], 0, 1)
    assert unchanged == wu
    cmp_out("fill", got, want)
    # bowgpu_fill_linear_sorted: the caller's own bowfill.go:35-42 has run (the cgo hook's position) - same result, no second order check
    got, unchanged = capi.fill_linear([capi.Column(ref, rb, capi.FLOAT64, 0, n, -1), capi.Column(fill, fb, ftyp, 0, n, -1)], 0, 1, ref_checked=True)
    assert unchanged == wu
    cmp_out("fill, ref checked by the caller", got, want)
    # no nulls => the reference returns the receiver
    got, unchanged = capi.fill_linear([capi.Column(ref, rb, capi.FLOAT64, 0, n, -1), capi.Column(fill, None, ftyp)], 0, 1)
    assert unchanged and got.null_count == 0


# ------------------------------------------------------------------ FillPrevious / FillNext / FillMean
def test_golden_fill_previous_next_mean(golden):
    # bowfill_test.go:29-154, :204-330
    for typ, methods in golden["fill_methods"].items():
        for method, expect in methods.items():
            for name in ["a", "b", "c", "d", "e"]:
                data = [None if x is None else (float(x) if typ == "float64" else x) for x in golden["fill_bow"][name]]
                out, unchanged = capi.fill(capi.Column.from_list(data, typ), method)
                assert not unchanged and out.type == T[typ]
                same_list(out.to_list(), expect[name])
    out, unchanged = capi.fill(capi.Column.from_list([1, 2, 3], "int64"), "Mean")
    assert unchanged and out.to_list() == [1, 2, 3]


@pytest.mark.parametrize("ftype", ["f64", "i64"])
@pytest.mark.parametrize("method", ["Previous", "Next", "Mean"])
def test_fill_random_vs_oracle(ftype, method):
    rng = np.random.default_rng(41)
    for n, null_frac, off in [(1, 1.0, 0), (7, 0.5, 0), (100_000, 0.4, 0), (100_000, 0.4, 13), (300_000, 0.999, 5)]:
        tot = n + off + 9
        vals = np.round(rng.standard_normal(tot) * 1000, 1) if ftype == "f64" else rng.integers(-10**12, 10**12, tot).astype(np.int64)
        valid = rng.random(tot) >= null_frac
        bm = np.packbits(valid, bitorder="little")
        typ = capi.FLOAT64 if ftype == "f64" else capi.INT64
        want, wu = orc.fill(orc.Column(vals, bm, typ, offset=off, length=n), method)
        # host-resident output; device-resident with a capacity of exactly the rows (bitmap through the working copy unless it ends on a
        # 64-bit word) and padded to 512 rows (the Arrow allocators' 64 bytes: bitmap written in place, round 5)
        for resid, cap in ((capi.HOST, None), (capi.DEVICE, None), (capi.DEVICE, (n + 511) // 512 * 512)):
            got, gu = capi.fill(capi.Column(vals, bm, typ, off, n, -1), method, out_residency=resid, capacity=cap)
            assert gu == wu
            cmp_out("%s n=%d off=%d" % (method, n, off), got, want)


def test_fill_long_null_runs_use_the_block_index():
    # runs of nulls far longer than a 4096-bit block of the neighbour index, starting / ending anywhere, plus leading and
    # trailing nulls (no previous / no next value).  The oracle (like the reference) walks row by row from every null row -
    # quadratic on such input - so the expectation here is numpy's forward / backward fill.
    n = 3_000_000
    valid = np.zeros(n, dtype=bool)
    valid[[5, 6, 4095, 4096, 4097, 1_000_000, 1_000_001, 2_500_123]] = True
    vals = np.arange(n, dtype=np.float64) * 0.5
    bm = np.packbits(valid, bitorder="little")
    for off in (0, 3):
        m = n - off
        v, ok = vals[off:], valid[off:]
        prev, nxt = prev_valid(ok), next_valid(ok)       # (tests/interp_model.py: np.maximum.accumulate / np.minimum.accumulate)
        exp = {"Previous": (np.where(prev >= 0, v[np.maximum(prev, 0)], 0.0), prev >= 0),
               "Next": (np.where(nxt < m, v[np.minimum(nxt, m - 1)], 0.0), nxt < m)}
        both = (prev >= 0) & (nxt < m)
        exp["Mean"] = (np.where(both, (v[np.maximum(prev, 0)] + v[np.minimum(nxt, m - 1)]) / 2, 0.0), both)
        for method in ("Previous", "Next", "Mean"):
            # (the kernel's bounded walk does not reach across these runs: the call is repeated with the neighbour index built - round 5)
            for cap in (None, (m + 511) // 512 * 512):
                got, _ = capi.fill(capi.Column(vals, bm, capi.FLOAT64, off, m, -1), method, out_residency=capi.DEVICE, capacity=cap)
                gv, gm = got.host_arrays()[0], got.valid_mask()
                wv, wm = exp[method]
                assert np.array_equal(gm, wm), (method, off)
                assert np.array_equal(gv[gm], wv[wm]), (method, off)
                assert got.null_count == int((~wm).sum())
    # FillLinear through the same index: ref = row number => linear in the row between the two valid neighbours
    ref = np.arange(n, dtype=np.int64)
    got, _ = capi.fill_linear([capi.Column(ref), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)], 0, 1)
    gv, gm = got.host_arrays()[0], got.valid_mask()
    idx = np.arange(n)
    prev, nxt = prev_valid(valid), next_valid(valid)
    both = (prev >= 0) & (nxt < n)
    assert np.array_equal(gm, both)
    p, q = np.maximum(prev, 0), np.minimum(nxt, n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        lin = (idx - p).astype(np.float64) / (q - p).astype(np.float64) * (vals[q] - vals[p]) + vals[p]  # bowfill.go:87-90
    sel = both & ~valid
    assert np.array_equal(gv[sel], lin[sel])
    assert np.array_equal(gv[valid], vals[valid])


def test_is_col_sorted():
    cases = [([1, 2, 2, 5], True), ([5, 4, 4, 1], True), ([1, 3, 2], False), ([None, None], False), ([], False),
             ([None, 1, None, 2, 3], True), ([3, None, 3, 3], True), ([1.0, float("nan"), 2.0], True)]
    for data, want in cases:
        typ = "float64" if any(isinstance(x, float) for x in data) else "int64"
        col = capi.Column.from_list(data, typ)
        assert capi.is_col_sorted(col) == want, data
        assert orc.is_col_sorted(orc.Column.from_list(data, typ)) == want, data


def test_is_col_sorted_across_trips():
    """the kernel works in 512-row trips joined afterwards: violations whose two rows lie in different trips (behind runs of
    nulls of any length), all-null stretches, Arrow offsets, both types"""
    rng = np.random.default_rng(17)
    for case in range(60):
        n = int(rng.choice([511, 512, 513, 1024, 5000, 140_000]))
        as_int = bool(rng.random() < 0.5)
        vals = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)
        if rng.random() < 0.3:
            vals = vals[::-1].copy()            # descending is sorted too (bowassertion.go:40-58)
        valid = rng.random(n) < [1.0, 0.7, 0.05][int(rng.integers(0, 3))]
        for _ in range(int(rng.integers(0, 3))):   # long runs of nulls over trip boundaries
            a = int(rng.integers(0, n)); valid[a:a + int(rng.integers(1, 3000))] = False
        if rng.random() < 0.6 and valid.sum() >= 3:  # one pair of consecutive valid rows out of order
            rows = np.flatnonzero(valid)
            j = int(rng.integers(1, len(rows)))
            vals[rows[j]:] += int(rng.choice([-1000, 1000]))
        if rng.random() < 0.1:
            valid[:] = False
        pad = int(rng.integers(0, 40))
        buf = np.concatenate([np.zeros(pad, np.int64), vals, np.zeros(5, np.int64)])
        vb = np.concatenate([np.ones(pad, bool), valid, np.ones(5, bool)])
        data = buf if as_int else buf.astype(np.float64)
        bm = None if valid.all() and rng.random() < 0.5 else np.packbits(vb, bitorder="little")
        typ = capi.INT64 if as_int else capi.FLOAT64
        got = capi.is_col_sorted(capi.Column(data, bm, typ, pad, n, -1 if bm is not None else 0))
        want = orc.is_col_sorted(orc.Column(data, bm, typ, offset=pad, length=n))
        assert got == want, (case, n, as_int, pad)


def test_is_col_sorted_without_nulls_every_neighbour_pair():
    """col_order_dense_kernel (round 6: a column without nulls in ONE launch - a row's left neighbour is the lane to the left, lane 63 of the
    group before, or the row in front of the trip): one pair out of order at every position that changes who the neighbour is (lane 0 / 63,
    128-row groups, 512-row trips, the ragged last trip), ascending and descending, both types, odd Arrow offsets (8-byte loads), NaN
    (compares false both ways: bowassertion.go:64-74) - against the oracle and against the general kernel (BOWGPU_ROUTE_FORCE_GENERAL)"""
    rng = np.random.default_rng(23)
    for n in (1, 2, 3, 127, 128, 129, 511, 512, 513, 640, 1024, 1537, 70_001):
        spots = sorted({p for p in (1, 2, 63, 64, 65, 126, 127, 128, 129, 255, 256, 383, 384, 510, 511, 512, 513, 1023, 1024, 1025, n - 2, n - 1,
                                    int(rng.integers(1, max(n, 2)))) if 1 <= p < n})
        for as_int in (True, False):
            for desc in (False, True):
                for pad in (0, 1):
                    base = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)
                    if desc:
                        base = base[::-1].copy()
                    for spot in [None] + spots:
                        vals = base.copy()
                        if spot is not None:
                            vals[spot:] += -10_000 if not desc else 10_000
                        buf = np.concatenate([np.full(pad, 7, np.int64), vals, np.zeros(3, np.int64)])
                        data = buf if as_int else buf.astype(np.float64)
                        if not as_int and spot is None and n > 4:
                            data[pad + n // 2] = np.nan
                        typ = capi.INT64 if as_int else capi.FLOAT64
                        col = capi.Column(data, None, typ, pad, n, 0)
                        want = orc.is_col_sorted(orc.Column(data, None, typ, offset=pad, length=n))
                        got = capi.is_col_sorted(col)
                        with capi.route(capi.ROUTE_FORCE_GENERAL):
                            general = capi.is_col_sorted(col)
                        assert got == want == general, (n, as_int, desc, pad, spot, got, want, general)
    dcol = capi.Column(np.arange(3_000_000, dtype=np.int64), None, capi.INT64).to_device()
    assert capi.is_col_sorted(dcol)
    z = np.zeros(1000, np.float64)
    assert capi.is_col_sorted(capi.Column(z, None, capi.FLOAT64)) == orc.is_col_sorted(orc.Column(z, None, capi.FLOAT64))   # all equal


# ------------------------------------------------------------------ window bounds (the iterator)
def test_golden_window_bounds(golden):
    for v in golden["iterate"]:
        ts = capi.Column.from_list(v["time"], "int64")
        s0, W, fi, sb, se, inc = capi.window_bounds(ts, v["interval"], v["offset"], v["inclusive"])
        assert W == len(v["windows"])
        for k, w in enumerate(v["windows"]):
            assert s0 + k * v["interval"] == w["start"]
            assert fi[k] == w["first_index"], (v["name"], k)
            assert [v["time"][r] for r in range(sb[k], se[k])] == w["time_rows"], (v["name"], k)


@pytest.mark.parametrize("inclusive", [False, True])
def test_window_bounds_random_vs_oracle(inclusive):
    rng = np.random.default_rng(8)
    for n, interval, offset in [(1, 3, 0), (5000, 4, 1), (80_000, 25, -3)]:
        ts = np.cumsum(rng.integers(0, 6, n)).astype(np.int64) - 40
        s0, W, fi, sb, se, inc = capi.window_bounds(capi.Column(ts), interval, offset, inclusive)
        wins = orc.iterate_windows(orc.Column(ts, None, orc.INT64), interval, offset, inclusive)
        assert W == len(wins)
        assert np.array_equal(fi, [w["first_index"] for w in wins])
        assert np.array_equal(sb, [w["slice_begin"] for w in wins])
        assert np.array_equal(se, [w["slice_end"] for w in wins])
        assert np.array_equal(inc, [w["is_inclusive"] for w in wins])


# ------------------------------------------------------------------ whole-frame Aggregate
def test_golden_whole(golden):
    for v in golden["whole"]:
        cols = [capi.Column.from_list(v["time"], "int64"), capi.Column.from_list(v["value"], "float64")]
        aggs = []
        for a in v["aggs"]:
            k, cname = a.split(":")
            aggs.append((k, 0 if cname == "time" else 1))
        outs = capi.aggregate_whole(cols, 0, aggs)
        for o, exp in zip(outs, v["expect"]):
            same_list(o.to_list(), exp)


def whole_within_the_stated_bound(label, aggs, got, ts, vals, valid, typ):
    """Sum / ArithmeticMean / the time-weighted reducers of one whole-frame call against tests/whole_model.py: bit for bit where every
    partial sum is exact, else |got - exact| within THE STATED TOLERANCE of one window of n rows (include/bowgpu.h, tests/tolerance.py)"""
    n = len(ts)
    want = wm.M.aggregate([wm.MCol(ts, np.ones(n, bool), wm.INT64), wm.MCol(vals, np.ones(n, bool) if valid is None else valid, typ)], 0, aggs)
    for a, g, w in zip(aggs, got, want):
        if a[0] not in wm.ORDER_SENSITIVE:
            continue
        assert g.null_count == (0 if w.valid else 1), (label, a)
        if not w.valid:
            continue
        x = float(g.host_arrays()[0].view(np.float64)[0])
        if not (np.isfinite(x) and np.isfinite(w.exact)):
            assert (np.isnan(x) and np.isnan(w.exact)) or x == w.exact, (label, a, x, w.exact)
        elif w.int_exact:
            assert x == w.as_float(), (label, a, x, w.as_float())
        else:
            assert abs(x - w.exact) <= wm.bound(w, a[0], []), (label, a, x, w.exact, wm.bound(w, a[0], []))


def test_whole_random_vs_oracle():
    rng = np.random.default_rng(23)
    n = 500_000
    ts = np.cumsum(rng.integers(1, 9, n)).astype(np.int64)
    vals = rng.standard_normal(n)
    valid = rng.random(n) >= 0.25
    bm = np.packbits(valid, bitorder="little")
    kinds = ["WindowStart", "Sum", "ArithmeticMean", "Min", "Max", "Count", "First", "Last", "IntegralStep",
             "IntegralTrapezoid", "WeightedAverageStep", "WeightedAverageLinear"]
    aggs = [(k, 0 if k == "WindowStart" else 1) for k in kinds]
    want = orc.aggregate_whole([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, aggs)
    # (round 5: whole_value_kernel<.., kTs> - terms with the next valid point found across lanes, chunks and steps; the shuffle-tree
    # kernel of rounds 1 - 4 stays behind ROUTE_FORCE_GENERAL as the second implementation)
    for mask in (0, capi.ROUTE_FORCE_GENERAL):
        with capi.route(mask):
            got = capi.aggregate_whole([capi.Column(ts), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)], 0, aggs)
        whole_within_the_stated_bound("random route=%d" % mask, aggs, got, ts, vals, valid, capi.FLOAT64)
        for k, g, w in zip(kinds, got, want):
            gl, wl = g.to_list(), w.to_list()
            assert len(gl) == len(wl) == 1 and (gl[0] is None) == (wl[0] is None), k
            if k in ("WindowStart", "Min", "Max", "Count", "First", "Last"):
                assert gl[0] == wl[0], k
            else:
                assert abs(gl[0] - wl[0]) <= 1e-10 * max(1.0, abs(wl[0])), (k, gl[0], wl[0])


def test_whole_time_weighted_sparse_points():
    """the integrals over the whole frame when valid points are rare and clustered: chunks, steps and whole wavefront ranges without
    a point, one point in the frame (no pair: nil), two points 100 000 rows apart, points only at the ends, Int64 values, slices"""
    rng = np.random.default_rng(77)
    kinds = ["IntegralStep", "IntegralTrapezoid", "WeightedAverageStep", "WeightedAverageLinear", "Count", "Last"]
    aggs = [(k, 1) for k in kinds]
    # (sizes of a few wavefront ranges, not more: the oracle - like the reference - walks to the next valid point from every row)
    for n, pts in ((5, [2]), (9_000, [2_000, 7_000]), (10_001, [0, 10_000]), (7_000, list(range(0, 7_000, 111))),
                   (9_457, sorted(rng.choice(9_457, 40, replace=False).tolist())), (4_000, []), (600, [0, 1, 2, 597, 598, 599])):
        for off in (0, 3):
            for typ_name in ("f64", "i64"):
                tot = n + off
                ts = np.cumsum(rng.integers(1, 50, tot)).astype(np.int64)
                vals = np.round(rng.standard_normal(tot) * 10, 1) if typ_name == "f64" else rng.integers(-100, 100, tot).astype(np.int64)
                valid = np.zeros(tot, dtype=bool)
                valid[[off + q for q in pts]] = True
                bm = np.packbits(valid, bitorder="little")
                typ = capi.FLOAT64 if typ_name == "f64" else capi.INT64
                want = orc.aggregate_whole([orc.Column(ts, None, orc.INT64, offset=off, length=n), orc.Column(vals, bm, typ, offset=off, length=n)], 0, aggs)
                for mask in (0, capi.ROUTE_FORCE_GENERAL):
                    with capi.route(mask):
                        got = capi.aggregate_whole([capi.Column(ts, None, capi.INT64, off, n, 0), capi.Column(vals, bm, typ, off, n, -1)], 0, aggs)
                    whole_within_the_stated_bound((n, off, typ_name, mask), aggs, got, ts[off:off + n], vals[off:off + n], valid[off:off + n], typ)
                    for k, g, w in zip(kinds, got, want):
                        gl, wl = g.to_list(), w.to_list()
                        assert (gl[0] is None) == (wl[0] is None), (k, n, off, typ_name, mask, gl, wl)
                        if gl[0] is not None:
                            assert abs(gl[0] - wl[0]) <= 1e-10 * max(1.0, abs(wl[0])), (k, n, off, typ_name, mask, gl[0], wl[0])


@pytest.mark.parametrize("vtype", ["f64", "i64"])
def test_whole_value_reducers_by_row_index(vtype):
    """aggregation.Aggregate with value reducers only takes whole_value_kernel (round 5): per-lane (value, row) pairs reduced by row
    index once per wavefront.  What depends on position - First / Last, the NaN seed of Min / Max, the EARLIEST of equal extremes
    (+0.0 / -0.0) - must come out as whole.go / minmax.go give it: sizes around the 512-row step and the workgroup chunk, Arrow slices
    at odd offsets (bitmap bit offsets 0 .. 7), NaN / signalling NaN / zeros of both signs planted first, last and in between."""
    rng = np.random.default_rng(5)
    kinds = ["Min", "Max", "First", "Last", "Count", "Sum", "ArithmeticMean"]
    aggs = [(k, 1) for k in kinds]
    for n in (1, 2, 7, 511, 512, 513, 4097, 70_001, 300_123):
        for off in (0, 1, 3, 5):
            for plant in ("none", "zeros", "nan-first", "nan-mid", "all-null", "no-bitmap"):
                tot = n + off + 5
                ts = np.arange(tot, dtype=np.int64)
                if vtype == "f64":
                    vals = np.round(rng.standard_normal(tot) * 100, 1)
                    if plant == "zeros":
                        vals[rng.random(tot) < 0.5] = 0.0
                        vals[rng.random(tot) < 0.3] = -0.0
                        vals = np.where(np.abs(vals) > 0, np.abs(vals), vals)       # zeros of both signs are the minimum
                    if plant == "nan-first":
                        vals[off] = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]   # a signalling NaN seed
                    if plant == "nan-mid" and n > 2:
                        vals[off + 1 + rng.integers(0, n - 1, max(1, n // 50))] = np.nan
                else:
                    vals = rng.integers(-1000, 1000, tot).astype(np.int64)
                    if plant == "zeros":
                        vals[rng.random(tot) < 0.6] = 0
                valid = rng.random(tot) >= 0.3
                if plant == "nan-first":
                    valid[off] = True
                if plant == "all-null":
                    valid[:] = False
                bm = None if plant == "no-bitmap" else np.packbits(valid, bitorder="little")
                typ = capi.FLOAT64 if vtype == "f64" else capi.INT64
                got = capi.aggregate_whole([capi.Column(ts, None, capi.INT64, off, n, 0), capi.Column(vals, bm, typ, off, n, -1 if bm is not None else 0)], 0, aggs)
                want = orc.aggregate_whole([orc.Column(ts, None, orc.INT64, offset=off, length=n), orc.Column(vals, bm, typ, offset=off, length=n)], 0, aggs)
                whole_within_the_stated_bound((n, off, plant), aggs, got, ts[off:off + n], vals[off:off + n], None if bm is None else valid[off:off + n], typ)
                for k, g, w in zip(kinds, got, want):
                    label = (k, n, off, plant)
                    w_null = w.to_list()[0] is None
                    assert g.length == w.length == 1 and g.null_count == (1 if w_null else 0), label
                    if w_null:
                        continue
                    gb, wb = g.host_arrays()[0].view(np.uint64)[0], w.values[:1].view(np.uint64)[0]
                    if k in ("Sum", "ArithmeticMean"):
                        gv, wv = g.host_arrays()[0].view(np.float64)[0], w.values[:1].view(np.float64)[0]
                        assert (np.isnan(gv) and np.isnan(wv)) or abs(gv - wv) <= 1e-10 * max(1.0, abs(wv)), label
                    else:
                        assert gb == wb, (label, hex(gb), hex(wb))


def test_window_bounds_across_a_gap_of_millions_of_empty_windows():
    """Two bursts of rows 3e8 apart with interval 10: 3e7 empty windows between them all take the second burst's first row as
    their FirstIndex.  One lane used to store them one by one (seconds); the grid fills long runs now."""
    import time
    a = np.arange(0, 1000, dtype=np.int64)
    gap = 300_000_000
    ts = np.concatenate([a, a + gap, a + 2 * gap + 5])
    col = capi.Column(ts, None, capi.INT64).to_device()
    capi.window_bounds(capi.Column(ts[:100], None, capi.INT64), 10)   # warm the context
    t0 = time.perf_counter()
    s0, W, first, lo, hi, inc = capi.window_bounds(col, 10)
    dt = time.perf_counter() - t0
    assert W == (2 * gap + 5 + 999) // 10 + 1 and s0 == 0
    k = np.arange(W, dtype=np.int64)
    want = np.searchsorted(ts, k * 10, side="left")        # FirstIndex = first row at or after the window start
    assert np.array_equal(first, want)
    empty = hi == lo
    assert empty.sum() == W - len(np.unique(ts // 10)) and np.array_equal(lo[~empty], want[~empty])
    assert dt < 5.0, dt     # (dominated by copying 4 x 8 x 6e7 bytes back to the host)


@pytest.mark.parametrize("vtype", ["f64", "i64"])
def test_interpolate_on_inclusive_windows(vtype):
    """Options.Inclusive + Interpolate: the reference concatenates the window bows, and an inclusive window's bow also holds the
    row that sits exactly on its end (rolling.go:201-209, interpolation.go:98-116) - that row appears twice.  Against the
    oracle's literal window walk: dense rows on the grid (every window start is a row), irregular rows, runs of empty windows."""
    rng = np.random.default_rng(21)
    typ = capi.FLOAT64 if vtype == "f64" else capi.INT64
    cases = []
    for n, interval, offset in [(1, 5, 0), (2, 5, 0), (40, 3, 1), (5000, 10, 0), (60_000, 100, 7), (30_000, 4, 0)]:
        cases.append((np.cumsum(rng.integers(1, 9, n)).astype(np.int64) + 3, interval, offset))
    cases.append((np.arange(0, 50_000, 5, dtype=np.int64), 10, 0))              # every other row sits on a window start
    cases.append((np.arange(0, 20_000, dtype=np.int64) * 10, 10, 0))            # every row does
    step = rng.integers(1, 4, 20_000)
    step[rng.random(20_000) < 0.004] = rng.integers(500, 20_000)
    cases.append((np.cumsum(step).astype(np.int64), 10, 3))                     # long runs of empty windows
    cases.append((np.repeat(np.arange(0, 3000, dtype=np.int64) * 7, 3), 7, 0))  # duplicated timestamps on window starts: only the first is the inclusive row
    for ts, interval, offset in cases:
        n = len(ts)
        vals = np.round(rng.standard_normal(n) * 100, 2) if vtype == "f64" else rng.integers(-1000, 1000, n).astype(np.int64)
        valid = rng.random(n) >= 0.3
        bm = np.packbits(valid, bitorder="little")
        for kind in ["Linear", "StepPrevious", "None"]:
            ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1}]
            got = capi.rolling_interpolate([capi.Column(ts).to_device(), capi.Column(vals, bm, typ, 0, n, -1).to_device()], 0, interval, ip,
                                           offset=offset, inclusive=True)
            want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, typ)], 0, interval, ip, offset=offset, inclusive=True)
            cmp_out("inclusive ts %s n=%d I=%d" % (kind, n, interval), got[0], want[0])
            cmp_out("inclusive val %s n=%d I=%d" % (kind, n, interval), got[1], want[1])
            plain = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, typ)], 0, interval, ip, offset=offset)
            assert want[0].length >= plain[0].length


def test_interpolate_count_to_fill_reuse_is_dropped_when_the_column_changes():
    """include/bowgpu.h, "CONTRACT between the two calls": a _fill that follows the _count of the same device-resident interval
    column reuses the count pass.  Writes and frees made through the library in between drop the reuse (the fill then scans the new
    data); a buffer rewritten behind the library's back is caught by the fill's own row count where the counts differ."""
    import ctypes as C
    rng = np.random.default_rng(12)
    n = 40_000
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
    L = capi.lib()

    def frame(seed, step):
        r = np.random.default_rng(seed)
        ts = np.cumsum(r.integers(1, step, n)).astype(np.int64)
        v = np.round(r.standard_normal(n), 3)
        m = r.random(n) > 0.3
        return ts, v, np.packbits(m, bitorder="little")

    ts_a, v_a, bm_a = frame(1, 9)
    ts_b, v_b, bm_b = frame(2, 25)       # other timestamps: another number of synthetic rows
    cols = [capi.Column(ts_a, None, capi.INT64).to_device(), capi.Column(v_a, bm_a, capi.FLOAT64, 0, n, -1).to_device()]
    carr, iarr = capi._cols(cols), capi._interps(ip)
    opts = capi.Options(0, 0, 0)

    def count():
        m = C.c_int64(0)
        capi.check(L.bowgpu_rolling_interpolate_count(carr, 2, 0, C.c_int64(10), C.byref(opts), iarr, 2, C.byref(m)))
        return m.value

    def fill(slots):
        outs = [capi.OutColumn(slots, capi.DEVICE) for _ in ip]
        oarr = (capi.Out * 2)()
        for i, o in enumerate(outs):
            oarr[i] = o.c()
        rc = L.bowgpu_rolling_interpolate_fill(carr, 2, 0, C.c_int64(10), C.byref(opts), iarr, 2, oarr)
        for i, o in enumerate(outs):
            o.absorb(oarr[i])
        return rc, outs

    want_a = orc.interpolate([orc.Column(ts_a, None, orc.INT64), orc.Column(v_a, bm_a, orc.FLOAT64)], 0, 10, ip)
    want_b = orc.interpolate([orc.Column(ts_b, None, orc.INT64), orc.Column(v_b, bm_b, orc.FLOAT64)], 0, 10, ip)
    assert want_a[0].length != want_b[0].length
    m_a = count()
    assert m_a == want_a[0].length
    rc, outs = fill(m_a)                                           # the ordinary pair of calls
    assert rc == 0
    cmp_out("reuse a ts", outs[0], want_a[0]); cmp_out("reuse a val", outs[1], want_a[1])
    # 1. the interval column rewritten THROUGH the library between the two calls: the fill scans the new column
    assert count() == m_a
    capi.check(L.bowgpu_memcpy_h2d(C.c_void_p(cols[0].values.ptr), ts_b.ctypes.data_as(C.c_void_p), C.c_int64(ts_b.nbytes)))
    rc, outs = fill(max(m_a, want_b[0].length) + 8)
    assert rc == 0 and outs[0].length == orc.interpolate([orc.Column(ts_b, None, orc.INT64), orc.Column(v_a, bm_a, orc.FLOAT64)], 0, 10, ip)[0].length
    # 2. ... behind the library's back (a raw hipMemcpy): the fill's own row count does not add up -> BOWGPU_ERR_ARG
    hip = capi.lib()     # hipMemcpy of the HIP runtime the library is linked to (torch may have loaded a second copy in this process)
    assert count() == outs[0].length
    assert hip.hipMemcpy(C.c_void_p(cols[0].values.ptr), ts_a.ctypes.data_as(C.c_void_p), C.c_size_t(ts_a.nbytes), 1) == 0
    rc, _ = fill(max(m_a, want_b[0].length) + 8)
    assert rc == -10 and b"changed between" in L.bowgpu_last_error()
    # ... and the thread goes on working: the same pair of calls on the column as it is now
    assert count() == m_a
    rc, outs = fill(m_a)
    assert rc == 0
    cmp_out("after the tampering, ts", outs[0], want_a[0]); cmp_out("after the tampering, val", outs[1], want_a[1])


def test_interpolate_redo_behind_a_reused_count():
    """A _fill that reuses its _count's pass 1 (device-resident columns, the ordinary pair of calls) and then meets a 512-row trip
    interp_wave3_kernel declines - here one that spans more than 2^31 from the start of its first row's window (interp_model.py
    trip_figures / outside_inclusive_interpolate) - makes pass 1 its own again before the workgroup kernel takes the call.  Exclusive
    windows: the oracle's rows, from interp_tile_kernel; the same frame without the gap: interp_wave3_kernel.  Inclusive windows have
    no second kernel: declined, behind a count and as one call alike."""
    rng = np.random.default_rng(31)
    n, interval, gap_row = 3_000, 10_000_000, 1_300          # (the gap lies inside trip 2: rows 1024 .. 1535)
    step = rng.integers(1, 200_000, n)
    vals = np.round(rng.standard_normal(n) * 100, 2)
    bm = np.packbits(rng.random(n) >= 0.3, bitorder="little")
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]

    def frame(with_gap):
        st = step.copy()
        if with_gap:
            st[gap_row] = 3_000_000_000
        ts = np.cumsum(st).astype(np.int64)
        span, crossed = trip_figures(ts, model_plan(ts, interval, 0)[0], interval)
        declined = (span >= 2 ** 31 - 1) | (crossed >= 0xFFFF - TRIP - 1)
        assert list(np.flatnonzero(declined)) == ([gap_row // TRIP] if with_gap else [])
        dcols = [capi.Column(ts, None, capi.INT64).to_device(), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1).to_device()]
        return ts, dcols

    for with_gap, kernel in ((True, "interp_tile_kernel"), (False, "interp_wave3_kernel")):
        ts, dcols = frame(with_gap)
        got = capi.rolling_interpolate(dcols, 0, interval, ip, out_residency=capi.DEVICE, padded=True)
        assert capi.last_kernel_name() == kernel, (with_gap, capi.last_kernel_name())
        want = orc.interpolate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, interval, ip)
        cmp_out("gap=%s ts" % with_gap, got[0], want[0])
        cmp_out("gap=%s val" % with_gap, got[1], want[1])
    ts, dcols = frame(True)
    for call in (capi.rolling_interpolate, capi.rolling_interpolate_onepass):
        with pytest.raises(capi.BowGpuError) as ei:
            call(dcols, 0, interval, ip, inclusive=True, out_residency=capi.DEVICE)
        assert ei.value.code == -9   # BOWGPU_ERR_UNSUPPORTED


@pytest.mark.parametrize("device", [False, True])
def test_interpolate_over_an_interval_column_with_nulls_more_than_sixteen_columns(device):
    """Round 6 (VERDICT r05 missing 5): a Bow of 21 columns over an interval column with nulls - BOWGPU_ERR_UNSUPPORTED until round 5 - goes
    through the compaction in groups of 15 value columns; every column against the oracle, exclusive and inclusive windows"""
    rng = np.random.default_rng(321)
    n = 20_000
    ts = np.cumsum(rng.integers(1, 9, n)).astype(np.int64)
    tv = rng.random(n) >= 0.25
    tv[0] = tv[-1] = True
    tbm = np.packbits(tv, bitorder="little")
    ccols, ocols, ip = [capi.Column(ts, tbm, capi.INT64, 0, n, -1)], [orc.Column(ts, tbm, orc.INT64)], [{"kind": "WindowStart", "col": 0}]
    kinds = ["Linear", "StepPrevious", "None"]
    for c in range(1, 21):
        as_int = c % 3 == 0
        v = rng.integers(-500, 500, n).astype(np.int64) if as_int else np.round(rng.standard_normal(n) * 50, 2)
        bm = np.packbits(rng.random(n) >= 0.1 * (c % 5), bitorder="little")
        typ = capi.INT64 if as_int else capi.FLOAT64
        ccols.append(capi.Column(v, bm, typ, 0, n, -1))
        ocols.append(orc.Column(v, bm, typ))
        ip.append({"kind": kinds[c % 3], "col": c})
    if device:
        ccols = [c.to_device() for c in ccols]
    for inclusive in (False, True):
        try:
            got = capi.rolling_interpolate(ccols, 0, 30, ip, offset=4, inclusive=inclusive)
        except capi.BowGpuError as e:     # (the two shapes inclusive iterations leave to the reference: include/bowgpu.h BOWGPU_ERR_TS_NULLS)
            assert inclusive and e.code == -13, e
            continue
        want = orc.interpolate(ocols, 0, 30, ip, offset=4, inclusive=inclusive)
        for k in range(21):
            cmp_out("21 columns, col %d inclusive=%s" % (k, inclusive), got[k], want[k])


def test_null_ts_fill_uses_what_its_count_built_and_notices_what_came_between():
    """Round 6 (ADVICE r04 / VERDICT r05 weak 10): over an interval column with nulls the _count's compaction of the kept rows stays for the
    _fill that follows it on the same DEVICE-resident columns (interp_null_ts.cpp NullTsState) instead of being built a second time.  The fill is
    right - against the oracle - when it follows its count, when a write through the library came between (the state is dropped), when
    ANOTHER frame's count came between, when it runs without a count, and when the interpolators differ from the count's."""
    import ctypes as C
    rng = np.random.default_rng(99)
    L = capi.lib()

    def frame(n, seed):
        r = np.random.default_rng(seed)
        ts = np.cumsum(r.integers(1, 9, n)).astype(np.int64)
        tv = r.random(n) >= 0.2
        tv[0] = tv[-1] = True
        v = np.round(r.standard_normal(n) * 10, 2)
        vv = r.random(n) >= 0.3
        tbm, vbm = np.packbits(tv, bitorder="little"), np.packbits(vv, bitorder="little")
        ccols = [capi.Column(ts, tbm, capi.INT64, 0, n, -1).to_device(), capi.Column(v, vbm, capi.FLOAT64, 0, n, -1).to_device()]
        ocols = [orc.Column(ts, tbm, orc.INT64), orc.Column(v, vbm, orc.FLOAT64)]
        return ccols, ocols

    def count(ccols, ip, interval):
        n_out = C.c_int64(0)
        opts = capi.Options(0, 0, 0)
        capi.check(L.bowgpu_rolling_interpolate_count(capi._cols(ccols), 2, 0, C.c_int64(interval), C.byref(opts), capi._interps(ip), 2, C.byref(n_out)))
        return n_out.value

    def fill(ccols, ip, interval, cap):
        outs = [capi.OutColumn((cap + 511) // 512 * 512, capi.HOST) for _ in ip]    # (host outputs: nothing is allocated on the device between the calls)
        oarr = (capi.Out * 2)()
        for i, o in enumerate(outs):
            oarr[i] = o.c()
        opts = capi.Options(0, 0, 0)
        capi.check(L.bowgpu_rolling_interpolate_fill(capi._cols(ccols), 2, 0, C.c_int64(interval), C.byref(opts), capi._interps(ip), 2, oarr))
        for i, o in enumerate(outs):
            o.absorb(oarr[i])
        return outs

    A, oA = frame(150_000, 1)
    B, oB = frame(90_000, 2)
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
    ip2 = [{"kind": "WindowStart", "col": 0}, {"kind": "StepPrevious", "col": 1}]
    wantA, wantB, wantA2 = orc.interpolate(oA, 0, 40, ip), orc.interpolate(oB, 0, 40, ip), orc.interpolate(oA, 0, 40, ip2)
    scratch = capi.DeviceBuffer(64)

    def check(label, got, want):
        for k in range(2):
            cmp_out("%s col %d" % (label, k), got[k], want[k])

    m = count(A, ip, 40)
    assert m == wantA[0].length
    check("fill right behind its count", fill(A, ip, 40, m), wantA)
    check("a fill on its own", fill(A, ip, 40, m), wantA)
    m = count(A, ip, 40)
    capi.check(L.bowgpu_memset(C.c_void_p(scratch.ptr), 0, C.c_int64(64)))        # a write through the library: the state is dropped
    check("a library write between count and fill", fill(A, ip, 40, m), wantA)
    m = count(A, ip, 40)
    mb = count(B, ip, 40)                                                          # another frame's count: the state is B's now
    check("A's fill after B's count", fill(A, ip, 40, m), wantA)
    mb = count(B, ip, 40)
    check("B's fill after B's count", fill(B, ip, 40, mb), wantB)
    m = count(A, ip, 40)
    check("other interpolators than the count's", fill(A, ip2, 40, m), wantA2)
    m = count(A, ip, 40)
    capi.trim(all_threads=False)                                                   # the blocks go back to the device: nothing dangles
    check("a trim between count and fill", fill(A, ip, 40, m), wantA)


@pytest.mark.parametrize("null_frac", [0.02, 0.3, 0.8])
def test_interpolate_over_an_interval_column_with_nulls(null_frac):
    """Rolling.Interpolate when the interval column has nulls (ts_nulls.hip): the output is the slices themselves -
    rows that belong to no window vanish (rolling.go:190-193, :224-228), null-timestamp rows inside a slice are copied with their
    null timestamp and their values' own validity, the interpolators look for neighbours among the rows whose timestamp AND value are
    valid (linear.go:20-31, stepprevious.go:19).  Every interpolator, a PrevRow, two value columns, both kernels, against the oracle."""
    rng = np.random.default_rng(int(null_frac * 100) + 7)
    seen_incl = [0]
    for n, interval, offset, mode in [(1, 10, 0, "dense"), (2, 3, 1, "dense"), (700, 5, 2, "dups"), (3000, 10, 0, "irregular"),
                                      (5000, 64, 7, "gappy"), (40_000, 25, -3, "irregular"), (40_000, 4000, 11, "dense"), (6000, 10, 3, "negative"),
                                      (9000, 1, 0, "dups"), (30_000, 4, 1, "dense")] + ([(3_000_000, 50, 7, "irregular")] if null_frac == 0.3 else []):
        if mode == "dense":
            ts = np.arange(n, dtype=np.int64) + int(rng.integers(-50, 50))
        elif mode == "dups":
            ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64) - 77
        elif mode == "gappy":
            step = rng.integers(1, 5, n)
            step[rng.random(n) < 0.01] = rng.integers(100, 5000)
            ts = np.cumsum(step).astype(np.int64) - 12345
        elif mode == "negative":
            ts = np.cumsum(rng.integers(1, 7, n)).astype(np.int64) - 3 * n
        else:
            ts = np.cumsum(rng.integers(1, 20, n)).astype(np.int64) + int(rng.integers(-1000, 1000))
        tvalid = rng.random(n) >= null_frac
        tvalid[0] = tvalid[-1] = True
        vals = np.round(rng.standard_normal(n) * 100, 2)
        ivals = rng.integers(-1000, 1000, n).astype(np.int64)
        v1, v2 = rng.random(n) >= 0.3, rng.random(n) >= 0.1
        tbm, b1, b2 = (np.packbits(x, bitorder="little") for x in (tvalid, v1, v2))
        for kinds in (("Linear", "StepPrevious"), ("StepPrevious", "None"), ("None", "Linear")):
            for prev in (None, (float(ts[0] - 3), True, 42.5, True, 42)):
                ip = [{"kind": "WindowStart", "col": 0}, {"kind": kinds[0], "col": 1}, {"kind": kinds[1], "col": 2}]
                if prev is not None:
                    ip[1]["prev"] = prev
                    ip[2]["prev"] = prev
                ccols = [capi.Column(ts, tbm, capi.INT64, 0, n, -1), capi.Column(vals, b1, capi.FLOAT64, 0, n, -1), capi.Column(ivals, b2, capi.INT64, 0, n, -1)]
                if n % 2 == 0:
                    ccols = [c.to_device() for c in ccols]
                got = both_interp_kernels(lambda: capi.rolling_interpolate(ccols, 0, interval, ip, offset=offset))
                ocols = [orc.Column(ts, tbm, orc.INT64), orc.Column(vals, b1, orc.FLOAT64), orc.Column(ivals, b2, orc.INT64)]
                want = orc.interpolate(ocols, 0, interval, ip, offset=offset)
                label = "n=%d I=%d %s %s prev=%s nulls=%.2f" % (n, interval, mode, kinds, prev is not None, null_frac)
                for k in range(3):
                    cmp_out("col %d %s" % (k, label), got[k], want[k])
                # inclusive windows (round 4): the window also takes the first row ON its end, the next one starts at `rowIndex - 1` - after null
                # rows without the row on its start, with a synthetic start row in its place.  Two shapes stay outside the device path: an
                # equal timestamp right behind those null rows, and such a row on -1 (interpolateWindow's "no first value")
                if n > 100_000:
                    continue
                s0, _W = orc.plan_windows(ocols[0], interval, offset)
                idx = np.arange(n)
                pv = np.concatenate(([-1], np.maximum.accumulate(np.where(tvalid, idx, -1))[:-1]))
                nxt = np.minimum.accumulate(np.where(tvalid, idx, n)[::-1])[::-1]
                nb = np.concatenate((nxt[1:], [n]))                      # next valid row behind row i
                quirk = np.zeros(n, bool)
                quirk[:-1] = tvalid[:-1] & ~tvalid[1:] & (ts[:-1] >= s0 + interval) & ((ts[:-1] - s0) % interval == 0)
                quirk &= (pv < 0) | (ts[np.maximum(pv, 0)] < ts)
                outside = bool((quirk & ((ts == -1) | ((nb < n) & (ts[np.minimum(nb, n - 1)] == ts))))[:n].any())
                if outside:
                    with pytest.raises(capi.BowGpuError) as e:
                        capi.rolling_interpolate(ccols, 0, interval, ip, offset=offset, inclusive=True)
                    assert e.value.code == -13
                    continue
                try:
                    got = capi.rolling_interpolate(ccols, 0, interval, ip, offset=offset, inclusive=True)
                except capi.BowGpuError as e:      # (negative window starts etc.: what inclusive Interpolate declines for ANY interval column)
                    assert e.code == -9 and "inclusive windows" in e.message, e
                    continue
                seen_incl[0] += int(quirk.sum())
                want = orc.interpolate(ocols, 0, interval, ip, offset=offset, inclusive=True)
                for k in range(3):
                    cmp_out("inclusive col %d %s" % (k, label), got[k], want[k])
    # the physically last timestamp null: HasNext is false from the start (rolling.go:162-173) - no window, no rows
    ts = np.array([10, 11, 20, 21, 30], dtype=np.int64)
    tvalid = np.array([1, 1, 0, 1, 0], bool)
    cols = [capi.Column(ts, np.packbits(tvalid, bitorder="little"), capi.INT64, 0, 5, -1), capi.Column(np.arange(5.0))]
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
    want = orc.interpolate([orc.Column(ts, np.packbits(tvalid, bitorder="little"), orc.INT64), orc.Column(np.arange(5.0), None, orc.FLOAT64)], 0, 10, ip)
    got = capi.rolling_interpolate(cols, 0, 10, ip)
    assert got[0].length == want[0].length == 0
    assert seen_incl[0] > 20 or null_frac > 0.5      # (rows on a window start with a null behind them went through the inclusive path)


@pytest.mark.parametrize("tail", [1, 63])
def test_interpolate_over_an_interval_column_with_nulls_row_count_beside_a_bitmap_word(tail):
    """the compacted call fills device temporaries that are handed to the caller's columns: an output of 64 k + 1 rows (one past a
    validity word) or 64 k + 63, nulls in that last word (interpolation.None keeps the value column's), host and device columns"""
    rng = np.random.default_rng(5)
    N, interval = 2400, 20
    ts = 2 * np.arange(N, dtype=np.int64) + 1
    tvalid = rng.random(N) >= 0.2
    tvalid[0] = True
    tvalid[-100:] = True                          # (every candidate frame below ends on a valid timestamp)
    vals = np.round(rng.standard_normal(N) * 100, 2)
    ivals = rng.integers(-1000, 1000, N).astype(np.int64)
    v1, v2 = rng.random(N) >= 0.3, rng.random(N) >= 0.1
    ip = [{"kind": "WindowStart", "col": 0}, {"kind": "None", "col": 1}, {"kind": "Linear", "col": 2}]

    def frame(n):
        w1 = v1[:n].copy()
        w1[-20:] = False
        tbm, b1, b2 = (np.packbits(x, bitorder="little") for x in (tvalid[:n], w1, v2[:n]))
        ccols = [capi.Column(ts[:n].copy(), tbm, capi.INT64, 0, n, -1), capi.Column(vals[:n].copy(), b1, capi.FLOAT64, 0, n, -1),
                 capi.Column(ivals[:n].copy(), b2, capi.INT64, 0, n, -1)]
        ocols = [orc.Column(ts[:n].copy(), tbm, orc.INT64), orc.Column(vals[:n].copy(), b1, orc.FLOAT64), orc.Column(ivals[:n].copy(), b2, orc.INT64)]
        return ccols, ocols

    for n in range(N, N - 100, -1):                # the longest frame whose output has the row count looked for
        ccols, ocols = frame(n)
        want = orc.interpolate(ocols, 0, interval, ip)
        if want[0].length % 64 == tail:
            break
    assert want[0].length % 64 == tail and want[1].to_list()[-1] is None
    for cols in (ccols, [c.to_device() for c in ccols]):
        got = both_interp_kernels(lambda: capi.rolling_interpolate(cols, 0, interval, ip))
        for k in range(3):
            cmp_out("col %d n=%d rows=%d" % (k, n, want[0].length), got[k], want[k])
