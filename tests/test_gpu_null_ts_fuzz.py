"""Differential fuzzing of the paths that serve an INTERVAL COLUMN WITH NULLS (bow_amd/csrc/ts_nulls.hip, aggregate_api.cpp
run_aggregate_null_ts, interp_null_ts.cpp) against the oracle: the seeded cases of tests/null_ts_cases.py - the interval column
and every value column at an Arrow offset inside longer buffers of random bits, row counts on the edges of the keep words and the
tiles, null runs past the near walk (2048 bits) and the blocks (4096) of the neighbour index and on its word edges, a null last row,
arbitrary bits in the timestamps of null rows, Int64 / Float64 value columns with and without validity, every reducer with Factor
chains, reducer lists that split into batches, nanosecond-scale timestamps - through every kernel route, strict_order, planned calls,
both Interpolate kernels, the one-pass fill, Interpolate -> Aggregate as one call and the fan-out's decline to one device
(BOW_FUZZ_SEEDS=N runs N / 2 seeds instead of 32).  Bit-exact except Sum / Mean / integrals of windows on an order-free path, which
must lie within the stated bound (tests/tolerance.py)."""
import os

import numpy as np
import pytest

import null_ts_cases as ntc
from bow_amd import capi
from oracle import pyoracle as orc
from test_gpu_aggregate import NULL_TS_AGGS_INCL, ORDER_SENSITIVE, compare
from test_gpu_callers import both_interp_kernels, cmp_out
from tolerance import order_free_bounds

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")) // 2)


def against_the_oracle(label, aggs, outs, info, exp, nic, bounds_of):
    assert info.new_interval_col == nic and info.num_windows == exp[0].length, label
    bounds = bounds_of() if info.long_windows else None
    for i, (a, g, w) in enumerate(zip(aggs, outs, exp)):
        exact = info.long_windows == 0 or a[0] not in ORDER_SENSITIVE
        compare("%s %s" % (label, a[0]), g, w, exact=exact, bound=None if exact else bounds[i])     # (lengths and null counts too)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_aggregate_null_interval_column(seed):
    for c in ntc.aggregate_cases(seed):
        ccols, ocols = c.ccols(), c.ocols()
        kw = dict(offset=c.offset, inclusive=c.inclusive)
        exp, nic = orc.aggregate(ocols, 0, c.interval, c.aggs, **kw)
        cache = []

        def bounds_of():
            if not cache:
                cache.append(order_free_bounds(ocols, 0, c.interval, c.aggs, ref=exp, **kw))
            return cache[0]

        for path in capi.agg_routes():
            outs, info = capi.rolling_aggregate(ccols, 0, c.interval, c.aggs, **kw)
            against_the_oracle("%s path=%s" % (c.label, path), c.aggs, outs, info, exp, nic, bounds_of)
            if c.n > 1 and not c.tvalid[-1]:      # HasNext is false from the start (rolling.go:162-173): W slots, all nil, for every reducer
                W = c.plan()[1]
                assert all(o.length == W and o.null_count == W and not o.valid_mask().any() for o in outs), c.label
        # bowgpu_options.strict_order: every window in row order - bit for bit; declined only when a window holds more than 2^20 rows
        try:
            outs, info = capi.rolling_aggregate(ccols, 0, c.interval, c.aggs, strict_order=True, **kw)
        except capi.BowGpuError as e:
            assert e.code == -9 and "2^20" in e.message, (c.label, e.message)
        else:
            assert info.long_windows == 0, c.label
            against_the_oracle(c.label + " strict", c.aggs, outs, info, exp, nic, None)
        if c.planned:                             # bowgpu_plan_windows_ex + bowgpu_rolling_aggregate_planned
            plan = capi.plan_windows_ex(ccols[0], c.interval, c.offset)
            assert (plan.s0, plan.num_windows) == c.plan(), c.label
            outs, info = capi.rolling_aggregate(ccols, 0, c.interval, c.aggs, plan=plan, **kw)
            against_the_oracle(c.label + " planned", c.aggs, outs, info, exp, nic, bounds_of)
        if not c.tvalid.all():                    # Mode over an interval column with nulls: declined, and that is all that is wrong
            with pytest.raises(capi.BowGpuError) as e:
                capi.rolling_aggregate(ccols, 0, c.interval, c.aggs + [("Mode", 1 + seed % len(c.raw))], **kw)
            assert e.value.code == -13, (c.label, e.value)


_inclusive = {"drawn": 0, "compared": 0, "declined": 0, "outside": 0}      # test_fuzz_interpolate_null_interval_column, over its seeds


def expects_ts_nulls(c):
    """inclusive Interpolate answers BOWGPU_ERR_TS_NULLS exactly for the two "outside" shapes (a frame whose last timestamp is null
    produces no row at all, whatever it holds)"""
    return bool(c.inclusive and c.tvalid[-1] and c.outside())


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_interpolate_null_interval_column(seed):
    """Inclusive cases: -13 exactly for the "outside" shapes; -9 only as "inclusive windows" (what inclusive Interpolate declines for
    ANY interval column), counted: at least 60 % of the inclusive cases drawn over the seeds run so far are compared with the oracle.
    Observed on an MI355X: over 32 seeds 420 inclusive cases drawn, 404 compared, 6 declined with -9 (1.4 %), 10 answered with
    -13; over 128 seeds 1687 drawn, 1628 compared, 25 declined (1.5 %), 34 answered with -13."""
    for c in ntc.interpolate_cases(seed):
        ccols, ocols = c.ccols(), c.ocols()
        kw = dict(offset=c.offset, inclusive=c.inclusive)
        _inclusive["drawn"] += c.inclusive
        forms = [("count + fill", lambda: both_interp_kernels(lambda: capi.rolling_interpolate(ccols, 0, c.interval, c.interps, **kw)))]
        if c.device:     # a fill without a count: nothing of a count's compaction to reuse (interp_null_ts.cpp NullTsState)
            forms.append(("one pass", lambda: capi.rolling_interpolate_onepass(ccols, 0, c.interval, c.interps, out_residency=capi.DEVICE, **kw)))
        want = None
        for form, run in forms:
            label = "%s %s" % (c.label, form)
            if expects_ts_nulls(c):
                with pytest.raises(capi.BowGpuError) as e:
                    run()
                assert e.value.code == -13, (label, e.value)
                _inclusive["outside"] += form == "count + fill"
                continue
            try:
                got = run()
            except capi.BowGpuError as e:
                assert c.inclusive and e.code == -9 and "inclusive windows" in e.message, (label, e)
                _inclusive["declined"] += form == "count + fill"
                continue
            if want is None:
                want = orc.interpolate(ocols, 0, c.interval, c.interps, **kw)
            for k in range(len(c.interps)):
                cmp_out("%s col %d" % (label, k), got[k], want[k])
            _inclusive["compared"] += c.inclusive and form == "count + fill"
    if seed == SEEDS[-1]:
        print("inclusive Interpolate cases:", _inclusive)
        assert _inclusive["compared"] >= 0.6 * _inclusive["drawn"], _inclusive


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_interpolate_then_aggregate_null_interval_column(seed):
    """bowgpu_rolling_interpolate_aggregate over an interval column with nulls - interp_null_ts makes an interpolated frame whose interval
    column has nulls, run_aggregate_null_ts reduces it - against oracle interpolate -> oracle aggregate, as one call and in the
    two-call form of the same entry point; the two forms decline alike."""
    for c in ntc.chain_cases(seed):
        ccols, ocols = c.ccols(), c.ocols()
        kw = dict(offset=c.offset, inclusive=c.inclusive)
        res = {}
        for form, mask in (("one call", 0), ("two-call form", capi.ROUTE_NO_FUSED)):
            with capi.route(mask):
                try:
                    res[form] = capi.rolling_interpolate_aggregate(ccols, 0, c.interval, c.interps, c.aggs, strict_order=True, **kw)
                except capi.BowGpuError as e:
                    res[form] = e
        errs = [r for r in res.values() if isinstance(r, capi.BowGpuError)]
        if expects_ts_nulls(c):
            assert len(errs) == 2 and errs[0].code == errs[1].code == -13, (c.label, res)
            continue
        if errs:
            # the interpolated interval column is not ascending (rows below the first window start), or what inclusive Interpolate declines
            assert len(errs) == 2 and errs[0].code == errs[1].code and errs[0].code in (-14, -9), (c.label, res)
            assert errs[0].code == -14 or (c.inclusive and "inclusive windows" in errs[0].message), (c.label, res)
            continue
        mid = orc.interpolate(ocols, 0, c.interval, c.interps, **kw)
        want, nic = orc.aggregate(mid, 0, c.interval, c.aggs, **kw)
        for form, (outs, info) in res.items():
            assert info.new_interval_col == nic and info.long_windows == 0, c.label
            for a, g, w in zip(c.aggs, outs, want):
                compare("%s %s %s" % (c.label, form, a[0]), g, w)


def test_null_interval_column_through_the_fan_out():
    """with a device list in force a call over an interval column with nulls is the one-device path's: the oracle's answer, one rank"""
    served = 0
    with capi.devices([0, 0], min_rows=100):
        for seed in range(4):
            for c in ntc.aggregate_cases(seed):
                if c.n < 2049 or c.tvalid.all():
                    continue
                ocols = c.ocols()
                kw = dict(offset=c.offset, inclusive=c.inclusive)
                exp, nic = orc.aggregate(ocols, 0, c.interval, c.aggs, **kw)
                outs, info = capi.rolling_aggregate(c.ccols(), 0, c.interval, c.aggs, **kw)
                assert capi.last_call_ranks() == 1, c.label
                against_the_oracle(c.label + " fan-out", c.aggs, outs, info, exp, nic,
                                   lambda: order_free_bounds(ocols, 0, c.interval, c.aggs, ref=exp, **kw))
                served += 1
    assert capi.get_devices() == [] and served >= 12, served


def test_null_run_across_a_tile_of_the_neighbour_index():
    """4 204 304 dense rows, device-resident, the interval column 37 rows into its buffers: a null run of 6000 rows lies across bit
    4 194 304 of the bitmap - the edge between two 1024-block tiles of the neighbour index, in the bitmap's own bit numbering
    (nbr_tile_kernel / nbr_scan_kernel: the carries from the tiles before and after) - with 2 % nulls everywhere else.  The one shape
    the seeded sizes cannot reach."""
    rng = np.random.default_rng(4194304)
    pad, n = 37, 4_194_304 + 10_000
    edge = 4_194_304 - pad
    tvalid = rng.random(n) >= 0.02
    tvalid[edge - 3000:edge + 3000] = False
    tvalid[0] = tvalid[-1] = True
    ts = np.arange(n, dtype=np.int64) + 5
    ts[~tvalid] = rng.integers(-2 ** 62, 2 ** 62, int((~tvalid).sum()))
    ts_buf = np.concatenate([rng.integers(-9, 9, pad), ts, rng.integers(-9, 9, 5)]).astype(np.int64)
    tbits = rng.random(pad + n + 5) < 0.5
    tbits[pad:pad + n] = tvalid
    tbm = np.packbits(tbits, bitorder="little")
    vals = np.round(rng.standard_normal(pad + n + 5) * 100, 3)
    vbm = np.packbits(rng.random(pad + n + 5) >= 0.1, bitorder="little")
    ccols = [capi.Column(ts_buf, tbm, capi.INT64, pad, n, -1).to_device(), capi.Column(vals, vbm, capi.FLOAT64, pad, n, -1).to_device()]
    ocols = [orc.Column(ts_buf, tbm, orc.INT64, offset=pad, length=n), orc.Column(vals, vbm, orc.FLOAT64, offset=pad, length=n)]
    want, nic = orc.aggregate(ocols, 0, 8, NULL_TS_AGGS_INCL, offset=3)
    got, info = capi.rolling_aggregate(ccols, 0, 8, NULL_TS_AGGS_INCL, offset=3, out_residency=capi.DEVICE)
    against_the_oracle("across a tile of the neighbour index", NULL_TS_AGGS_INCL, got, info, want, nic,
                       lambda: order_free_bounds(ocols, 0, 8, NULL_TS_AGGS_INCL, offset=3, ref=want))
    # the windows either side of the run: [.., run) ends at the last valid row in front of it, the next one with rows starts behind it
    lo, hi = (edge - 3000 + 5 - want[0].values[0]) // 8, (edge + 3000 + 5 - want[0].values[0]) // 8
    k = [a[0] for a in NULL_TS_AGGS_INCL].index("NumRows")
    rows = want[k].values[:want[k].length]
    assert not rows[lo + 1:hi].any() and rows[lo - 2:lo].all() and rows[hi + 1:hi + 3].all()
