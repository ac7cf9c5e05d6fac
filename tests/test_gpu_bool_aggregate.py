"""Rolling.Aggregate over Boolean value columns on the device (rolling_bool.hip) against the reference's golden vectors and
the oracle.  Every comparison is exact: value bits, validity bytes, padding bits, null_count, type and length."""
import os

import numpy as np
import pytest

from bow_amd import capi
from oracle import pyoracle as orc
from bool_agg_common import BOOL_RESULT, TIME_AGGS, VALUE_AGGS, bool_cols, compare_exact, pack
from staging_common import Shifted

pytestmark = pytest.mark.gpu

T = {"float64": capi.FLOAT64, "int64": capi.INT64, "bool": capi.BOOLEAN}
ALL_VALUE = [("WindowStart", 0)] + [(k, 1) for k in VALUE_AGGS] + [("NumRows", 1)]
LANE = capi.BOOL_LANE_ROWS


def same_list(a, b):
    assert len(a) == len(b), (a, b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or (x == y and type(x) is type(y))), (a, b)


def check_call(label, ccols, ocols, interval, aggs, offset=0, inclusive=False, residency=capi.HOST, outs=None, strict_order=False):
    exp, nic = orc.aggregate(ocols, 0, interval, aggs, offset=offset, inclusive=inclusive)
    outs, info = capi.rolling_aggregate(ccols, 0, interval, aggs, offset=offset, inclusive=inclusive, out_residency=residency, outs=outs,
                                        strict_order=strict_order)
    assert info.new_interval_col == nic, label
    for a, g, w in zip(aggs, outs, exp):
        compare_exact("%s %s" % (label, a[0]), g, w)
    return outs, info, exp


def frame_of_windows(lens, interval=10):
    """timestamps of a frame whose window k holds lens[k] rows (0: an empty window); the last window must hold a row"""
    assert lens[-1] > 0 and lens[0] > 0
    return np.concatenate([np.full(m, k * interval + (k % 3), np.int64) for k, m in enumerate(lens)])


# ------------------------------------------------------------------ 4. the reference's own vectors
def test_golden_sparse_bool(golden):
    seen = []
    for v in golden["reducers"]:
        b = golden["bows"][v["bow"]]
        if b["value_type"] != "bool":
            continue
        cols = [capi.Column.from_list(b["time"], "int64"), capi.Column.from_list(b["value"], "bool")]
        outs, info = capi.rolling_aggregate(cols, 0, v["interval"], [("WindowStart", 0), (v["reducer"], 1, v["factors"])], offset=v["offset"])
        assert outs[0].type == capi.INT64
        same_list(outs[0].to_list(), v["expect_time"])
        assert outs[1].type == T[v["expect_type"]], (v["reducer"], v["name"])
        same_list(outs[1].to_list(), v["expect_value"])
        seen.append(v["reducer"])
    assert sorted(seen) == sorted(["Sum", "ArithmeticMean", "Min", "Max", "First", "Last", "Mode"] + TIME_AGGS), seen


# ------------------------------------------------------------------ 5. shapes at which a bit-range kernel goes wrong
# windows inside one 32-bit word, across one word boundary, across several; 64 rows on a 64-bit boundary (rows 128 .. 191); one row
# below, at and above the class boundary; a run of more than 64 empty windows (a whole wavefront without a valid row, twice over)
SHAPE_LENS = [5, 20, 10, 70, 23, 64, 1, LANE - 1, LANE, LANE + 1, 2, 33] + [0] * 150 + [3, 31, 32, 1]


@pytest.mark.parametrize("arrow_offset", [0, 3, 13])
@pytest.mark.parametrize("nulls", ["no buffer", "some", "most", "all"])
@pytest.mark.parametrize("device", [False, True])
def test_shapes(arrow_offset, nulls, device):
    assert sum(SHAPE_LENS[:5]) == 128
    rng = np.random.default_rng(arrow_offset * 10 + len(nulls))
    ts = frame_of_windows(SHAPE_LENS)
    n = len(ts)
    vals = rng.random(n) < 0.5
    valid = {"no buffer": None, "some": rng.random(n) >= 0.3, "most": rng.random(n) >= 0.9, "all": np.zeros(n, bool)}[nulls]
    ccols, ocols = bool_cols(ts, vals, valid, offset=arrow_offset)
    if device:
        ccols = [c.to_device() for c in ccols]
    outs, info, exp = check_call("shapes off=%d %s" % (arrow_offset, nulls), ccols, ocols, 10, ALL_VALUE,
                                 residency=capi.DEVICE if device else capi.HOST)
    assert outs[0].length == len(SHAPE_LENS)
    if nulls == "all":
        assert all(o.null_count == o.length for a, o in zip(ALL_VALUE, outs) if a[0] in ("ArithmeticMean", "Min", "Max", "First", "Last", "Mode"))


def test_known_null_count_and_counted_one_agree():
    rng = np.random.default_rng(5)
    ts = frame_of_windows([7, 40, 0, 0, 9, 300, 1])
    vals, valid = rng.random(len(ts)) < 0.5, rng.random(len(ts)) >= 0.4
    res = []
    for nc in (-1, int((~valid).sum())):
        ccols, ocols = bool_cols(ts, vals, valid, offset=3, null_count=nc)
        outs, _, _ = check_call("null_count=%d" % nc, ccols, ocols, 10, ALL_VALUE)
        res.append([tuple(np.asarray(x).tobytes() for x in o.host_arrays()) for o in outs])
    assert res[0] == res[1]


def test_one_window_of_20000_rows():
    rng = np.random.default_rng(6)
    n = 20_000
    ts = np.sort(rng.integers(0, 1000, n)).astype(np.int64)
    for valid in (None, rng.random(n) >= 0.5, np.arange(n) == 12_345):
        ccols, ocols = bool_cols(ts, rng.random(n) < 0.5, valid, offset=13)
        outs, info, _ = check_call("one window", ccols, ocols, 1000, ALL_VALUE)
        assert outs[0].length == 1


@pytest.mark.parametrize("shift", [1, 3, 6])
def test_device_pointers_at_odd_byte_addresses(shift):
    rng = np.random.default_rng(7 + shift)
    ts = frame_of_windows([3, 50, 0, LANE + 7, 64, 9])
    n = len(ts)
    vals, valid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    ccols, ocols = bool_cols(ts, vals, valid, offset=5)
    lead = np.full(shift, 0xFF, np.uint8)
    dv = capi.DeviceBuffer.from_numpy(np.concatenate([lead, ccols[1].values, np.full(8, 0xFF, np.uint8)]))
    db = capi.DeviceBuffer.from_numpy(np.concatenate([lead, lead, ccols[1].validity, np.full(8, 0xFF, np.uint8)]))
    dcol = capi.Column(Shifted(dv, shift), Shifted(db, 2 * shift), capi.BOOLEAN, 5, n, -1)
    check_call("odd addresses", [ccols[0].to_device(), dcol], ocols, 10, ALL_VALUE + [("WeightedAverageStep", 1)], residency=capi.DEVICE)


def guarded_outs(W, count, residency):
    """output columns of exactly W slots with poisoned bytes behind them"""
    outs = []
    for _ in range(count):
        o = capi.OutColumn(W, capi.HOST)
        o.residency = residency
        nb = (W + 7) // 8
        if residency == capi.DEVICE:
            o.values = capi.DeviceBuffer.from_numpy(np.full(W * 8 + 64, 0x5A, np.uint8))
            o.validity = capi.DeviceBuffer.from_numpy(np.full(nb + 64, 0xA5, np.uint8))
        elif residency == capi.HOST_PINNED:   # (registered here, unregistered when the OutColumn goes)
            o.values = capi.page_aligned(W + 8, np.uint64, 0x5A5A5A5A5A5A5A5A)
            o.validity = capi.page_aligned(nb + 64, np.uint8, 0xA5)
            capi.host_register(o.values)
            capi.host_register(o.validity)
        else:
            o.values = np.full(W + 8, 0x5A5A5A5A5A5A5A5A, np.uint64)
            o.validity = np.full(nb + 64, 0xA5, np.uint8)
        outs.append(o)
    return outs


def check_guards(label, W, outs):
    nb = (W + 7) // 8
    for i, o in enumerate(outs):
        used = nb if o.type == capi.BOOLEAN else W * 8
        if o.residency == capi.DEVICE:
            v, b = o.values.to_numpy(np.uint8, o.values.nbytes), o.validity.to_numpy(np.uint8, o.validity.nbytes)
        else:
            v, b = o.values.view(np.uint8), o.validity
        assert (v[used:] == 0x5A).all(), (label, i, "values written past byte %d" % used, np.flatnonzero(v[used:] != 0x5A)[:5])
        assert (b[nb:] == 0xA5).all(), (label, i, "validity written past byte %d" % nb)


@pytest.mark.parametrize("W", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1000])
@pytest.mark.parametrize("residency", [capi.HOST, capi.DEVICE, capi.HOST_PINNED])
def test_nothing_past_the_last_byte(W, residency):
    rng = np.random.default_rng(W)
    lens = [int(x) for x in rng.integers(0, 6, W)]
    lens[0] = lens[-1] = 2
    ts = frame_of_windows(lens)
    ccols, ocols = bool_cols(ts, rng.random(len(ts)) < 0.5, rng.random(len(ts)) >= 0.3, offset=3)
    if residency == capi.DEVICE:
        ccols = [c.to_device() for c in ccols]
    outs = guarded_outs(W, len(ALL_VALUE), residency)
    check_call("W=%d" % W, ccols, ocols, 10, ALL_VALUE, residency=residency, outs=outs)
    assert outs[0].length == W
    check_guards("W=%d" % W, W, outs)


@pytest.mark.parametrize("inclusive", [False, True])
def test_rows_below_the_first_window_start(inclusive):
    # Go's truncating division: first ts -7, interval 5, offset 4 -> s0 = -6 above the first rows, which ride in window 0
    cases = [([-7, -7, -6, -5, -1, 0, 3, 4, 9], 5, 4),
             ([-37, -36, -35, -20, -5, 3], 10, -4),          # window 0 = only rows below s0: empty
             ([-7, -7, -1, 3, 3, 8], 5, 4),                  # the next window's first row sits on its start: an inclusive call keeps window 0
             ([-15, -12, 1000], 10, 9)]
    rng = np.random.default_rng(11)
    for ts, interval, offset in cases:
        ts = np.asarray(ts, np.int64)
        for valid in (None, rng.random(len(ts)) >= 0.3):
            ccols, ocols = bool_cols(ts, rng.random(len(ts)) < 0.5, valid)
            aggs = ALL_VALUE + ([("IntegralTrapezoid", 1)] if inclusive else [])
            check_call("below s0 %s incl=%d" % (list(ts), inclusive), ccols, ocols, interval, aggs, offset=offset, inclusive=inclusive)


def test_mode_ties_both_ways_round():
    ts = np.asarray([0, 1, 10, 11, 20, 21, 22, 23, 30, 31, 32], np.int64)
    vals = [True, False, False, True, True, False, False, True, True, False, True]
    valid = [True, True, True, True, True, True, True, True, True, True, False]
    ccols, ocols = bool_cols(ts, vals, valid)
    outs, _, _ = check_call("ties", ccols, ocols, 10, [("WindowStart", 0), ("Mode", 1), ("Last", 1)])
    assert outs[1].to_list() == [True, False, False, True]     # a tie goes to the value the last valid row does not have
    assert outs[2].to_list() == [False, True, True, False]


# ------------------------------------------------------------------ 6. residencies
@pytest.mark.parametrize("inputs", ["host", "pinned", "device"])
@pytest.mark.parametrize("outputs", [capi.HOST, capi.HOST_PINNED, capi.DEVICE])
def test_residencies(inputs, outputs):
    rng = np.random.default_rng(12)
    n = 3000
    ts = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    ccols, ocols = bool_cols(ts, rng.random(n) < 0.5, rng.random(n) >= 0.3, offset=13)
    aggs = ALL_VALUE + [("WeightedAverageStep", 1)]
    if inputs == "device":
        ccols = [c.to_device() for c in ccols]
    elif inputs == "pinned":
        pinned = []
        for c in ccols:
            v = capi.page_aligned(c.values.size, c.values.dtype)
            v[:] = c.values
            b = None
            if c.validity is not None:
                b = capi.page_aligned(c.validity.size, np.uint8)
                b[:] = c.validity
            pinned.append(capi.Column(v, b, c.type, c.offset, c.length, c.null_count).pin())
        ccols = pinned
    try:
        check_call("%s -> %d" % (inputs, outputs), ccols, ocols, 25, aggs, residency=outputs)
    finally:
        if inputs == "pinned":
            for c in ccols:
                c.unpin()


# ------------------------------------------------------------------ 7. one call with everything in it
def test_mixed_call_more_than_sixteen_outputs():
    rng = np.random.default_rng(13)
    n = 2500
    ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)           # ~10 rows per window of 10
    f = rng.standard_normal(n) * 100
    fvalid = rng.random(n) >= 0.2
    ints = rng.integers(-3, 4, n).astype(np.int64)
    bvals, bvalid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    bc, bo = bool_cols(ts, bvals, bvalid, offset=3)
    ccols = [bc[0], capi.Column(f, np.packbits(fvalid, bitorder="little"), capi.FLOAT64, 0, n, -1), bc[1], capi.Column(ints, None, capi.INT64)]
    ocols = [bo[0], orc.Column(f, np.packbits(fvalid, bitorder="little"), orc.FLOAT64), bo[1], orc.Column(ints, None, orc.INT64)]
    aggs = ([("WindowStart", 0)] + [(k, 1) for k in ("Sum", "ArithmeticMean", "Min", "Max", "Count", "First", "Last")]
            + [(k, 2) for k in VALUE_AGGS] + [("Mode", 3), ("IntegralTrapezoid", 1), ("WeightedAverageStep", 2), ("WeightedAverageLinear", 2),
                                             ("NumRows", 2), ("Sum", 2, [2.0, -0.5]), ("Count", 2, [3.0])])
    assert len(aggs) > 16
    ccols = [c.to_device() for c in ccols]
    runs = []
    for _ in range(2):
        outs, info, _ = check_call("mixed", ccols, ocols, 10, aggs, inclusive=True, residency=capi.DEVICE)
        assert info.inclusive == 1 and info.long_windows == 0
        runs.append([tuple(np.asarray(x).tobytes() for x in o.host_arrays()) for o in outs])
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ 8. the time-weighted reducers (through the widening)
def test_time_weighted_over_boolean():
    rng = np.random.default_rng(14)
    n = 4000
    ts = np.cumsum(rng.integers(0, 5, n)).astype(np.int64)
    for valid in (None, rng.random(n) >= 0.3):
        for off in (0, 13):
            ccols, ocols = bool_cols(ts, rng.random(n) < 0.5, valid, offset=off)
            aggs = [("WindowStart", 0)] + [(k, 1) for k in TIME_AGGS] + [("IntegralStep", 1, [0.5])]
            outs, info, _ = check_call("time-weighted", ccols, ocols, 20, aggs)
            assert info.long_windows == 0 and info.inclusive == 1
            outs, info, _ = check_call("time-weighted device", [c.to_device() for c in ccols], ocols, 20, aggs, residency=capi.DEVICE)
            assert info.long_windows == 0


def test_time_weighted_long_window_strict_order():
    rng = np.random.default_rng(15)
    n = 9000
    ts = np.sort(rng.integers(0, 3000, n)).astype(np.int64)         # three windows of ~3000 rows
    ccols, ocols = bool_cols(ts, rng.random(n) < 0.5, rng.random(n) >= 0.3, offset=3)
    aggs = [("WindowStart", 0)] + [(k, 1) for k in TIME_AGGS] + [(k, 1) for k in VALUE_AGGS]
    outs, info, _ = check_call("long, strict", ccols, ocols, 1000, aggs, strict_order=True)
    assert info.long_windows == 0 and outs[0].length == 3


# ------------------------------------------------------------------ 9. fuzz
FUZZ_CASES = 12


def fuzz_case(rng):
    n = int(rng.integers(0, 5001)) if rng.random() < 0.8 else int(rng.integers(0, 70))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        ts = np.arange(n)
    elif kind == 1:
        ts = np.cumsum(rng.integers(0, 4, n))
    elif kind == 2:
        step = rng.integers(0, 3, n)
        step[rng.random(n) < 0.01] = rng.integers(50, 5000)        # runs of empty windows
        ts = np.cumsum(step)
    else:
        ts = np.cumsum(rng.integers(0, 3, n)) - int(rng.integers(0, 2 * n + 2))   # negative timestamps: rows below the first window start
    ts = ts.astype(np.int64)
    span = int(ts[-1] - ts[0]) + 1 if n else 1
    # windows from one row to all rows: the interval from 1 up to the whole span
    interval = max(1, int(span ** rng.random()) if rng.random() < 0.8 else span + int(rng.integers(0, 5)))
    while n and span // interval > 200_000:
        interval *= 10
    offset = int(rng.integers(-2 * interval, 2 * interval + 1))
    density = [0.0, 0.05, 0.3, 0.9, 1.0][int(rng.integers(0, 5))]
    valid = None if density == 0.0 and rng.random() < 0.5 else rng.random(n) >= density
    vals = rng.random(n) < [0.5, 0.1, 0.9][int(rng.integers(0, 3))]
    return ts, vals, valid, interval, offset, int(rng.integers(0, 70)) if rng.random() < 0.5 else 0


@pytest.mark.parametrize("seed", range(int(os.environ.get("BOW_FUZZ_SEEDS", "64"))))
def test_fuzz(seed):
    rng = np.random.default_rng(9000 + seed)
    ran = 0
    for case in range(FUZZ_CASES):
        ts, vals, valid, interval, offset, arrow_offset = fuzz_case(rng)
        ccols, ocols = bool_cols(ts, vals, valid, offset=arrow_offset)
        device = rng.random() < 0.4
        if device:
            ccols = [c.to_device() for c in ccols]
        label = "seed=%d case=%d n=%d I=%d off=%d arrow=%d" % (seed, case, len(ts), interval, offset, arrow_offset)
        if len(ts) == 0:
            outs, info = capi.rolling_aggregate(ccols, 0, interval, ALL_VALUE, offset=offset)
            assert all(o.length == 0 for o in outs), label
            assert [o.type for o in outs] == [capi.INT64, capi.FLOAT64, capi.FLOAT64, capi.FLOAT64, capi.FLOAT64, capi.INT64, capi.BOOLEAN,
                                              capi.BOOLEAN, capi.BOOLEAN, capi.FLOAT64], label
        else:
            check_call(label, ccols, ocols, interval, ALL_VALUE, offset=offset, residency=capi.DEVICE if device else capi.HOST)
        ran += 1
    assert ran == FUZZ_CASES


# ------------------------------------------------------------------ 10. what stays declined
def test_null_timestamps_with_a_boolean_aggregation():
    ts = capi.Column.from_list([0, 1, None, 12, 13, 25], "int64")
    b = capi.Column.from_list([True, False, True, None, True, False], "bool")
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate([ts, b], 0, 10, [("WindowStart", 0), ("Count", 1)])
    assert e.value.code == -13 and "Boolean" in e.value.message, e.value.message
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate([ts, b], 0, 10, [("WindowStart", 0), ("WeightedAverageStep", 1)])
    assert e.value.code == -13, e.value.message


def test_device_list_serves_a_boolean_call_on_one_device():
    rng = np.random.default_rng(16)
    n = 6000
    ts = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    ccols, ocols = bool_cols(ts, rng.random(n) < 0.5, rng.random(n) >= 0.3, offset=3)
    fcol = capi.Column(rng.standard_normal(n), None, capi.FLOAT64)
    aggs = ALL_VALUE + [("WeightedAverageStep", 1)]
    one, _ = capi.rolling_aggregate(ccols, 0, 10, aggs)
    before = capi.get_devices()
    try:
        with capi.devices([0, 0], min_rows=1000):
            capi.rolling_aggregate([ccols[0], fcol], 0, 10, [("WindowStart", 0), ("Sum", 1)])
            assert capi.last_call_ranks() == 2            # (the list is in force: a call without a Boolean column is cut in two)
            outs, _, _ = check_call("device list", ccols, ocols, 10, aggs)
            assert capi.last_call_ranks() == 1
            capi.rolling_aggregate(ccols + [fcol], 0, 10, [("WindowStart", 0), ("Sum", 2), ("NumRows", 1)])
            assert capi.last_call_ranks() == 1            # any aggregation that names a Boolean column keeps the call whole
    finally:
        capi.set_devices(before)
    assert capi.get_devices() == before
    for a, b in zip(one, outs):
        assert [np.asarray(x).tobytes() for x in a.host_arrays()] == [np.asarray(x).tobytes() for x in b.host_arrays()]


def test_sharded_call_declines_a_boolean_column():
    ts = np.arange(100, dtype=np.int64)
    ccols, _ = bool_cols(ts, ts % 3 == 0, None)
    dcols = [c.to_device() for c in ccols]
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate_sharded([dcols, dcols], 0, 10, [("WindowStart", 0), ("Count", 1)], [0, 0])
    assert e.value.code == -9 and "Boolean" in e.value.message, e.value.message
