"""Rolling.Aggregate over Boolean value columns, the part that needs no device: the closed forms bool_windows_kernel computes
(counts of valid and of valid-true rows, first and last valid bit) against the oracle, that validation lets such a call
through to the device, and what stays declined."""
import re
import os

import numpy as np
import pytest

from bow_amd import capi
from oracle import pyoracle as orc
from bool_agg_common import VALUE_AGGS, bool_cols, closed_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_frame(rng, density):
    n = int(rng.integers(1, 70))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        ts = np.cumsum(rng.integers(0, 4, n))
    elif kind == 1:
        ts = np.cumsum(rng.integers(1, 30, n))
    elif kind == 2:
        ts = np.cumsum(rng.integers(0, 3, n)) - int(rng.integers(1, 3 * n + 2))   # negative timestamps: rows below the first window start
    else:
        ts = np.sort(rng.integers(-40, 40, n))
    ts = ts.astype(np.int64)
    if rng.random() < 0.5:
        vals = rng.random(n) < 0.5
    else:
        vals = (np.arange(n) + int(rng.integers(0, 2))) % 2 == 0     # alternating: Mode ties in every even window
    valid = rng.random(n) >= density
    interval = int([1, 2, 4, 7, 10, 50, 1000][int(rng.integers(0, 7))])
    offset = int(rng.integers(-2 * interval, 2 * interval + 1))
    return ts, vals, valid, interval, offset


def test_closed_forms_against_the_oracle():
    rng = np.random.default_rng(20251)
    frames = windows = ties = below = 0
    for case in range(400):
        density = [0.0, 0.3, 0.9, 1.0][case % 4]
        ts, vals, valid, interval, offset = small_frame(rng, density)
        _, ocols = bool_cols(ts, vals, valid if density > 0.0 or case % 8 < 4 else None, offset=int(rng.integers(0, 14)))
        if ocols[1].validity is None:
            valid = np.ones(len(ts), bool)
        aggs = [("WindowStart", 0)] + [(k, 1) for k in VALUE_AGGS]
        exp, _ = orc.aggregate(ocols, 0, interval, aggs, offset=offset)
        wins = orc.iterate_windows(ocols[0], interval, offset, False)
        s0, W = orc.plan_windows(ocols[0], interval, offset)
        assert W == len(wins)
        rows = [(w["slice_begin"], w["slice_end"]) for w in wins]
        below += int(len(ts) > 0 and ts[0] < s0)
        want = closed_forms(rows, vals, valid)
        for k, col in zip(VALUE_AGGS, exp[1:]):
            assert col.type == (orc.BOOLEAN if k in ("First", "Last", "Mode") else orc.INT64 if k == "Count" else orc.FLOAT64), k
            assert col.to_list() == want[k], (case, k, col.to_list(), want[k])
        for a, b in rows:
            v = valid[a:b]
            ties += int(v.any() and 2 * int((vals[a:b] & v).sum()) == int(v.sum()))
        frames += 1
        windows += W
    assert frames == 400 and windows > 5000 and ties > 300 and below > 20, (frames, windows, ties, below)


def test_boolean_aggregation_reaches_the_device():
    """host-resident columns: validation passes and the call goes on to the device - BOWGPU_ERR_NO_DEVICE where there is none"""
    ccols, ocols = bool_cols([10, 11, 20, 40, 41], [True, False, True, True, False], [True, True, False, True, True])
    aggs = [("WindowStart", 0), ("Count", 1), ("Sum", 1), ("First", 1)]
    try:
        outs, info = capi.rolling_aggregate(ccols, 0, 10, aggs)
    except capi.BowGpuError as e:
        assert e.code == -11, (e.code, e.message)
        return
    exp, _ = orc.aggregate(ocols, 0, 10, aggs)
    assert [o.type for o in outs] == [capi.INT64, capi.INT64, capi.FLOAT64, capi.BOOLEAN]
    for o, w in zip(outs, exp):
        assert o.to_list() == w.to_list()


def test_declines():
    ccols, _ = bool_cols([10, 11, 20], [True, False, True], None)
    for kind in ("First", "Last", "Mode"):
        with pytest.raises(capi.BowGpuError) as e:
            capi.rolling_aggregate(ccols, 0, 10, [("WindowStart", 0), (kind, 1, [2.0])])
        assert e.value.code == -9 and "factor: invalid type bool" in e.value.message, (kind, e.value.message)
    # a Factor on a Float64 / Int64 result over the same column is served: validation lets it through
    try:
        capi.rolling_aggregate(ccols, 0, 10, [("WindowStart", 0), ("Sum", 1, [2.0]), ("Count", 1, [3.0])])
    except capi.BowGpuError as e:
        assert e.code == -11, (e.code, e.message)
    scols = [ccols[0], capi.Column(np.zeros(8, np.uint8), None, capi.STRING, 0, 3, 0)]
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate(scols, 0, 10, [("WindowStart", 0), ("Count", 1)])
    assert e.value.code == -9 and "String" in e.value.message, e.value.message
    # the sharded call: declined by its validation, before a device is looked for
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout([ccols, ccols], 0, 10, [("WindowStart", 0), ("Count", 1)], [0, 0])
    assert e.value.code == -9 and "Boolean" in e.value.message, e.value.message
    # Interpolate + Aggregate keeps declining a Boolean column
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_interpolate_aggregate(ccols, 0, 10, [{"kind": "WindowStart", "col": 0}], [("WindowStart", 0), ("Count", 1)])
    assert e.value.code in (-7, -9), (e.value.code, e.value.message)


def test_class_boundary_constant_is_the_kernels():
    """capi.BOOL_LANE_ROWS (what the GPU tests place their window lengths around) is common.h's kBoolLaneRows"""
    with open(os.path.join(ROOT, "bow_amd", "csrc", "common.h")) as f:
        m = re.search(r"constexpr int kBoolLaneRows = (\d+);", f.read())
    assert m and int(m.group(1)) == capi.BOOL_LANE_ROWS
