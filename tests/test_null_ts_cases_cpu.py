"""tests/null_ts_cases.py checked without a GPU: the oracle carries every case the generator draws, and the first 16 seeds hold what
tests/test_gpu_null_ts_fuzz.py is there to exercise - so that test cannot turn green by drawing nothing of interest or by skipping
the shapes inclusive Interpolate declines."""
import numpy as np
import pytest

import null_ts_cases as ntc
from oracle import pyoracle as orc

SEEDS = range(16)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_oracle_carries_every_aggregate_case_and_a_seed_holds_every_shape(seed):
    seen = set()
    a5 = 0
    for c in ntc.aggregate_cases(seed):
        ocols = c.ocols()
        want, _nic = orc.aggregate(ocols, 0, c.interval, c.aggs, offset=c.offset, inclusive=c.inclusive_call)     # (no OracleError)
        _s0, W = c.plan()
        assert all(w.length == W for w in want), c.label
        assert c.tvalid[0] and len(c.tvalid) == c.n == ocols[0].length
        assert np.array_equal(ocols[0].valid_mask(), c.tvalid), c.label
        if c.pad % 8:
            seen.add("an interval column at pad % 8 != 0")
        if ntc.longest_null_run(c.tvalid) > 2048:
            seen.add("a null run longer than 2048 rows")
        if c.n > 1 and not c.tvalid[-1]:
            seen.add("a null last row")
            assert not any(w.valid_mask().any() for w in want), c.label      # (the all-nil output path)
        if any(typ == orc.INT64 for _v, _bm, typ, _off in c.raw):
            seen.add("an Int64 value column")
        if any(bm is None for _v, bm, _typ, _off in c.raw):
            seen.add("a value column without validity")
        if c.ns:
            seen.add("a nanosecond-scale frame")
        if len(c.aggs) > ntc.MAX_AGGS_PER_LAUNCH:
            seen.add("a batch-splitting reducer list")
        if c.inclusive_call and c.tvalid[-1]:         # (behind a null last row every slot is nil)
            a5 += c.a5_rows()
    missing = {"an interval column at pad % 8 != 0", "a null run longer than 2048 rows", "a null last row", "an Int64 value column",
               "a value column without validity", "a nanosecond-scale frame", "a batch-splitting reducer list"} - seen
    assert not missing, (seed, missing)
    assert a5 >= 50, (seed, a5)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_oracle_carries_every_interpolate_case(seed):
    a5 = 0
    for c in ntc.interpolate_cases(seed):
        got = orc.interpolate(c.ocols(), 0, c.interval, c.interps, offset=c.offset, inclusive=c.inclusive)        # (no OracleError)
        assert len(got) == len(c.interps), c.label
        if c.inclusive:
            s0, _W = c.plan()
            assert c.ts[0] >= 0 and 0 <= c.offset < c.interval and 0 <= s0 <= c.ts[0], c.label      # the documented domain
            assert int(c.ts[c.tvalid].max()) < 2 ** 24, c.label
            a5 += c.a5_rows()
    assert a5 >= 50, (seed, a5)
    for c in ntc.chain_cases(seed):
        mid = orc.interpolate(c.ocols(), 0, c.interval, c.interps, offset=c.offset, inclusive=c.inclusive)
        assert mid[0].length >= 0 and len(c.aggs) >= 2, c.label


def test_few_inclusive_interpolate_cases_hold_a_shape_the_device_path_declines():
    """at most 15 % of the inclusive Interpolate cases of the 16 seeds are answered with BOWGPU_ERR_TS_NULLS instead of being compared"""
    cs = [c for seed in SEEDS for c in ntc.interpolate_cases(seed) if c.inclusive]
    n_incl, n_out = len(cs), sum(c.outside() for c in cs)
    assert n_incl >= 100, n_incl
    assert n_out <= 0.15 * n_incl, (n_out, n_incl)


def test_the_predicates_on_a_frame_made_by_hand():
    #              0   1   2   3   4   5   6   7   8   9
    ts = np.array([10, 11, 20, 99, 21, 30, 77, 30, 40, 41], dtype=np.int64)
    tv = np.array([1, 1, 1, 0, 1, 1, 0, 1, 1, 1], bool)
    # row 2 sits on the start of window 1 with a null behind it; row 5 too (window 2) - and is followed by an equal timestamp
    assert list(np.flatnonzero(ntc.rows_on_a_start_with_a_null_behind(ts, tv, 10, 10))) == [2, 5]
    assert ntc.outside_inclusive_interpolate(ts, tv, 10, 10)
    assert not ntc.outside_inclusive_interpolate(ts[:5], tv[:5], 10, 10)
    assert list(np.flatnonzero(ntc.rows_on_a_start_with_a_null_behind(ts, tv, 10, 5))) == [2, 5]
    assert not ntc.rows_on_a_start_with_a_null_behind(ts, tv, 11, 10).any()
    # window 0's start does not count, nor does a second row with the same timestamp
    ts = np.array([10, 10, 20, 20, 5, 30], dtype=np.int64)
    tv = np.array([1, 1, 1, 1, 0, 1], bool)
    assert not ntc.rows_on_a_start_with_a_null_behind(ts, tv, 10, 10).any()
    # a row on -1
    ts = np.array([-11, -1, 0, 3], dtype=np.int64)
    tv = np.array([1, 1, 0, 1], bool)
    assert ntc.rows_on_a_start_with_a_null_behind(ts, tv, -11, 10)[1] and ntc.outside_inclusive_interpolate(ts, tv, -11, 10)
    assert ntc.longest_null_run(np.array([1, 0, 0, 1, 0, 0, 0, 1, 0], bool)) == 3 and ntc.longest_null_run(np.ones(4, bool)) == 0
