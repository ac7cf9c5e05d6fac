"""Bow.DropNils / Bow.Diff / Bow.Distinct on the device (bowgpu_valid_mask / bowgpu_drop_nils / bowgpu_diff / bowgpu_distinct) against
numpy, which is exact for all of this, and against the fixture of the reference's own tests: every comparison is bit for bit - values,
validity bytes, null_count, zeroed null slots, clear padding bits, and the sentinels of the output buffers intact past the rows
produced (or everywhere, when a call says contiguous or returns an error).  The one exception: Diff results that are NaN are compared
as NaN at the same rows (the sign of a NaN the subtraction generates is the device's: include/bowgpu.h)."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from bow_amd import capi
from test_gpu_filter import (DEVICE, GROUP, HOST, I64_MAX, I64_MIN, N_SCAN, PINNED, POISON, T, Col, assert_result, assert_untouched,
                             make_outs, pack, place, raw, release)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNTS = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
OFFSETS = [0, 1, 7, 63, 64, 65]
MASK_COLS = 8                 # bitmaps ANDed per launch of valid_mask_kernel (bow_amd/csrc/common.h kValidMaskCols)
ERR_UNSUPPORTED, ERR_ARG = -9, -10


# ------------------------------------------------------------------ oracles (numpy: exact)
def valid_of(col):
    return np.ones(len(col.values), bool) if col.valid is None else col.valid


def keep_rows(frame, idx=None, and_bits=None):
    sel = sorted(set(idx)) if idx else range(len(frame))
    keep = np.ones(len(frame[0].values), bool)
    for i in sel:
        keep &= valid_of(frame[i])
    return keep if and_bits is None else keep & and_bits


def diff_want(col):
    """(payloads with 0 in the null slots, validity) of Bow.Diff of one column"""
    n, v = len(col.values), valid_of(col)
    ok = np.zeros(n, bool)
    ok[1:] = v[1:] & v[:-1]
    d = np.zeros(n, np.uint64)
    if n > 1:
        if col.values.dtype == np.int64:
            d[1:] = col.bits()[1:] - col.bits()[:-1]              # wraps, as Go's int64 does
        else:
            with np.errstate(all="ignore"):
                d[1:] = (col.values[1:] - col.values[:-1]).view(np.uint64)   # one IEEE subtraction
    return np.where(ok, d, np.uint64(0)), ok


def distinct_want(col):
    """payloads of Bow.Distinct: the valid values, each once, ascending; the zero that survives is the LAST one in row order"""
    vals = col.values[valid_of(col)]
    u = np.unique(vals)
    bits = u.view(np.uint64).copy()
    zeros = vals[vals == 0]
    if len(zeros):
        bits[u == 0] = zeros[-1:].view(np.uint64)
    return bits


def assert_diff(col, o, cap):
    n = len(col.values)
    want, ok = diff_want(col)
    v, b = raw(o, cap)
    nb = (n + 7) // 8
    assert o.length == n and o.type == col.typ and o.null_count == n - int(ok.sum())
    got = v[:n]
    if col.values.dtype == np.float64:
        nan = np.isnan(want.view(np.float64))
        assert np.array_equal(np.isnan(got.view(np.float64)), nan)   # NaN at the same rows ...
        assert np.array_equal(got[~nan], want[~nan])                 # ... every other row bit for bit; null slots 0
    else:
        assert np.array_equal(got, want)
    assert np.array_equal(b[:nb], pack(ok))                          # validity; row 0 null; the padding bits of the last byte clear
    assert (v[n:cap] == POISON).all() and (b[nb:] == 0xA5).all()


def assert_distinct(col, o, nd, cap):
    want = distinct_want(col)
    assert nd == len(want)
    if nd == 0:
        assert_untouched([o], cap)
        return
    v, b = raw(o, cap)
    nb = (nd + 7) // 8
    assert o.length == nd and o.type == col.typ and o.null_count == 0
    assert np.array_equal(v[:nd], want)
    assert np.array_equal(b[:nb], pack(np.ones(nd, bool)))
    assert (v[nd:cap] == POISON).all() and (b[nb:] == 0xA5).all()


def assert_mask(keep, mask, selected, first, last):
    rows = np.flatnonzero(keep)
    assert selected == len(rows)
    assert (first, last) == ((rows[0], rows[-1]) if len(rows) else (-1, -1))
    assert np.array_equal(mask, pack(keep))


# ------------------------------------------------------------------ runners
def run_drop(frame, idx=None, in_res=HOST, out_res=HOST, cap=None, mask_too=True):
    n = len(frame[0].values)
    cap = n if cap is None else cap
    keep = keep_rows(frame, idx)
    cols = [place(c, in_res) for c in frame]
    try:
        outs, first, count, contiguous = capi.drop_nils(cols, idx, outs=make_outs(len(frame), cap, out_res))
        assert_result(frame, keep, outs, cap, first, count, contiguous)
        if mask_too:
            assert_mask(keep, *capi.valid_mask(cols, idx))
    finally:
        release(cols)
    return keep, outs


def run_diff(frame, idx=None, in_res=HOST, out_res=HOST, cap=None):
    n = len(frame[0].values)
    cap = n if cap is None else cap
    sel = sorted(set(idx)) if idx else list(range(len(frame)))
    cols = [place(c, in_res) for c in frame]
    try:
        outs = capi.diff(cols, idx, outs=make_outs(len(sel), cap, out_res))
        assert len(outs) == len(sel)      # an unselected column has no output slot
        for i, o in zip(sel, outs):
            assert_diff(frame[i], o, cap)
    finally:
        release(cols)
    return outs


def run_distinct(col, in_res=HOST, out_res=HOST, cap=None):
    cap = int(valid_of(col).sum()) if cap is None else cap
    c = place(col, in_res)
    try:
        out, nd = capi.distinct(c, out=make_outs(1, cap, out_res)[0])
        assert_distinct(col, out, nd, cap)
    finally:
        release([c])
    return out, nd


# ------------------------------------------------------------------ null patterns
def nulls_none(n, rng):
    return np.ones(n, bool)


def nulls_all(n, rng):
    return np.zeros(n, bool)


def nulls_random(p):
    return lambda n, rng: rng.random(n) >= p


def nulls_one_in_a_tile(n, rng):
    v = np.ones(n, bool)
    v[T // 2::T] = False
    return v


def nulls_at(*where):
    """the reference's "consecutively at start/middle/end", scaled past a tile where the frame is long enough"""
    def f(n, rng):
        v = np.ones(n, bool)
        run = T + 3 if n > 4 * T else max(n // 5, 1)
        for w in where:
            lo = {"start": 0, "middle": (n - run) // 2, "end": n - run}[w]
            v[max(lo, 0):lo + run] = False
        return v
    return f


NULLS = {
    "none": nulls_none, "all": nulls_all, "sparse": nulls_one_in_a_tile, "p0.3": nulls_random(0.3),
    "start": nulls_at("start"), "middle": nulls_at("middle"), "end": nulls_at("end"), "start+middle+end": nulls_at("start", "middle", "end"),
}
SELECTIONS = [None, [1], [1, 2], [2, 1, 1]]
SWEEP = [(n, name) for n in ROW_COUNTS for name in NULLS]


def sweep_frame(n, name, offset_a=3, offset_b=65):
    """three columns: Int64 without a bitmap; Float64 with the pattern's nulls (null_count given); Int64 with a few nulls of its own
    (null_count -1: to be read)"""
    rng = np.random.default_rng(100 + n % 1000)
    return [Col(rng.integers(-50, 50, n)),
            Col(rng.standard_normal(n), NULLS[name](n, rng), offset=offset_a),
            Col(rng.integers(I64_MIN, I64_MAX, n), rng.random(n) < 0.9, offset=offset_b, null_count_known=False)]


# ------------------------------------------------------------------ valid_mask / drop_nils
@pytest.mark.parametrize("n,name", SWEEP, ids=["%d-%s" % s for s in SWEEP])
def test_drop_nils_row_counts_and_null_patterns(n, name):
    frame = sweep_frame(n, name)
    for k, idx in enumerate(SELECTIONS):
        run_drop(frame, idx, mask_too=(k < 2))


def test_drop_nils_past_the_first_workgroup_of_the_scan():
    """T * 4096 + 1 rows: the last tile is the first count of the scan's second workgroup; device-resident, 30 % nulls"""
    n = N_SCAN
    rng = np.random.default_rng(5)
    frame = [Col(np.arange(n, dtype=np.int64)), Col(rng.standard_normal(n), rng.random(n) >= 0.3, offset=7)]
    frame[1].valid[-1] = True
    keep = keep_rows(frame)
    cols = [place(c, DEVICE) for c in frame]
    cap = int(keep.sum())
    outs, first, count, contiguous = capi.drop_nils(cols, outs=make_outs(2, cap, DEVICE))
    assert_result(frame, keep, outs, cap, first, count, contiguous)
    mask, selected, lo, hi = capi.valid_mask(cols, [1, 0])
    assert_mask(keep, mask, selected, lo, hi)


@pytest.mark.parametrize("offset", OFFSETS)
def test_arrow_offsets(offset):
    """every call at a bit offset that is no multiple of 8 / 32 / 64, with stray bits in front of and behind the slice"""
    n = T + 65
    frame = sweep_frame(n, "p0.3", offset_a=offset, offset_b=(offset + 64) if offset else 0)
    run_drop(frame)
    run_drop(frame, [2])
    run_diff(frame)
    run_distinct(Col(np.random.default_rng(offset).integers(0, 40, n).astype(np.float64), frame[1].valid, offset=offset))
    # a device-resident bitmap whose first byte is not word-aligned either
    run_drop(frame, [1], in_res=DEVICE, out_res=DEVICE)
    run_diff(frame, [1, 2], in_res=DEVICE, out_res=DEVICE)


@pytest.mark.parametrize("out_res", [HOST, DEVICE, PINNED], ids=["out-host", "out-device", "out-pinned"])
@pytest.mark.parametrize("in_res", [HOST, DEVICE, PINNED], ids=["in-host", "in-device", "in-pinned"])
def test_residencies(in_res, out_res):
    for n in (65, T + 1):
        frame = sweep_frame(n, "p0.3")
        run_drop(frame, None, in_res, out_res)
        run_diff(frame, [2, 1], in_res, out_res)
        run_distinct(Col(np.random.default_rng(n).integers(-20, 20, n), frame[1].valid, offset=1), in_res, out_res)


@pytest.mark.parametrize("mask_res", [HOST, DEVICE], ids=["mask-host", "mask-device"])
@pytest.mark.parametrize("and_res", [HOST, PINNED, DEVICE], ids=["and-host", "and-pinned", "and-device"])
def test_valid_mask_and_mask_and_output_residencies(and_res, mask_res):
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    frame = sweep_frame(n, "p0.3")
    and_bits = rng.random(n) < 0.7
    keep = keep_rows(frame, None, and_bits)
    am = pack(and_bits)
    if and_res == DEVICE:
        am = capi.DeviceBuffer.from_numpy(np.concatenate([np.zeros(1, np.uint8), am]))
        am.ptr += 1     # (a caller bitmap at an odd address)
    elif and_res == PINNED:
        buf = capi.page_aligned(len(am), np.uint8)
        buf[:] = am
        capi.host_register(buf)
        am = buf
    cols = [c.column() for c in frame]
    try:
        mask, selected, first, last = capi.valid_mask(cols, and_mask=am, out_residency=mask_res, mask_pinned=and_res == PINNED)
        if mask_res == DEVICE:
            mask = mask.to_numpy(np.uint8, (n + 7) // 8)
        assert_mask(keep, mask, selected, first, last)
        # without a bitmap to look at, a device-resident mask is still written: all ones, padding clear
        mask, selected, first, last = capi.valid_mask(cols, [0], out_residency=mask_res)
        if mask_res == DEVICE:
            mask = mask.to_numpy(np.uint8, (n + 7) // 8)
        assert_mask(np.ones(n, bool), mask, selected, first, last)
    finally:
        if and_res == DEVICE:
            am.ptr -= 1
        elif and_res == PINNED:
            capi.host_unregister(am)


@pytest.mark.parametrize("n", [1, 65, T + 1, 3 * T + 17])
@pytest.mark.parametrize("mask_res", [HOST, DEVICE], ids=["mask-host", "mask-device"])
def test_valid_mask_then_compact_equals_drop_nils_and_feeds_filter(n, mask_res):
    frame = sweep_frame(n, "p0.3")
    keep = keep_rows(frame, [1, 2])
    cols = [c.column() for c in frame]
    mask, selected, first, last = capi.valid_mask(cols, [1, 2], out_residency=mask_res)
    assert selected == keep.sum()
    cap = max(int(selected), 1)
    a, fa, ca, ga = capi.compact(cols, mask, outs=make_outs(3, cap, HOST))
    b, fb, cb, gb = capi.drop_nils(cols, [2, 1], outs=make_outs(3, cap, HOST))
    assert (fa, ca, ga) == (fb, cb, gb)
    assert_result(frame, keep, a, cap, fa, ca, ga)
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(raw(x, cap), raw(y, cap)))
        assert (x.length, x.null_count, x.type) == (y.length, y.null_count, y.type)
    # a Filter and a DropNils in one compaction: the mask as and_mask of bowgpu_filter
    wanted = np.arange(-30, 0, dtype=np.int64)
    both = keep & np.isin(frame[0].values, wanted)
    cap = max(int(both.sum()), 1)
    outs, first, count, contiguous = capi.filter(cols, [(0, wanted)], and_mask=mask, outs=make_outs(3, cap, HOST))
    assert_result(frame, both, outs, cap, first, count, contiguous)


@pytest.mark.parametrize("ncols", [GROUP + 1, 2 * GROUP + 1, MASK_COLS + 2])
def test_more_columns_than_a_launch_takes(ncols):
    """more columns than one scatter / diff launch moves (kMoveCols) and more bitmaps than one mask launch ANDs (kValidMaskCols)"""
    n = T + 77
    rng = np.random.default_rng(ncols)
    frame = [Col(rng.integers(-9, 9, n) if i % 2 else rng.standard_normal(n), rng.random(n) < 0.97, offset=i, null_count_known=bool(i % 3))
             for i in range(ncols)]
    run_drop(frame)
    run_drop(frame, [ncols - 1, 0])
    run_diff(frame)
    run_diff(frame, [ncols - 1, 1, ncols - 1])


def test_contiguous_answers_and_capacity():
    n = 2 * T
    rng = np.random.default_rng(3)
    vals = rng.standard_normal(n)
    for valid, want in ((nulls_none(n, rng), (0, n)), (nulls_all(n, rng), (0, 0)), (nulls_at("start")(n, rng), (n // 5, n - n // 5)),
                        (nulls_at("end")(n, rng), (0, n - n // 5))):
        frame = [Col(np.arange(n, dtype=np.int64)), Col(vals, valid, offset=5, null_count_known=False)]
        cols = [c.column() for c in frame]
        outs, first, count, contiguous = capi.drop_nils(cols, outs=make_outs(2, 1, HOST))     # (no capacity is needed to say so)
        assert (first, count, contiguous) == (want[0], want[1], True)
        assert_untouched(outs, 1)
    valid = rng.random(n) < 0.5
    frame = [Col(np.arange(n, dtype=np.int64)), Col(vals, valid)]
    cols = [c.column() for c in frame]
    need = int(valid.sum())
    for out_res in (HOST, DEVICE):
        outs = make_outs(2, need, out_res)
        outs[1] = make_outs(1, need - 1, out_res)[0]
        with pytest.raises(capi.BowGpuError) as e:      # one slot short: the size needed is named and nothing is written
            capi.drop_nils(cols, outs=outs)
        assert e.value.code == ERR_ARG and "%d needed" % need in e.value.message
        assert_untouched(outs[:1], need)
        assert_untouched(outs[1:], need - 1)
        outs, first, count, contiguous = capi.drop_nils(cols, outs=make_outs(2, need, out_res))   # exact
        assert_result(frame, valid, outs, need, first, count, contiguous)


# ------------------------------------------------------------------ diff
@pytest.mark.parametrize("n", ROW_COUNTS[1:])
def test_diff_row_counts(n):
    rng = np.random.default_rng(n)
    frame = [Col(rng.integers(I64_MIN, I64_MAX, n)), Col(rng.standard_normal(n), rng.random(n) >= 0.3, offset=7),
             Col(rng.integers(-5, 5, n), rng.random(n) >= 0.3, offset=64, null_count_known=False), Col(rng.standard_normal(n))]
    run_diff(frame)
    run_diff(frame, [1])
    run_diff(frame, [3, 0])


def test_diff_past_2_pow_24_rows_device_resident():
    n = N_SCAN
    rng = np.random.default_rng(9)
    frame = [Col(rng.standard_normal(n), rng.random(n) >= 0.3, offset=1)]
    run_diff(frame, None, DEVICE, DEVICE)


def test_diff_null_pairs_across_word_and_tile_boundaries():
    """a null at i only, at i-1 only, at both - with the pair inside a word, astride a 64-row word, a 256-row wave trip, a tile"""
    n = 2 * T + 9
    for typ in (np.int64, np.float64):
        vals = (np.arange(n) ** 2).astype(typ)
        for edge in (5, 64, 128, 256, 1024, T, 2 * T):
            for nulls in ((edge,), (edge - 1,), (edge - 1, edge), (edge, edge + 1), ()):
                valid = np.ones(n, bool)
                valid[list(nulls)] = False
                outs = run_diff([Col(vals, valid, offset=3)])
                assert outs[0].null_count == 1 + len(set(nulls) | {i + 1 for i in nulls})
    for n in (1, 2):      # one-row frames: row 0 is null whatever it holds
        outs = run_diff([Col(np.arange(n, dtype=np.int64)), Col(np.ones(n), np.ones(n, bool))])
        assert [o.null_count for o in outs] == [1, 1]


def test_diff_integer_wrap_and_float_specials():
    ints = np.array([I64_MAX, I64_MIN, I64_MAX, 0, I64_MIN, -1, I64_MAX], np.int64)      # MIN - MAX = 1, MAX - MIN = -1 (wrapped)
    outs = run_diff([Col(ints)])
    assert outs[0].host_arrays()[0].tolist()[:3] == [0, 1, -1]
    tiny = np.float64(5e-324)
    flts = np.array([np.inf, np.inf, -np.inf, 1.0, np.inf, tiny, 2 * tiny, -tiny, 1e308, -1e308, 3.5, 3.5, -0.0, 0.0, np.nan, 1.0,
                     1.5 * 2.0 ** -1030, 2.0 ** -1030], np.float64)      # (the last two: denormals)
    flts = np.concatenate([flts, np.frombuffer(np.array([0x7FF8DEADBEEF0001, 0xFFF0000000000000], np.uint64).tobytes(), np.float64)])
    outs = run_diff([Col(flts)])
    got = outs[0].host_arrays()[0]
    assert np.isnan(got[[1, 14, 15]]).all() and got[2] == -np.inf      # inf - inf; a NaN in, a NaN out (assert_diff has compared every row)
    assert got[11] == 0.0 and not np.signbit(got[11])      # x - x = +0
    rng = np.random.default_rng(2)
    wide = rng.integers(0, 1 << 64, T + 3, dtype=np.uint64).view(np.float64)      # every exponent, NaNs and infinities among them
    run_diff([Col(wide, rng.random(T + 3) < 0.9, offset=65)])


# ------------------------------------------------------------------ distinct
def order_keys(name, n, rng):
    if name == "all-equal":
        return np.full(n, 42, np.int64)
    if name == "all-distinct":
        return rng.permutation(n).astype(np.int64) * 3 - n
    if name == "sorted-dups":
        return np.sort(rng.integers(0, max(n // 3, 1), n))
    if name == "reversed":
        return np.sort(rng.integers(0, max(n // 3, 1), n))[::-1].copy()
    return rng.integers(-7, 7, n) * (1 << 40)      # shuffled, few values, high digits only


ORDERS = ["all-equal", "all-distinct", "sorted-dups", "reversed", "shuffled"]
DISTINCT_ROWS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


@pytest.mark.parametrize("name", ORDERS)
@pytest.mark.parametrize("n", DISTINCT_ROWS)
def test_distinct_orders_and_row_counts(n, name):
    rng = np.random.default_rng(n)
    keys = order_keys(name, n, rng)
    run_distinct(Col(keys))
    run_distinct(Col(keys.astype(np.float64) / 4, offset=7))
    run_distinct(Col(keys, rng.random(n) < 0.7, offset=63, null_count_known=False))      # nulls interleaved


def test_distinct_past_the_first_workgroup_of_the_scan():
    n = N_SCAN
    rng = np.random.default_rng(8)
    col = Col(rng.integers(0, 1000, n) * 7919 - 4000)
    _, nd = run_distinct(col, DEVICE, DEVICE, cap=1000)
    assert nd == 1000
    run_distinct(Col(np.arange(n, dtype=np.int64) // 3), DEVICE, DEVICE, cap=n // 3 + 1)      # sorted: nothing is sorted again


def test_distinct_group_across_a_tile_of_the_sorted_order():
    """a group of equal values at rows T-1 .. T+1 of the sorted order, its last row in the second tile"""
    rng = np.random.default_rng(4)
    keys = np.concatenate([np.arange(T - 1), [T - 1] * 3, np.arange(T, 2 * T)]).astype(np.int64)
    for k in (keys, rng.permutation(keys)):
        _, nd = run_distinct(Col(k))
        assert nd == 2 * T
        run_distinct(Col(k.astype(np.float64)))


def test_distinct_extremes_zeros_nulls():
    run_distinct(Col(np.array([I64_MAX, 0, I64_MIN, -1, I64_MAX, I64_MIN, 1], np.int64)))
    # -0.0 and +0.0 are one value; the last zero in row order survives, whatever the order and wherever the sort puts them
    for zeros in ([0.0, -0.0], [-0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 0.0, -0.0, 0.0]):
        for rest in ([], [3.5, -2.0], [-1.0, -1.0, 7.0]):      # (zeros alone are "already sorted": the shortcut)
            vals = np.array(zeros[:1] + rest + zeros[1:], np.float64)
            out, nd = run_distinct(Col(vals))
            got = out.host_arrays()[0]
            assert np.signbit(got[got == 0][0]) == np.signbit(np.float64(zeros[-1]))
    n = T + 5
    rng = np.random.default_rng(6)
    vals = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    run_distinct(Col(np.concatenate([vals, [1.0, -1.0]]), np.concatenate([rng.random(n) < 0.5, [True, True]])))
    run_distinct(Col(np.array([-np.inf, np.inf, 5e-324, -5e-324, 1.0, np.inf])))
    # all rows null: counted on the device where the caller does not say; nothing is written
    for known in (True, False):
        out, nd = run_distinct(Col(np.arange(70, dtype=np.int64), np.zeros(70, bool), offset=1, null_count_known=known), DEVICE, HOST, cap=4)
        assert nd == 0


@pytest.mark.parametrize("out_res", [HOST, DEVICE], ids=["out-host", "out-device"])
def test_distinct_nan_and_capacity(out_res):
    n = T + 9
    rng = np.random.default_rng(1)
    vals = rng.integers(0, 50, n).astype(np.float64)
    nan_at = T + 2
    vals[nan_at] = np.nan
    for sort_first in (False, True):      # the NaN is seen by the same read that finds the column in order, or not
        v = np.sort(vals) if sort_first else vals
        out = make_outs(1, n, out_res)[0]
        with pytest.raises(capi.BowGpuError) as e:
            capi.distinct(Col(v).column(), out=out)
        assert e.value.code == ERR_UNSUPPORTED and "NaN" in e.value.message
        assert_untouched([out], n)
    valid = np.ones(n, bool)
    valid[nan_at] = False
    _, nd = run_distinct(Col(vals, valid), HOST, out_res)      # a NaN under a null is no value of the column
    assert nd == 50
    out = make_outs(1, nd - 1, out_res)[0]
    with pytest.raises(capi.BowGpuError) as e:      # one slot short
        capi.distinct(Col(vals, valid).column(), out=out)
    assert e.value.code == ERR_ARG and "%d needed" % nd in e.value.message
    assert_untouched([out], nd - 1)
    run_distinct(Col(vals, valid), HOST, out_res, cap=nd)      # exact


# ------------------------------------------------------------------ the reference's tests
def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "frame_ops_vectors.json")) as f:
        return json.load(f)["cases"]


def _frame(cols):
    out = []
    for c in cols:
        dt = np.int64 if c["type"] == "int64" else np.float64
        data = c["data"]
        out.append(Col(np.array([0 if x is None else x for x in data], dt), np.array([x is not None for x in data], bool)))
    return out


@pytest.mark.parametrize("residency", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("case", _vectors(), ids=[c["name"] for c in _vectors()])
def test_golden_vectors(case, residency):
    frame = _frame(case["cols"])
    n = len(frame[0].values)
    cols = [place(c, residency) for c in frame]
    if case.get("error"):
        with pytest.raises(capi.BowGpuError) as e:
            capi.diff(cols, case["col_idx"])
        assert e.value.code == -6
        return
    want = _frame(case["expected"])
    if case["op"] == "distinct":
        out, nd = capi.distinct(cols[case["col"]], out=make_outs(1, n, residency)[0])
        assert nd == len(want[0].values) and np.array_equal(raw(out, n)[0][:nd], want[0].bits())
        assert_distinct(frame[case["col"]], out, nd, n)
        return
    if case["op"] == "diff":
        sel = sorted(set(case["col_idx"])) or list(range(len(frame)))
        outs = capi.diff(cols, case["col_idx"], outs=make_outs(len(sel), n, residency))
        for i, o in zip(sel, outs):
            assert o.length == n and o.null_count == n - int(want[i].valid.sum())
            if n:
                assert np.array_equal(raw(o, n)[0][:n], want[i].bits()) and np.array_equal(raw(o, n)[1][:(n + 7) // 8], pack(want[i].valid))
        return
    outs, first, count, contiguous = capi.drop_nils(cols, case["col_idx"], outs=make_outs(len(frame), n, residency))
    assert count == len(want[0].values)
    assert (contiguous and count == n) == case["unchanged"]
    if contiguous:
        assert_untouched(outs, n)
        for c, w in zip(frame, want):
            assert np.array_equal(c.bits()[first:first + count], w.bits()) and np.array_equal(c.valid[first:first + count], w.valid)
        return
    for o, w in zip(outs, want):
        assert o.null_count == count - int(w.valid.sum())
        assert np.array_equal(raw(o, n)[0][:count], w.bits()) and np.array_equal(raw(o, n)[1][:(count + 7) // 8], pack(w.valid))


def test_cpp_mirror_replays_the_fixture():
    exe = os.path.join(ROOT, "tests", "cpp", "test_frame_ops")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures, 13 cases" in p.stdout


def test_four_threads_different_calls():
    """four OS threads at once, each its own call on its own context and stream: the bytes are those of the same calls made one by one"""
    n = 3 * T + 17
    frame = sweep_frame(n, "p0.3")
    keys = Col(np.random.default_rng(0).integers(-300, 300, n), frame[1].valid)
    cols = [c.column() for c in frame]

    def snapshot(outs):
        return [(o.length, o.null_count, o.type) + tuple(x.tobytes() for x in raw(o, n)) for o in outs]

    calls = [lambda: snapshot(capi.drop_nils(cols, outs=make_outs(3, n, HOST))[0]),
             lambda: snapshot(capi.diff(cols, [1, 2], outs=make_outs(2, n, DEVICE))),
             lambda: snapshot([capi.distinct(keys.column(), out=make_outs(1, n, HOST)[0])[0]]),
             lambda: capi.valid_mask(cols, [2])[0].tobytes()]
    serial = [call() for call in calls]
    got, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = calls[k]()
        except Exception as e:      # noqa: BLE001 - reported below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == serial
