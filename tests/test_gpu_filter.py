"""Bow.Filter on the device (bowgpu_filter_mask / bowgpu_compact / bowgpu_filter) against numpy boolean indexing, which is exact: every
comparison here is bit for bit - values, validity bits, null_count, zeroed null slots, clear padding bits, and the sentinels of the
output buffers intact past the rows produced (or everywhere, in the contiguous case)."""
import ctypes as C
import functools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from bow_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A
HOST, DEVICE, PINNED = capi.HOST, capi.DEVICE, capi.HOST_PINNED

T = 4096                      # rows per tile (bow_amd/csrc/common.h kFilterTileRows)
GROUP = 4                     # columns per scatter launch (kMoveCols)
# The tile counts are scanned by sort.hip's three-launch scan: one workgroup covers kScanBlock = kThreads * kScanItems = 256 * 16 =
# 4096 counts, i.e. 4096 tiles = 4096 * 4096 rows.  One row more makes tile 4096, the first count of the scan's second workgroup.
SCAN_BLOCK_TILES = 256 * 16
N_SCAN = T * SCAN_BLOCK_TILES + 1
ROW_COUNTS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, N_SCAN]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ------------------------------------------------------------------ frames, the oracle, the comparison
class Col:
    """one column of a test frame: values (int64 / float64), valid (bool array or None), the Arrow offset it is sliced at"""

    def __init__(self, values, valid=None, offset=0, null_count_known=True):
        self.values, self.valid, self.offset, self.known = np.ascontiguousarray(values), valid, offset, null_count_known
        self.typ = capi.INT64 if self.values.dtype == np.int64 else capi.FLOAT64

    def column(self):
        n, off = len(self.values), self.offset
        junk = np.full(off, -77, self.values.dtype)
        vals = np.concatenate([junk, self.values])
        if self.valid is None:
            return capi.Column(vals, None, self.typ, off, n, 0)
        bits = np.concatenate([np.arange(off) % 2 == 0, self.valid, np.ones(5, bool)])   # (stray bits before and behind the slice)
        bm = np.packbits(bits, bitorder="little")
        return capi.Column(vals, bm, self.typ, off, n, int(n - self.valid.sum()) if self.known else -1)

    def bits(self):
        return self.values.view(np.uint64)


def place(col, residency):
    c = col.column()
    if residency == DEVICE:
        return c.to_device()
    if residency == PINNED:
        pc = capi.Column(capi.page_aligned(len(c.values), c.values.dtype), None if c.validity is None else capi.page_aligned(len(c.validity), np.uint8),
                         c.type, c.offset, c.length, c.null_count)
        pc.values[:] = c.values
        if c.validity is not None:
            pc.validity[:] = c.validity
        return pc.pin()
    return c


def release(cols):
    for c in cols:
        if c.residency == PINNED:
            c.unpin()


def make_outs(ncols, cap, residency):
    outs = [capi.OutColumn(cap, residency) for _ in range(ncols)]
    if residency == DEVICE:   # the sentinels of the host-resident forms
        for o in outs:
            v = np.full(max(cap, 1), POISON, np.uint64)
            b = np.full(max((cap + 7) // 8, 1), 0xA5, np.uint8)
            capi.check(capi.lib().bowgpu_memcpy_h2d(C.c_void_p(o.values.ptr), v.ctypes.data_as(C.c_void_p), C.c_int64(v.nbytes)))
            capi.check(capi.lib().bowgpu_memcpy_h2d(C.c_void_p(o.validity.ptr), b.ctypes.data_as(C.c_void_p), C.c_int64(b.nbytes)))
    return outs


def raw(o, cap):
    """the whole output buffers, whatever the call said it produced"""
    nv, nb = max(cap, 1), max((cap + 7) // 8, 1)
    if o.residency == DEVICE:
        return o.values.to_numpy(np.uint64, nv), o.validity.to_numpy(np.uint8, nb)
    return np.asarray(o.values[:nv]).view(np.uint64), np.asarray(o.validity[:nb])


def pred_rows(col, values, match_null=False):
    """Go's == of the boxed value against each of `values` (numpy's == is IEEE for float64, exact for int64); nil == nil"""
    x = col.values
    hit = np.zeros(len(x), bool)
    for v in np.asarray(values, dtype=x.dtype):
        hit |= x == v
    if col.valid is not None:
        hit = np.where(col.valid, hit, bool(match_null))
    return hit


def oracle_keep(frame, preds, and_bits=None):
    keep = np.ones(len(frame[0].values) if frame else 0, bool)
    for p in preds:
        keep &= pred_rows(frame[p[0]], p[1], p[2] if len(p) > 2 else False)
    if and_bits is not None:
        keep &= and_bits
    return keep


def is_contiguous(keep):
    rows = np.flatnonzero(keep)
    return len(rows) == 0 or len(rows) == rows[-1] - rows[0] + 1


def pack(bits):
    return np.packbits(bits, bitorder="little") if len(bits) else np.zeros(0, np.uint8)


def assert_untouched(outs, cap):
    for o in outs:
        v, b = raw(o, cap)
        assert o.null_count == -1 and o.type == 0
        assert (v == POISON).all() and (b == 0xA5).all()


def assert_result(frame, keep, outs, cap, first, count, contiguous):
    rows = np.flatnonzero(keep)
    assert count == len(rows)
    assert contiguous == is_contiguous(keep)
    if contiguous:
        assert first == (rows[0] if len(rows) else 0)
        assert_untouched(outs, cap)
        return
    nb = (count + 7) // 8
    for col, o in zip(frame, outs):
        valid = np.ones(count, bool) if col.valid is None else col.valid[rows]
        want = np.where(valid, col.bits()[rows], np.uint64(0))
        v, b = raw(o, cap)
        assert o.length == count and o.type == col.typ and o.null_count == count - int(valid.sum())
        assert np.array_equal(v[:count], want)                       # raw payloads; null slots 0
        assert np.array_equal(b[:nb], pack(valid))                   # validity bits, the padding bits of the last byte clear
        assert (v[count:cap] == POISON).all() and (b[nb:] == 0xA5).all()   # nothing past slot count - 1 / byte ceil(count/8) - 1


def run_filter(frame, preds, and_bits=None, in_res=HOST, out_res=HOST, and_res=HOST, cap=None):
    n = len(frame[0].values)
    cap = n if cap is None else cap
    keep = oracle_keep(frame, preds, and_bits)
    cols = [place(c, in_res) for c in frame]
    try:
        outs = make_outs(len(frame), cap, out_res)
        am = None if and_bits is None else pack(and_bits)
        if am is not None and and_res == DEVICE:
            am = capi.DeviceBuffer.from_numpy(am)
        outs, first, count, contiguous = capi.filter(cols, preds, and_mask=am, outs=outs)
        assert_result(frame, keep, outs, cap, first, count, contiguous)
    finally:
        release(cols)
    return keep, outs


# ------------------------------------------------------------------ selections
def sel_none(n, rng):
    return np.zeros(n, bool)


def sel_all(n, rng):
    return np.ones(n, bool)


def sel_rows(*where):
    def f(n, rng):
        k = np.zeros(n, bool)
        for w in where:
            k[w(n)] = True
        return k
    return f


def tile_run(n):
    """a run of consecutive rows across a tile boundary (the first one, where the frame has one; else across a word boundary or less)"""
    edge = T if n > T + 5 else 64 if n > 70 else n // 2
    return slice(max(edge - 5, 0), min(edge + 5, n))


def sel_run(n, rng):
    k = np.zeros(n, bool)
    k[tile_run(n)] = True
    return k


def sel_run_and_far_row(n, rng):
    k = sel_run(n, rng)
    r = tile_run(n)
    k[n - 1 if n - 1 > r.stop else 0] = True   # one more row, away from the run
    return k


def sel_alternating(n, rng):
    return np.arange(n) % 2 == 0


def sel_random(p):
    def f(n, rng):
        return rng.random(n) < p
    return f


def sel_empty_tiles_between(n, rng):
    """rows in tiles 0, 2 and the last one only: whole tiles without a selected row in between"""
    k = rng.random(n) < 0.3
    tile = np.arange(n) // T
    return k & ((tile == 0) | (tile == 2) | (tile == (n - 1) // T))


def sel_count(multiple_of_64):
    def f(n, rng):
        m = min(128, n // 2 // 64 * 64)   # a non-contiguous selection of exactly m rows (every other row), m a multiple of 64
        k = np.zeros(n, bool)
        k[np.arange(m if multiple_of_64 else m + 1) * 2] = True
        return k
    return f


SELECTIONS = {
    "none": (sel_none, 0), "all": (sel_all, 0),
    "row0": (sel_rows(lambda n: 0), 1), "last": (sel_rows(lambda n: n - 1), 1), "middle": (sel_rows(lambda n: n // 2), 3),
    "run": (sel_run, 4), "run+far": (sel_run_and_far_row, 16),
    "alternating": (sel_alternating, 3), "p0.01": (sel_random(0.01), 1), "p0.5": (sel_random(0.5), 1), "p0.99": (sel_random(0.99), 1),
    "empty_tiles": (sel_empty_tiles_between, 2 * T + 1), "count%64==0": (sel_count(True), 200), "count%64!=0": (sel_count(False), 200),
}
SWEEP = [(n, name) for n in ROW_COUNTS for name, (_, min_rows) in SELECTIONS.items() if n >= min_rows]


@functools.lru_cache(maxsize=2)
def sweep_value_column(n):
    """the Float64 value column of the sweep: nulls, a slice at bit offset 3; device-resident copies are made once per row count"""
    rng = np.random.default_rng(1000 + n % 1000)
    col = Col(rng.standard_normal(n), rng.random(n) < 0.8, offset=3)
    return col, (place(col, DEVICE) if n == N_SCAN else None)


@pytest.mark.parametrize("n,name", SWEEP, ids=["%d-%s" % s for s in SWEEP])
def test_row_counts_and_selections(n, name):
    """the selection is made by a predicate on an Int64 column: rows to keep hold one of three wanted values, the others never do"""
    rng = np.random.default_rng(7)
    keep = SELECTIONS[name][0](n, rng)
    wanted = np.array([5, I64_MIN, 1 << 40], np.int64)
    key = np.where(keep, wanted[np.arange(n) % 3], rng.integers(6, 1000, n))
    val, val_dev = sweep_value_column(n)
    frame = [Col(key), val]
    preds = [(0, wanted)]
    if name == "run" and n > 1:
        assert is_contiguous(keep) and keep.sum() > 1
    if name == "run+far" or name.startswith("count"):
        assert not is_contiguous(keep)
    if name.startswith("count"):
        assert (keep.sum() % 64 == 0) == name.endswith("==0")
    if n < N_SCAN:
        got, _ = run_filter(frame, preds)
        assert np.array_equal(got, keep)
        return
    # the large frame lives on the device (the value column uploaded once); outputs device-resident too
    cols = [place(frame[0], DEVICE), val_dev]
    cap = int(keep.sum()) if not is_contiguous(keep) else 8
    outs, first, count, contiguous = capi.filter(cols, preds, outs=make_outs(2, cap, DEVICE))
    assert_result(frame, keep, outs, cap, first, count, contiguous)


# ------------------------------------------------------------------ the reference's table
def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "filter_vectors.json")) as f:
        return json.load(f)["cases"]


def _convert(v):
    if isinstance(v, str):
        try:
            return float(v)
        except ValueError:
            return None
    return float(v)


@pytest.mark.parametrize("residency", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("case", _vectors(), ids=[c["name"] for c in _vectors()])
def test_golden_vectors(case, residency):
    frame = [Col(np.array(c["data"], np.float64)) for c in case["cols"]]
    preds = []
    for p in case["preds"]:
        conv = [_convert(v) for v in p["values"]]
        preds.append((p["col"], np.array([v for v in conv if v is not None], np.float64), any(v is None for v in conv)))
    keep, outs = run_filter(frame, preds, in_res=residency, out_res=residency)
    assert int(keep.sum()) == case["count"] and is_contiguous(keep) == case["contiguous"]
    if case["contiguous"]:
        assert (np.flatnonzero(keep)[0] if case["count"] else 0) == case["first"]
    else:
        assert outs[0].host_arrays()[0].tolist() == case["expected"][0]["data"]


# ------------------------------------------------------------------ predicates
N = 3 * T + 17


def mixed_frame(n=N, seed=3):
    """Int64 without nulls; Int64 with nulls at offset 8; Float64 with nulls, NaNs and both zeros at offset 3; Float64 without nulls"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 6, n)
    b = rng.integers(-3, 3, n)
    b[rng.random(n) < 0.05] = I64_MIN
    b[rng.random(n) < 0.05] = I64_MAX
    f = rng.integers(-2, 3, n).astype(np.float64)
    f[rng.random(n) < 0.1] = np.nan
    f[rng.random(n) < 0.1] = -0.0
    g = rng.integers(0, 4, n) * 0.25
    return [Col(a), Col(b, rng.random(n) < 0.7, offset=8, null_count_known=False), Col(f, rng.random(n) < 0.6, offset=3), Col(g)]


PRED_CASES = {
    "int-1-value": [(0, [3])],
    "int-2-values": [(0, [0, 5])],
    "int-32-values": [(1, [I64_MIN, I64_MAX] + list(range(100, 129)) + [-2])],
    "int-min-max": [(1, [I64_MIN, I64_MAX])],
    "float-nan-in-set-and-column": [(2, [np.nan, 1.0])],
    "float-only-nan": [(2, [np.nan])],
    "float-minus-zero-in-set": [(2, [-0.0])],
    "float-plus-zero-in-set": [(2, [0.0, 2.0])],
    "match-null-with-nulls": [(2, [1.0], True)],
    "match-null-alone": [(1, [], True)],
    "match-null-without-nulls": [(0, [], True)],
    "match-null-and-values-without-nulls": [(3, [0.5], True)],
    "no-values": [(0, [])],
    "two-preds": [(0, [1, 2, 3]), (2, [0.0, 1.0, -1.0])],
    "eight-preds": [(0, [0, 1, 2, 3, 4]), (1, [-3, -2, -1, 0, 1, 2, I64_MAX], True), (2, [-2.0, -1.0, 0.0, 1.0, 2.0], True),
                    (3, [0.0, 0.25, 0.5]), (0, [1, 2, 3, 4, 5]), (3, [0.25, 0.5, 0.75]), (1, [-3, -1, 0, 1, 2, I64_MAX], True), (0, [1, 2, 3])],
}


@pytest.mark.parametrize("name", list(PRED_CASES))
def test_predicates(name):
    frame = mixed_frame()
    keep, _ = run_filter(frame, PRED_CASES[name])
    if name in ("float-only-nan", "match-null-without-nulls", "no-values"):
        assert not keep.any()
    if name == "float-minus-zero-in-set":   # both zeros of the column match, whatever their sign bit
        zeros = frame[2].valid & (frame[2].values == 0)
        assert np.array_equal(keep, zeros) and len({int(x) for x in frame[2].bits()[zeros]}) == 2
    if name in ("match-null-alone",):
        assert np.array_equal(keep, ~frame[1].valid)


@pytest.mark.parametrize("and_res", [HOST, DEVICE], ids=["host-mask", "device-mask"])
def test_predicates_anded_with_a_caller_mask_and_a_mask_alone(and_res):
    frame = mixed_frame()
    rng = np.random.default_rng(11)
    bits = rng.random(N) < 0.4
    keep, _ = run_filter(frame, [(0, [1, 2, 3])], and_bits=bits, and_res=and_res)
    assert keep.any() and not np.array_equal(keep, bits)
    keep, _ = run_filter(frame, [], and_bits=bits, and_res=and_res)
    assert np.array_equal(keep, bits)
    run_filter(frame, [], and_bits=np.zeros(N, bool), and_res=and_res)     # nothing: the empty slice
    run_filter(frame, [], and_bits=np.ones(N, bool), and_res=and_res)      # everything: a slice, nothing written


def test_registered_host_masks_are_read_in_place():
    """and_mask / mask with BOWGPU_HOST_PINNED residency; a buffer that was never registered is BOWGPU_ERR_ARG saying so"""
    frame = mixed_frame(n=T + 100)
    n = T + 100
    cols = [c.column() for c in frame]
    bits = np.random.default_rng(21).random(n) < 0.4
    m = capi.page_aligned((n + 7) // 8, np.uint8)
    m[:] = pack(bits)
    capi.host_register(m)
    try:
        preds = [(0, [1, 2, 3])]
        keep = oracle_keep(frame, preds, bits)
        outs, first, count, contiguous = capi.filter(cols, preds, and_mask=m, mask_pinned=True, outs=make_outs(4, n, HOST))
        assert_result(frame, keep, outs, n, first, count, contiguous)
        mask, selected, lo, hi = capi.filter_mask(cols, preds, and_mask=m, mask_pinned=True)
        assert np.array_equal(mask, pack(keep)) and selected == keep.sum()
        outs, first, count, contiguous = capi.compact(cols, m, mask_pinned=True, outs=make_outs(4, n, HOST))
        assert_result(frame, bits, outs, n, first, count, contiguous)
    finally:
        capi.host_unregister(m)
    plain = capi.page_aligned((n + 7) // 8, np.uint8)     # pages of its own, never registered
    plain[:] = pack(bits)
    outs = make_outs(4, n, HOST)
    for call in (lambda: capi.filter(cols, [(0, [1])], and_mask=plain, mask_pinned=True, outs=outs),
                 lambda: capi.compact(cols, plain, mask_pinned=True, outs=outs)):
        with pytest.raises(capi.BowGpuError) as e:
            call()
        assert e.value.code == -10 and "not registered" in e.value.message
    assert_untouched(outs, n)


# ------------------------------------------------------------------ columns
@pytest.mark.parametrize("ncols", [1, GROUP, GROUP + 1, 2 * GROUP + 1])
def test_column_counts_cross_the_launch_group(ncols):
    rng = np.random.default_rng(ncols)
    frame = []
    for c in range(ncols):
        if c % 2 == 0:
            frame.append(Col(rng.integers(0, 4, N), None if c == 0 else rng.random(N) < 0.5, offset=(0, 3, 8)[c % 3]))
        else:
            frame.append(Col(rng.standard_normal(N), rng.random(N) < 0.9, offset=(0, 3, 8)[c % 3], null_count_known=c % 4 == 1))
    run_filter(frame, [(0, [1, 3])])
    run_filter(frame, [(ncols - 1, [0.0, 2.0], True)] if ncols % 2 == 0 else [(ncols - 1, [2], ncols > 1)])


MOVE_ROWS = [1, 63, 64, 65, T - 1, T, T + 1]          # validity-word and tile edges
RES3 = (DEVICE, HOST, PINNED)


@pytest.mark.parametrize("n", MOVE_ROWS)
@pytest.mark.parametrize("ncols,pred_cols", [(GROUP + 1, (4,)), (2 * GROUP + 1, (0, 4))], ids=["5cols-pred4", "9cols-pred0+4"])
def test_predicate_column_in_the_second_group_mixed_columns(ncols, pred_cols, n):
    """Launch groups of 4 + 1 and 4 + 4 + 1 columns.  Column 4 - pageable host memory with nulls, staged for the predicate pass - is
    moved with the second group; inside every group the inputs differ in residency and in having nulls, the outputs in residency"""
    rng = np.random.default_rng(100 * ncols + n)
    frame = []
    for c in range(ncols):
        vals = rng.integers(0, 4, n) if c % 2 == 0 else rng.standard_normal(n)
        nullable = c % 2 == 1 or c == 4
        frame.append(Col(vals, rng.random(n) < 0.7 if nullable else None, offset=(0, 3, 8)[c % 3], null_count_known=c % 4 != 1))
    preds = [(c, [1, 3]) for c in pred_cols]
    keep = oracle_keep(frame, preds)
    cols = [place(col, RES3[c % 3]) for c, col in enumerate(frame)]
    try:
        outs = [make_outs(1, n, (HOST, DEVICE)[(c // 2) % 2])[0] for c in range(ncols)]
        outs, first, count, contiguous = capi.filter(cols, preds, outs=outs)
        assert_result(frame, keep, outs, n, first, count, contiguous)
    finally:
        release(cols)
    assert is_contiguous(keep) == (n == 1)


@pytest.mark.parametrize("mask_res", [HOST, DEVICE], ids=["mask-host", "mask-device"])
@pytest.mark.parametrize("and_res", [HOST, PINNED, DEVICE], ids=["and-host", "and-pinned", "and-device"])
def test_filter_mask_and_mask_and_output_residencies(and_res, mask_res):
    n = T + 1
    frame = mixed_frame(n=n)
    cols = [c.column() for c in frame]
    bits = np.random.default_rng(41).random(n) < 0.6
    preds = [(0, [1, 2, 3])]
    keep = oracle_keep(frame, preds, bits)
    rows = np.flatnonzero(keep)
    am = pack(bits)
    if and_res == DEVICE:
        am = capi.DeviceBuffer.from_numpy(am)
    elif and_res == PINNED:
        am = capi.page_aligned((n + 7) // 8, np.uint8)
        am[:] = pack(bits)
        capi.host_register(am)
    try:
        mask, selected, first, last = capi.filter_mask(cols, preds, and_mask=am, out_residency=mask_res, mask_pinned=and_res == PINNED)
    finally:
        if and_res == PINNED:
            capi.host_unregister(am)
    assert (selected, first, last) == (len(rows), rows[0], rows[-1])
    got = mask if mask_res == HOST else mask.to_numpy(np.uint8, (n + 7) // 8)
    assert np.array_equal(got, pack(keep))


@pytest.mark.parametrize("offset", [0, 3, 8])
@pytest.mark.parametrize("dtype", [np.int64, np.float64], ids=["int64", "float64"])
def test_sliced_columns_with_validity(dtype, offset):
    rng = np.random.default_rng(offset)
    n = 2 * T + 77
    vals = rng.integers(0, 5, n).astype(dtype)
    frame = [Col(vals, rng.random(n) < 0.7, offset=offset), Col(rng.standard_normal(n), rng.random(n) < 0.5, offset=offset)]
    run_filter(frame, [(0, [1, 4])])
    run_filter(frame, [(0, [2], True)])


def test_nan_payloads_survive():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 51, N).astype(np.uint64) | np.uint64(0x7FF8000000000000) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    frame = [Col(rng.integers(0, 3, N)), Col(bits.view(np.float64), rng.random(N) < 0.9, offset=3)]
    keep, outs = run_filter(frame, [(0, [1])])
    got = outs[1].host_arrays()[0].view(np.uint64)
    valid = frame[1].valid[keep]
    assert np.array_equal(got[valid], bits[keep][valid]) and len(set(got[valid].tolist())) > 100


@pytest.mark.parametrize("out_res", [HOST, DEVICE, PINNED], ids=["out-host", "out-device", "out-pinned"])
@pytest.mark.parametrize("in_res", [HOST, DEVICE, PINNED], ids=["in-host", "in-device", "in-pinned"])
def test_residencies(in_res, out_res):
    frame = mixed_frame(n=T + 100)
    run_filter(frame, [(0, [1, 2]), (2, [0.0, 1.0], True)], in_res=in_res, out_res=out_res)
    run_filter(frame, [(0, [0, 1, 2, 3, 4, 5])], in_res=in_res, out_res=out_res)   # everything: nothing written


# ------------------------------------------------------------------ the two-call form
@pytest.mark.parametrize("n", [1, 65, T + 1, N])
@pytest.mark.parametrize("mask_res", [HOST, DEVICE], ids=["mask-host", "mask-device"])
def test_filter_mask_then_compact_equals_filter(n, mask_res):
    frame = mixed_frame(n=n)
    rng = np.random.default_rng(n)
    and_bits = rng.random(n) < 0.8
    cols = [c.column() for c in frame]
    for preds, ab in (([(0, [0, 2, 4]), (2, [0.0, 1.0, 2.0], True)], None), ([(0, [0, 2, 4])], and_bits), ([], and_bits), ([(0, [77])], None)):
        keep = oracle_keep(frame, preds, ab)
        mask, selected, first, last = capi.filter_mask(cols, preds, and_mask=None if ab is None else pack(ab), out_residency=mask_res)
        rows = np.flatnonzero(keep)
        assert (selected, first, last) == ((len(rows), rows[0], rows[-1]) if len(rows) else (0, -1, -1))
        got = mask if mask_res == HOST else mask.to_numpy(np.uint8, (n + 7) // 8)
        assert np.array_equal(got, pack(keep))      # (packbits leaves the padding bits of the last byte clear)
        # exact buffers: capacity = selected
        cap = selected if not is_contiguous(keep) else 3
        a, first_a, count_a, cont_a = capi.compact(cols, mask, outs=make_outs(len(cols), cap, HOST))
        assert_result(frame, keep, a, cap, first_a, count_a, cont_a)
        b, first_b, count_b, cont_b = capi.filter(cols, preds, and_mask=None if ab is None else pack(ab), outs=make_outs(len(cols), cap, HOST))
        assert (first_a, count_a, cont_a) == (first_b, count_b, cont_b)
        for x, y in zip(a, b):
            assert np.array_equal(raw(x, cap)[0], raw(y, cap)[0]) and np.array_equal(raw(x, cap)[1], raw(y, cap)[1])
            assert (x.length, x.null_count, x.type) == (y.length, y.null_count, y.type)


def test_compact_ignores_mask_bits_past_the_last_row():
    frame = mixed_frame(n=13)
    keep = np.arange(13) % 3 == 0
    mask = pack(keep)
    mask[-1] |= 0xE0
    outs, first, count, contiguous = capi.compact([c.column() for c in frame], mask, outs=make_outs(4, 13, HOST))
    assert_result(frame, keep, outs, 13, first, count, contiguous)


@pytest.mark.parametrize("out_res", [HOST, DEVICE], ids=["out-host", "out-device"])
def test_capacity(out_res):
    frame = mixed_frame()
    preds = [(0, [1, 4])]
    count = int(oracle_keep(frame, preds).sum())
    run_filter(frame, preds, out_res=out_res, cap=count)      # exactly count slots
    cols = [c.column() for c in frame]
    for short in ([count - 1] * 4, [count, count, count - 1, count]):
        outs = [make_outs(1, cap, out_res)[0] for cap in short]
        with pytest.raises(capi.BowGpuError) as e:
            capi.filter(cols, preds, outs=outs)
        assert e.value.code == -10 and ("%d needed" % count) in e.value.message
        for o, cap in zip(outs, short):
            assert_untouched([o], cap)


def test_same_call_twice_gives_the_same_bytes():
    frame = mixed_frame()
    cols = [c.column() for c in frame]
    preds = [(0, [1, 2, 3]), (2, [0.0, 1.0], True)]
    runs = []
    for _ in range(2):
        outs, first, count, contiguous = capi.filter(cols, preds, outs=make_outs(4, N, HOST))
        mask = capi.filter_mask(cols, preds)[0]
        runs.append([raw(o, N)[0].tobytes() + raw(o, N)[1].tobytes() for o in outs] + [mask.tobytes(), (first, count, contiguous)])
    assert runs[0] == runs[1]


def test_four_threads_filter_their_own_frames():
    errors = []

    def work(k):
        try:
            frame = mixed_frame(seed=100 + k)
            for _ in range(3):
                run_filter(frame, [(0, [k % 6, (k + 2) % 6]), (3, [0.0, 0.25 * (k % 4)])])
        except BaseException as e:   # noqa: BLE001 - reported in the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_cpp_mirror_replays_the_fixture():
    """tests/cpp/test_filter: Bow::MakeFilterValues / Bow::Filter of the C++ mirror over the fixture's cases, plus a user closure"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_filter")
    assert os.path.exists(exe), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures, 8 tables" in r.stdout
