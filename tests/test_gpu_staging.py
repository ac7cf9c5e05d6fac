"""The staging layer (bow_amd/csrc/dev_cols.cpp) under the entry points: validity bitmaps of 8-byte columns at odd byte addresses,
in device memory and in registered host memory, and the argument checks of an output whose values are bit-packed.  Every
comparison is exact."""
import functools

import numpy as np
import pytest

from bow_amd import capi
from oracle import pyoracle as orc
from bool_agg_common import bool_cols, compare_exact
from staging_common import Shifted

pytestmark = pytest.mark.gpu

# rows per window: inside one 32-bit bitmap word (5, 20), across one word boundary (10), across several (70), 64 rows on a 64-bit
# boundary (rows 128 .. 191), single rows, a run of empty windows; the Arrow offset and the pointer's shift move all of them
LENS = [5, 20, 10, 70, 23, 64, 1, 2, 33, 0, 0, 0, 3, 31, 32, 1, 9]
AGGS = [("WindowStart", 0), ("Count", 1), ("Sum", 1), ("Min", 1), ("First", 1), ("WeightedAverageStep", 1)]


@functools.lru_cache(maxsize=None)
def frame(arrow_offset):
    """the frame [ts Int64, value Float64 with ~30 % nulls, key Int64 with nulls] sliced at `arrow_offset`: host columns, the
    oracle's Aggregate results and the HOST-residency results of the product, computed once"""
    assert sum(LENS[:5]) == 128 and sum(LENS) == 304
    rng = np.random.default_rng(40 + arrow_offset)
    ts = np.concatenate([k * 10 + np.arange(m, dtype=np.int64) * 10 // m for k, m in enumerate(LENS) if m])   # every window spans time
    n = len(ts)
    vals = rng.integers(-1000, 1000, n) / 4.0      # (sums of these are exact in any order)
    valid = rng.random(n) >= 0.3
    key = rng.integers(0, 4, n).astype(np.int64)
    key_valid = rng.random(n) >= 0.2

    def sliced(values, bits):
        v = np.concatenate([np.full(arrow_offset, -77, values.dtype), values])
        if bits is None:
            return capi.Column(v, None, None, arrow_offset, n, 0)
        stray = np.concatenate([np.arange(arrow_offset) % 2 == 0, bits, np.ones(5, bool)])   # (stray bits before and behind the slice)
        return capi.Column(v, np.packbits(stray, bitorder="little"), None, arrow_offset, n, -1)

    cols = [sliced(ts, None), sliced(vals, valid), sliced(key, key_valid)]
    want, _ = orc.aggregate([orc.Column(ts, None, orc.INT64), orc.Column(vals, np.packbits(valid, bitorder="little"), orc.FLOAT64)], 0, 10, AGGS)
    host, _ = capi.rolling_aggregate(cols[:2], 0, 10, AGGS)
    assert 0.2 < 1 - valid.mean() < 0.4 and host[3].null_count > 0      # (Min: the empty windows, the windows of nulls only)
    return cols, want, host


def raw(o):
    v, b = o.host_arrays()
    return o.length, o.type, o.null_count, np.asarray(v).tobytes(), np.asarray(b).tobytes()


def shifted_device_column(col, shift):
    """the column device-resident, its validity behind a pointer `shift` bytes into an allocation (bytes of ones around it)"""
    lead, tail = np.full(shift, 0xFF, np.uint8), np.full(8, 0xFF, np.uint8)
    db = capi.DeviceBuffer.from_numpy(np.concatenate([lead, col.validity, tail]))
    return capi.Column(capi.DeviceBuffer.from_numpy(col.values.view(np.uint8)), Shifted(db, shift), col.type, col.offset, col.length, col.null_count)


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("arrow_offset", [0, 5])
def test_validity_pointer_at_an_odd_byte_address(arrow_offset, where, shift):
    cols, want, host = frame(arrow_offset)
    registered = []
    try:
        if where == "device":
            ccols = [cols[0].to_device(), shifted_device_column(cols[1], shift)]
        else:
            ccols = []
            for c, s in ((cols[0], 0), (cols[1], shift)):
                v = capi.page_aligned(c.values.size, c.values.dtype)
                v[:] = c.values
                b = None
                if c.validity is not None:   # the bitmap starts `shift` bytes into a registered page-aligned array
                    page = capi.page_aligned(s + c.validity.size + 8, np.uint8, 0xFF)
                    page[s:s + c.validity.size] = c.validity
                    b = page[s:s + c.validity.size]
                    assert b.ctypes.data % 4 == s % 4
                for arr in (v, page if b is not None else None):
                    if arr is not None:
                        capi.host_register(arr)
                        registered.append(arr)
                pc = capi.Column(v, b, c.type, c.offset, c.length, c.null_count)
                assert b is None or pc.validity.ctypes.data == b.ctypes.data
                pc.residency = capi.HOST_PINNED
                ccols.append(pc)
        got, _ = capi.rolling_aggregate(ccols, 0, 10, AGGS)
        for (kind, _c), g, w, h in zip(AGGS, got, want, host):
            label = "%s off=%d shift=%d %s" % (where, arrow_offset, shift, kind)
            compare_exact(label, g, w)
            assert raw(g) == raw(h), label
    finally:
        for arr in registered:
            capi.host_unregister(arr)
    if where != "device":
        return
    # the same shifted column moved by Filter (move_group_prepare), the predicate on another column, null rows matching
    preds = [(2, [1, 2], True)]
    h_outs, h_first, h_count, h_contig = capi.filter(cols, preds)
    d_cols = [cols[0].to_device(), ccols[1], shifted_device_column(cols[2], shift)]
    d_outs, d_first, d_count, d_contig = capi.filter(d_cols, preds)
    assert (d_first, d_count, d_contig) == (h_first, h_count, h_contig) and not h_contig and 0 < h_count < cols[0].length
    assert h_outs[1].null_count > 0 and h_outs[2].null_count > 0      # (match_null rows are among the selected)
    for i, (d, h) in enumerate(zip(d_outs, h_outs)):
        assert raw(d) == raw(h), ("filter off=%d shift=%d column %d" % (arrow_offset, shift, i))


def test_unknown_residency_of_a_boolean_output():
    ts = np.arange(40, dtype=np.int64)
    ccols, _ = bool_cols(ts, ts % 3 == 0, ts % 5 != 0)
    outs = [capi.OutColumn(4, capi.HOST) for _ in range(2)]
    outs[1].residency = 7
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate(ccols, 0, 10, [("WindowStart", 0), ("First", 1)], outs=outs)
    assert e.value.code == -10 and "unknown residency 7" in e.value.message, e.value.message
