"""What the tests of Rolling.Aggregate over Boolean columns share: frames with a Boolean value column for the product and for
the oracle, the exact comparison of an output (Boolean results included) and the closed forms the device kernel rests on."""
import numpy as np

from bow_amd import capi
from oracle import pyoracle as orc

VALUE_AGGS = ["Sum", "ArithmeticMean", "Min", "Max", "Count", "First", "Last", "Mode"]   # bool_windows_kernel
TIME_AGGS = ["IntegralStep", "IntegralTrapezoid", "WeightedAverageStep", "WeightedAverageLinear"]   # through the widening
BOOL_RESULT = {"First", "Last", "Mode"}


def pack(bits, offset=0, tail=0, fill=False):
    """bools -> Arrow LSB-first bytes with `offset` leading and `tail` trailing bits of `fill`"""
    b = np.concatenate([np.full(offset, fill, bool), np.asarray(bits, bool), np.full(tail, fill, bool)])
    return np.packbits(b, bitorder="little") if b.size else np.zeros(0, np.uint8)


def bool_cols(ts, vals, valid, offset=0, null_count=-1):
    """(product columns, oracle columns) of the frame [ts Int64, value Boolean]; valid None: no validity buffer.  The bits
    around the column's own (Arrow offset, padding of the last byte) are set so that a kernel reading them shows up"""
    n = len(ts)
    vb = pack(vals, offset, 5, True)
    mb = None if valid is None else pack(valid, offset, 5, True)
    ccols = [capi.Column(np.asarray(ts, np.int64), None, capi.INT64),
             capi.Column(vb, mb, capi.BOOLEAN, offset, n, 0 if mb is None else null_count)]
    ocols = [orc.Column(np.asarray(ts, np.int64), None, orc.INT64), orc.Column(vb, mb, orc.BOOLEAN, offset, n)]
    return ccols, ocols


def compare_exact(name, got, want):
    """got: capi.OutColumn, want: orc.Column - type, length, null count, validity bytes, value bits, null slots 0, padding clear"""
    assert got.type == want.type, (name, got.type, want.type)
    assert got.length == want.length, (name, got.length, want.length)
    n = got.length
    nb = (n + 7) // 8
    gv, gb = got.host_arrays()
    wm = want.valid_mask()
    assert np.array_equal(np.asarray(gb[:nb]), want.validity[:nb]), (name, "validity", np.flatnonzero(got.valid_mask() != wm)[:10])
    assert got.null_count == int((~wm).sum()), (name, got.null_count, int((~wm).sum()))
    if got.type == capi.BOOLEAN:
        gbits = np.unpackbits(np.asarray(gv[:nb]), bitorder="little")[:n].astype(bool)
        wbits = orc.unpack_validity(want.values, n)
        assert not gbits[~wm].any(), (name, "null slots hold 0")
        assert np.array_equal(gbits[wm], wbits[wm]), (name, np.flatnonzero(gbits != wbits)[:10])
        if n % 8:
            assert (int(gv[nb - 1]) >> (n % 8)) == 0, (name, "value padding bits")
    else:
        g64, w64 = gv.view(np.uint64), want.values[:n].view(np.uint64)
        assert not g64[~wm].any(), (name, "null slots hold 0")
        bad = np.flatnonzero(g64[wm] != w64[wm])
        assert bad.size == 0, (name, bad[:10], gv[wm][bad[:5]], want.values[:n][wm][bad[:5]])
    if n % 8:
        assert (int(gb[nb - 1]) >> (n % 8)) == 0, (name, "validity padding bits")


def closed_forms(windows, vals, valid):
    """the eight value reducers of every window [a, b) from nv, nt and the first / last valid bit: {kind: list with None for nil}"""
    vals, valid = np.asarray(vals, bool), np.asarray(valid, bool)
    out = {k: [] for k in VALUE_AGGS}
    for a, b in windows:
        v, t = valid[a:b], vals[a:b] & valid[a:b]
        nv, nt = int(v.sum()), int(t.sum())
        rows = np.flatnonzero(v)
        out["Sum"].append(float(nt))
        out["Count"].append(nv)
        if nv == 0:
            for k in ("ArithmeticMean", "Min", "Max", "First", "Last", "Mode"):
                out[k].append(None)
            continue
        first, last = bool(t[rows[0]]), bool(t[rows[-1]])
        out["ArithmeticMean"].append(float(nt) / float(nv))
        out["Min"].append(0.0 if nt < nv else 1.0)
        out["Max"].append(1.0 if nt > 0 else 0.0)
        out["First"].append(first)
        out["Last"].append(last)
        out["Mode"].append(True if 2 * nt > nv else False if 2 * nt < nv else (not last))
    return out
