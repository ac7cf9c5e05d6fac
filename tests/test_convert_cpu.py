"""Bow.Convert through the C ABI without a GPU: the header, the binding and the library hold bowgpu_convert; everything it decides
about its arguments - type codes, null arguments, negative lengths and offsets, residencies, capacities - is answered before any
device is touched, with the outputs untouched; calls without rows or without columns succeed on a box that has no GPU; and a
well-formed call with rows is BOWGPU_ERR_NO_DEVICE there: the path has no CPU fallback."""
import os
import re

import numpy as np
import pytest

import convert_model as cm
from bow_amd import capi
from convert_model import B, F, I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A
ERR_UNSUPPORTED, ERR_ARG, ERR_NO_DEVICE = -9, -10, -11


def _gpu_count():
    try:
        return capi.device_count()
    except capi.BowGpuError:
        return 0


def untouched(outs):
    return all(o.null_count == -1 and o.type == 0 and (o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)


def raises(code, call):
    with pytest.raises(capi.BowGpuError) as e:
        call()
    assert e.value.code == code, e.value.message
    return e.value.message


def raw(cols, types, outs, ncols=None):
    oarr = (capi.Out * max(len(outs), 1))(*[o.c() for o in outs])
    tarr = (capi.C.c_int32 * max(len(types), 1))(*types)
    return capi.lib().bowgpu_convert(capi._cols(cols), tarr, len(cols) if ncols is None else ncols, oarr)


def test_header_binding_and_library_hold_the_symbol():
    with open(os.path.join(ROOT, "include", "bowgpu.h")) as f:
        header = f.read()
    assert re.search(r"int bowgpu_convert\(const bowgpu_col \*cols, const int32_t \*to_types, int32_t ncols, bowgpu_out \*outs\);", header)
    assert "#define BOWGPU_ABI_VERSION 14" in header
    assert "bowgpu_convert" in header.split("#define BOWGPU_ABI_VERSION")[0]          # named where the header lists what 14 holds
    for word in ("0x8000000000000000", "amd64", "must not overlap", "BOWGPU_ERR_NO_DEVICE"):
        assert word in header.split("/* ---- Bow.Convert")[1].split("int bowgpu_convert")[0], word
    assert "bowgpu_convert" in capi.SYMBOLS
    assert hasattr(capi.lib(), "bowgpu_convert")


def test_declines_come_before_any_device():
    ints = capi.Column.from_list([3, None, 2], "int64")
    flts = capi.Column.from_list([1.0, None, 3.0], "float64")
    bools = capi.Column.from_list([True, False, None], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)

    def outs(k, slots=3):
        return [capi.OutColumn(slots) for _ in range(k)]

    # a String source or target: the reference's own loop serves those
    for src in (ints, flts, bools):
        o = outs(2)
        assert "String" in raises(ERR_UNSUPPORTED, lambda: capi.convert([ints, src], [F, capi.STRING], outs=o))
        assert untouched(o)
    for to in cm.TYPES:
        o = outs(2)
        raises(ERR_UNSUPPORTED, lambda: capi.convert([string, ints], [to, to], outs=o))
        assert untouched(o)
    # any other type code, as source or as target
    for code in (0, 5, 6, 7, -1, 99):
        o = outs(1)
        raises(ERR_ARG, lambda: capi.convert([flts], [code], outs=o))
        odd = capi.Column(np.zeros(3, np.int64), None, code, 0, 3, 0)
        raises(ERR_ARG, lambda: capi.convert([odd], [I], outs=o))
        assert untouched(o)
    # null arguments with ncols > 0, a negative count
    o = outs(1)
    oarr = (capi.Out * 1)(o[0].c())
    tarr = (capi.C.c_int32 * 1)(I)
    L = capi.lib()
    assert L.bowgpu_convert(None, tarr, 1, oarr) == ERR_ARG
    assert L.bowgpu_convert(capi._cols([flts]), None, 1, oarr) == ERR_ARG
    assert L.bowgpu_convert(capi._cols([flts]), tarr, 1, None) == ERR_ARG
    assert L.bowgpu_convert(capi._cols([flts]), tarr, -1, oarr) == ERR_ARG
    # a negative length or offset, an unknown residency of a column
    for field, value in (("length", -1), ("offset", -1), ("residency", 9)):
        carr = capi._cols([ints, flts])
        setattr(carr[1], field, value)
        o = outs(2)
        oarr = (capi.Out * 2)(o[0].c(), o[1].c())
        tarr = (capi.C.c_int32 * 2)(B, B)
        assert L.bowgpu_convert(carr, tarr, 2, oarr) == ERR_ARG, field
        assert untouched(o)
    # outputs: an unknown residency, a missing buffer, a capacity below the column's length
    for spoil in ("values", "validity", "residency", "length"):
        o = outs(2)
        oarr = (capi.Out * 2)(o[0].c(), o[1].c())
        if spoil == "residency":
            oarr[1].residency = 9
        elif spoil == "length":
            oarr[1].length = 2
        else:
            setattr(oarr[1], spoil, None)
        tarr = (capi.C.c_int32 * 2)(F, I)
        assert L.bowgpu_convert(capi._cols([ints, flts]), tarr, 2, oarr) == ERR_ARG, spoil
        assert untouched(o)
    assert "3 needed" in raises(ERR_ARG, lambda: capi.convert([bools], [I], outs=outs(1, 2)))
    # a column with rows and no values buffer
    carr = capi._cols([ints])
    carr[0].values = None
    o = outs(1)
    assert L.bowgpu_convert(carr, (capi.C.c_int32 * 1)(F), 1, (capi.Out * 1)(o[0].c())) == ERR_ARG
    assert untouched(o)


def test_zero_rows_and_zero_columns_need_no_device():
    assert capi.convert([], []) == []
    assert raw([], [], [], 0) == 0
    assert capi.lib().bowgpu_convert(None, None, 0, None) == 0
    empties = {I: capi.Column.from_list([], "int64"), F: capi.Column.from_list([], "float64"), B: capi.Column.from_list([], "bool")}
    nullable = capi.Column(np.zeros(0, np.int64), np.zeros(1, np.uint8), I, 0, 0, -1)
    cols = [empties[a] for a, _ in cm.PAIRS] + [nullable]
    types = [b for _, b in cm.PAIRS] + [B]
    outs = capi.convert(cols, types)
    assert [(o.length, o.null_count, o.type) for o in outs] == [(0, 0, t) for t in types]
    assert all((o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)
    # a capacity is allowed to be larger; an offset into nothing is no error
    outs = capi.convert([capi.Column(np.zeros(9, np.float64), None, F, 9, 0, 0)], [B], outs=[capi.OutColumn(5)])
    assert (outs[0].length, outs[0].null_count, outs[0].type) == (0, 0, B)
    # the declines hold for calls without rows too
    raises(ERR_UNSUPPORTED, lambda: capi.convert([empties[I]], [capi.STRING]))
    raises(ERR_ARG, lambda: capi.convert([empties[I]], [0]))


def test_no_cpu_fallback_without_gpu():
    """well-formed calls with rows: served where there is a GPU, BOWGPU_ERR_NO_DEVICE where there is none"""
    ints = capi.Column.from_list([3, None, 0, -7], "int64")
    flts = capi.Column.from_list([1.5, None, -0.0, 1e30], "float64")
    bools = capi.Column.from_list([True, False, None, True], "bool")
    calls = ((lambda: capi.convert([ints], [B])[0].to_list(), [True, None, False, True]),
             (lambda: capi.convert([flts], [I])[0].to_list(), [1, None, 0, cm.INT64_MIN]),
             (lambda: capi.convert([bools], [F])[0].to_list(), [1.0, 0.0, None, 1.0]),
             (lambda: [o.null_count for o in capi.convert([ints, capi.Column.from_list([], "bool"), bools], [F, I, B])], [1, 0, 1]))
    if _gpu_count() > 0:
        for call, want in calls:
            assert call() == want
        return
    for call, _ in calls:
        raises(ERR_NO_DEVICE, call)
