"""AppendBows and Bow.Find / FindNext / Contains through the C ABI without a GPU: the fixture of the reference's own test literals is
well-formed, and everything bowgpu_append / bowgpu_find_next decide about host-resident arguments before they touch the device - the
number of pieces, unequal lengths, types, the row limit, capacities - is answered on a box that has none, as are a single piece, pieces
without rows and the searches that need no look at the column.  A valid call with rows to move or to look at is BOWGPU_ERR_NO_DEVICE
there: the path has no CPU fallback."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A
ERR_TYPE, ERR_UNSUPPORTED, ERR_ARG, ERR_NO_DEVICE = -7, -9, -10, -11
MAX_PIECES = 1 << 18      # include/bowgpu.h: the stated limit of bowgpu_append


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "append_find_vectors.json")) as f:
        return json.load(f)


def case_cols(cols):
    return [capi.Column.from_list(c["data"], c["type"]) for c in cols]


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


def scan(data, value, start):
    """bowfind.go:11-27 in plain Python"""
    if value is None:
        return next((i for i, x in enumerate(data) if x is None), -1)
    return next((i for i in range(start, len(data)) if data[i] is not None and data[i] == value), -1)


def test_fixture_is_well_formed():
    doc = vectors()
    names = [c["name"] for c in doc["cases"]]
    assert len(names) == len(set(names)) == 7
    assert "bowappend_test.go" in doc["source"] and "bowfind_test.go" in doc["source"]
    for word in ("String", "Boolean", "metadata", "toto(0)", "other type: not found"):
        assert word in doc["note"]
    files = {"append": "bowappend_test.go:", "find": "bowfind_test.go:"}
    for c in doc["cases"]:
        assert c["source"].startswith(files[c["op"]]), c["name"]
        lo, hi = (int(x) for x in c["source"].split(":")[1].split("-"))
        assert 0 < lo < hi
        if c["op"] == "find":
            assert c["col"]["type"] in ("int64", "float64")
            for lookups, data in ((c["lookups"], c["col"]["data"]), (c["empty_lookups"], [])):
                assert len(lookups) == 4
                for lk in lookups:
                    if isinstance(lk["value"], str):
                        assert lk["value"] == "other type: not found" and lk["expect"] == -1
                    else:
                        assert lk["expect"] == scan(data, lk["value"], lk["row_start"]), (c["name"], lk)
            continue
        for f in c["frames"]:
            assert len({len(col["data"]) for col in f}) == 1
            assert all(col["type"] in ("int64", "float64") for col in f)
        if c.get("error"):
            assert "expected" not in c
            assert any(a["type"] != b["type"] for f in c["frames"] for a, b in zip(c["frames"][0], f))
            continue
        # the expected frame follows from the pieces by plain Python
        want = [sum((f[i]["data"] for f in c["frames"]), []) for i in range(len(c["frames"][0]))]
        assert [e["data"] for e in c["expected"]] == want, c["name"]
        assert [(e["name"], e["type"]) for e in c["expected"]] == [(x["name"], x["type"]) for x in c["frames"][0]]      # (from the first bow)
        assert c["unchanged"] == (len(c["frames"]) == 1)


def test_append_validation_on_host_arguments_needs_no_gpu():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    boolean = capi.Column.from_list([True, False, True], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)
    short = capi.Column.from_list([1.0, 2.0], "float64")

    def outs(k, slots=6):
        return [capi.OutColumn(slots) for _ in range(k)]

    # a column's type differs between pieces: the reference's text (bowappend.go:40-42), whichever piece it is
    o = outs(2)
    assert "incompatible types 'float64' and 'int64'" in raises(ERR_TYPE, lambda: capi.append([[key, val], [key, key]], outs=o))
    assert "incompatible types 'int64' and 'float64'" in raises(ERR_TYPE, lambda: capi.append([[key, val], [key, val], [val, val]], outs=o))
    # Boolean / String anywhere
    for bad in (boolean, string):
        raises(ERR_UNSUPPORTED, lambda: capi.append([[key, bad], [key, bad]], outs=o))
        raises(ERR_UNSUPPORTED, lambda: capi.append([[key, val], [key, bad]], outs=o))
        raises(ERR_UNSUPPORTED, lambda: capi.append([[bad]], outs=o[:1]))
    # unequal lengths inside a piece
    raises(ERR_ARG, lambda: capi.append([[key, val], [key, short]], outs=o))
    raises(ERR_ARG, lambda: capi.append([[key, short]], outs=o))
    assert untouched(o)
    # no piece
    unchanged = C.c_int32(7)
    oarr = (capi.Out * 1)(o[0].c())
    parr = (C.POINTER(capi.Col) * 1)()
    for nframes in (0, -1):
        assert capi.lib().bowgpu_append(parr, nframes, 1, oarr, C.byref(unchanged)) == ERR_ARG
    # more pieces than the stated limit (at least 65536): named
    assert MAX_PIECES >= 65536
    one = capi._cols([key])
    many = (C.POINTER(capi.Col) * (MAX_PIECES + 1))(*([C.cast(one, C.POINTER(capi.Col))] * (MAX_PIECES + 1)))
    assert capi.lib().bowgpu_append(many, MAX_PIECES + 1, 1, oarr, C.byref(unchanged)) == ERR_UNSUPPORTED
    assert str(MAX_PIECES) in capi.lib().bowgpu_last_error().decode()
    # 2^31 rows in total: the limit is named (nothing is read: the pieces claim a length they do not have)
    half = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 30, 0)
    assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.append([[half], [half]], outs=o[:1]))
    # capacity: the total is needed
    o = outs(2, 5)
    assert "6 needed" in raises(ERR_ARG, lambda: capi.append([[key, val], [key, val]], outs=o))
    o = [capi.OutColumn(6), capi.OutColumn(5)]
    assert "6 needed" in raises(ERR_ARG, lambda: capi.append([[key, val], [key, val]], outs=o))
    assert untouched(o)
    # outputs: an unknown residency, a missing buffer; null arguments
    for spoil in ("values", "residency"):
        o = outs(2)
        oarr = (capi.Out * 2)(o[0].c(), o[1].c())
        if spoil == "values":
            oarr[1].values = None
        else:
            oarr[1].residency = 9
        fr = capi._cols([key, val])
        parr = (C.POINTER(capi.Col) * 2)(C.cast(fr, C.POINTER(capi.Col)), C.cast(fr, C.POINTER(capi.Col)))
        assert capi.lib().bowgpu_append(parr, 2, 2, oarr, C.byref(unchanged)) == ERR_ARG, spoil
        assert untouched(o)
    assert capi.lib().bowgpu_append(parr, 2, 2, oarr, None) == ERR_ARG
    assert capi.lib().bowgpu_append(None, 2, 2, oarr, C.byref(unchanged)) == ERR_ARG
    assert capi.lib().bowgpu_append(parr, 2, 2, None, C.byref(unchanged)) == ERR_ARG


def test_one_piece_is_unchanged_and_pieces_without_rows_need_no_device():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    outs, unchanged = capi.append([[key, val]])      # bowappend.go:19-21: the argument itself
    assert unchanged and untouched(outs)
    empty = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    nullable = [capi.Column(np.zeros(0, np.int64), np.zeros(1, np.uint8), capi.INT64, 0, 0, -1), capi.Column.from_list([], "float64")]
    for frames in ([empty, empty], [empty, nullable, empty]):
        outs, unchanged = capi.append(frames, capacity=4)
        assert not unchanged
        assert [(o.length, o.null_count, o.type) for o in outs] == [(0, 0, capi.INT64), (0, 0, capi.FLOAT64)]
        assert all((o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)
    # the fixture's cases that move no row
    for c in vectors()["cases"]:
        if c["op"] != "append":
            continue
        frames = [case_cols(f) for f in c["frames"]]
        total = sum(len(f[0]["data"]) for f in c["frames"])
        if c.get("error"):
            o = [capi.OutColumn(total) for _ in frames[0]]
            assert c["error"] in raises(ERR_TYPE, lambda: capi.append(frames, outs=o))
            assert untouched(o)
        elif total == 0 or len(frames) == 1:
            outs, unchanged = capi.append(frames, capacity=2)
            assert unchanged == c["unchanged"]
            assert unchanged or [o.length for o in outs] == [0] * len(outs)


def test_find_next_validation_and_answers_that_need_no_device():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, 2.0, 3.0], "float64")
    stated = capi.Column(np.array([5, 6, 7], np.int64), np.zeros(1, np.uint8), capi.INT64, 0, 3, 0)      # (the bitmap is not read)
    boolean = capi.Column.from_list([True, False, True], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)
    for bad in (boolean, string):
        raises(ERR_UNSUPPORTED, lambda: capi.find_next(bad, 1))
    raises(ERR_ARG, lambda: capi.find_next(key, 1, -1))
    huge = capi.Column(np.zeros(1, np.int64), np.zeros(1, np.uint8), capi.INT64, 0, 1 << 31, -1)
    assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.find_next(huge, 1))
    c, row, v = key.c(), C.c_int64(7), np.array([1], np.int64)
    assert capi.lib().bowgpu_find_next(None, C.c_int64(0), v.ctypes.data_as(C.c_void_p), C.byref(row)) == ERR_ARG
    assert capi.lib().bowgpu_find_next(C.byref(c), C.c_int64(0), v.ctypes.data_as(C.c_void_p), None) == ERR_ARG
    # zero rows; a row_start past the end; a NaN value; nil on a column with no nulls to look at
    for empty in (capi.Column.from_list([], "int64"), capi.Column(np.zeros(0, np.float64), np.zeros(1, np.uint8), capi.FLOAT64, 0, 0, -1)):
        assert capi.find_next(empty, 1) == -1 and capi.find_next(empty, None) == -1 and capi.find_next(empty, 1, 1) == -1
    assert capi.find_next(key, 1, 3) == -1 and capi.find_next(val, 2.0, 1000) == -1
    assert capi.find_next(val, math.nan) == -1 and capi.find_next(val, math.nan, 2) == -1
    assert capi.find_next(key, None) == -1 and capi.find_next(val, None, 2) == -1 and capi.find_next(stated, None) == -1
    # the fixture's lookups on the empty slice
    for c in vectors()["cases"]:
        if c["op"] != "find":
            continue
        empty = capi.Column.from_list([], c["col"]["type"])
        for lk in c["empty_lookups"]:
            if not isinstance(lk["value"], str):
                assert capi.find_next(empty, lk["value"], lk["row_start"]) == lk["expect"] == -1


def test_no_cpu_fallback_without_gpu():
    """valid calls with rows to move or to look at: served where there is a GPU, BOWGPU_ERR_NO_DEVICE where there is none"""
    key = capi.Column.from_list([10, 16, 15, 16], "int64")
    val = capi.Column.from_list([1.0, None, 3.0, 4.5], "float64")
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    calls = ((lambda: capi.append([[key, val], [key, val]])[0][1].null_count, 2),
             (lambda: capi.append([none, [key, val]])[0][0].length, 4),
             (lambda: capi.find_next(key, 16), 1),
             (lambda: capi.find_next(key, 16, 2), 3),
             (lambda: capi.find_next(key, 11), -1),
             (lambda: capi.find_next(val, 4.5), 3),
             (lambda: capi.find_next(val, None, 3), 1))
    if _gpu_count() > 0:
        for call, want in calls:
            assert call() == want
        return
    for call, _ in calls:
        raises(ERR_NO_DEVICE, call)
