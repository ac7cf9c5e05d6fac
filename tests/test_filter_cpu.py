"""Bow.Filter through the C ABI without a GPU: the fixture of the reference's own test literals is well-formed, and everything
bowgpu_filter / bowgpu_filter_mask / bowgpu_compact decide about host-resident arguments before they touch the device - types, limits,
column indices, unequal lengths - is answered on a box that has none, as are the empty filter and frames without rows.  A valid
selective call there is BOWGPU_ERR_NO_DEVICE: the path has no CPU fallback."""
import json
import os

import numpy as np
import pytest

from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A


def filter_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "filter_vectors.json")) as f:
        return json.load(f)


def convert_float64(v):
    """Type.Convert on a Float64 column (bowtypes.go:64-81): a number, a numeric string, or nil"""
    if isinstance(v, str):
        try:
            return float(v)
        except ValueError:
            return None
    return float(v)


def case_preds(case):
    """the fixture's predicates as capi.filter takes them: (col, converted values, match_null)"""
    out = []
    for p in case["preds"]:
        conv = [convert_float64(v) for v in p["values"]]
        out.append((p["col"], [v for v in conv if v is not None], any(v is None for v in conv)))
    return out


def _gpu_count():
    try:
        return capi.device_count()
    except capi.BowGpuError:
        return 0


def untouched(outs):
    return all(o.null_count == -1 and o.type == 0 and (o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)


def test_fixture_is_well_formed():
    doc = filter_vectors()
    names = [c["name"] for c in doc["cases"]]
    assert len(names) == len(set(names)) == 8
    for want in ("empty filter", "empty result", "match one", "match half", "match all", "not convertible", "match non concomitant"):
        assert want in names
    assert "String" in doc["note"] and "dropped_string_preds" in doc["note"]
    for c in doc["cases"]:
        assert c["source"].startswith("bowsetters_test.go:")
        assert "dropped_string_preds" in c
        assert [col["type"] for col in c["cols"]] == ["float64"]
        data = c["cols"][0]["data"]
        keep = np.ones(len(data), bool)
        for col, values, match_null in case_preds(c):
            assert col == 0
            keep &= np.array([(x is None and match_null) or (x is not None and x in values) for x in data], bool)
        rows = np.flatnonzero(keep)
        assert c["count"] == len(rows), c["name"]
        contiguous = len(rows) == 0 or len(rows) == rows[-1] - rows[0] + 1
        assert c["contiguous"] == contiguous, c["name"]
        if contiguous:
            assert c["first"] == (rows[0] if len(rows) else 0)
        else:
            assert c["expected"][0]["data"] == [data[i] for i in rows]
    assert not [c for c in doc["cases"] if c["name"] == "match half"][0]["count"]
    assert [c for c in doc["cases"] if not c["contiguous"]][0]["name"] == "match non concomitant"


def test_validation_on_host_arguments_needs_no_gpu():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    boolean = capi.Column.from_list([True, False, True], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)
    mask = np.array([0b101], np.uint8)
    for bad in (boolean, string):      # Boolean / String anywhere: as a predicate column, as a value column
        for cols, preds in (([bad, val], [(0, [1])]), ([key, bad], [(0, [1])]), ([key, bad], [])):
            with pytest.raises(capi.BowGpuError) as e:
                capi.filter(cols, preds, and_mask=mask)
            assert e.value.code == -9
            with pytest.raises(capi.BowGpuError) as e:
                capi.filter_mask(cols, preds, and_mask=mask)
            assert e.value.code == -9
            with pytest.raises(capi.BowGpuError) as e:
                capi.compact(cols, mask)
            assert e.value.code == -9
    with pytest.raises(capi.BowGpuError) as e:     # more values than BOWGPU_FILTER_MAX_VALUES
        capi.filter([key, val], [(0, list(range(capi.FILTER_MAX_VALUES + 1)))])
    assert e.value.code == -9 and "BOWGPU_FILTER_MAX_VALUES = 32" in e.value.message
    with pytest.raises(capi.BowGpuError) as e:     # more predicates than BOWGPU_FILTER_MAX_PREDS
        capi.filter_mask([key, val], [(0, [1])] * (capi.FILTER_MAX_PREDS + 1))
    assert e.value.code == -9 and "BOWGPU_FILTER_MAX_PREDS = 8" in e.value.message
    for bad in (-1, 2, 7):
        with pytest.raises(capi.BowGpuError) as e:
            capi.filter([key, val], [(bad, [1])])
        assert e.value.code == -6, bad
        with pytest.raises(capi.BowGpuError) as e:
            capi.filter_mask([key, val], [(0, [1]), (bad, [1])])
        assert e.value.code == -6, bad
    short = capi.Column.from_list([1.0, 2.0], "float64")
    outs = [capi.OutColumn(3), capi.OutColumn(3)]
    with pytest.raises(capi.BowGpuError) as e:     # unequal lengths
        capi.filter([key, short], [(0, [1])], outs=outs)
    assert e.value.code == -10
    with pytest.raises(capi.BowGpuError) as e:
        capi.compact([key, short], mask, outs=outs)
    assert e.value.code == -10
    with pytest.raises(capi.BowGpuError) as e:
        capi.filter_mask([key, short], [(0, [1])])
    assert e.value.code == -10
    assert untouched(outs)
    # outputs: an unknown residency, a missing buffer - decided before the selected count is known
    for spoil in ("values", "residency"):
        outs = [capi.OutColumn(3), capi.OutColumn(3)]
        oarr = (capi.Out * 2)(outs[0].c(), outs[1].c())
        if spoil == "values":
            oarr[1].values = None
        else:
            oarr[1].residency = 9
        first, count, contiguous = capi.C.c_int64(0), capi.C.c_int64(0), capi.C.c_int32(0)
        parr, keepalive = capi._preds([key, val], [(0, [1])])
        rc = capi.lib().bowgpu_filter(capi._cols([key, val]), 2, parr, 1, None, capi.HOST, oarr, capi.C.byref(first), capi.C.byref(count),
                                      capi.C.byref(contiguous))
        assert rc == -10, spoil
        rc = capi.lib().bowgpu_compact(capi._cols([key, val]), 2, mask.ctypes.data_as(capi.C.c_void_p), capi.HOST, oarr, capi.C.byref(first),
                                       capi.C.byref(count), capi.C.byref(contiguous))
        assert rc == -10, spoil
        assert untouched(outs)
    # 2^31 rows and more: the limit is named (nothing is read: the column claims a length it does not have)
    huge = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 31, 0)
    with pytest.raises(capi.BowGpuError) as e:
        capi.filter([huge], [(0, [1])], outs=[capi.OutColumn(1)])
    assert e.value.code == -9 and "2^31" in e.value.message


def test_empty_filter_and_empty_frames_need_no_device():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    outs, first, count, contiguous = capi.filter([key, val], [])      # the reference's "empty filter": every row, a slice
    assert (first, count, contiguous) == (0, 3, True) and untouched(outs)
    mask, selected, lo, hi = capi.filter_mask([key, val], [])
    assert (selected, lo, hi) == (3, 0, 2) and mask.tolist() == [0b111]
    case = [c for c in filter_vectors()["cases"] if c["name"] == "empty filter"][0]
    cols = [capi.Column.from_list(col["data"], col["type"]) for col in case["cols"]]
    outs, first, count, contiguous = capi.filter(cols, case_preds(case))
    assert (first, count, contiguous) == (case["first"], case["count"], case["contiguous"]) and untouched(outs)
    # frames without rows, whatever the selector
    empty = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    for preds, and_mask in (([], None), ([(0, [1, 2])], None), ([(1, [], True)], np.zeros(0, np.uint8))):
        outs, first, count, contiguous = capi.filter(empty, preds, and_mask=and_mask)
        assert (first, count, contiguous) == (0, 0, True) and untouched(outs)
        mask, selected, lo, hi = capi.filter_mask(empty, preds, and_mask=and_mask)
        assert (selected, lo, hi) == (0, -1, -1) and len(mask) == 0
    outs, first, count, contiguous = capi.compact(empty, np.zeros(0, np.uint8))
    assert (first, count, contiguous) == (0, 0, True) and untouched(outs)
    outs, first, count, contiguous = capi.filter([], [])
    assert (first, count, contiguous) == (0, 0, True)


def test_no_cpu_fallback_without_gpu():
    """a valid selective call: served where there is a GPU, BOWGPU_ERR_NO_DEVICE where there is none"""
    key = capi.Column.from_list([10, 16, 15], "int64")
    val = capi.Column.from_list([1.0, 2.0, 3.0], "float64")
    # (the call, the position of the selected count in what it returns)
    calls = ((lambda: capi.filter([key, val], [(0, [10, 15])]), 2),
             (lambda: capi.filter_mask([key, val], [(0, [10, 15])]), 1),
             (lambda: capi.compact([key, val], np.array([0b101], np.uint8)), 2),
             (lambda: capi.filter([key, val], [], and_mask=np.array([0b101], np.uint8)), 2))
    if _gpu_count() > 0:
        for call, count_at in calls:
            assert call()[count_at] == 2      # rows 0 and 2
        return
    for call, _ in calls:
        with pytest.raises(capi.BowGpuError) as e:
            call()
        assert e.value.code == -11
