"""Bow.SortByCol through the C ABI without a GPU: the fixture of the reference's own test literals is well-formed, and everything
bowgpu_sort_by_col / bowgpu_argsort / bowgpu_take decide about host-resident columns before they touch the device - the reference's
"nil values" error, the type and column checks, unequal lengths - is answered on a box that has none.  A valid unsorted call there
is BOWGPU_ERR_NO_DEVICE: the path has no CPU fallback."""
import json
import os

import numpy as np
import pytest

from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sort_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "sort_vectors.json")) as f:
        return json.load(f)


def _gpu_count():
    try:
        return capi.device_count()
    except capi.BowGpuError:
        return 0


def test_fixture_is_well_formed():
    doc = sort_vectors()
    names = [c["name"] for c in doc["cases"]]
    assert len(names) == len(set(names)) == 9
    for want in ("sorted", "unsorted with different cols", "unsorted with nil values and all types", "sorted in desc order",
                 "duplicate values in sort by column", "empty bow", "ERR: nil values in sort by column"):
        assert want in names
    for c in doc["cases"]:
        assert c["source"].startswith("bowsort_test.go:")
        n = len(c["cols"][0]["data"])
        assert 0 <= c["key_col"] < len(c["cols"])
        for col in c["cols"]:
            assert col["type"] in ("int64", "float64") and len(col["data"]) == n
        assert sum(k in c for k in ("expected", "unchanged", "error")) == 1
        key = c["cols"][c["key_col"]]["data"]
        if "error" in c:
            assert None in key and c["error"]["code"] == -16
            continue
        assert None not in key
        order = sorted(range(n), key=lambda i: (key[i], i))   # stable
        if "unchanged" in c:
            assert order == list(range(n))
            continue
        assert order != list(range(n))
        for col, exp in zip(c["cols"], c["expected"]):
            assert exp["name"] == col["name"] and exp["type"] == col["type"]
            assert exp["data"] == [col["data"][i] for i in order], c["name"]


def test_nulls_in_the_key_are_the_references_error():
    case = [c for c in sort_vectors()["cases"] if "error" in c][0]
    cols = [capi.Column.from_list(col["data"], col["type"]) for col in case["cols"]]
    with pytest.raises(capi.BowGpuError) as e:
        capi.sort_by_col(cols, case["key_col"])
    assert e.value.code == -16 == case["error"]["code"] and e.value.message == case["error"]["message"]
    assert capi.ERR_NAMES[-16] == "SORT_NULLS"
    # the count: given, or counted from the bitmap when the caller says -1 (a slice at an odd offset included)
    key = capi.Column.from_list([5, None, 3, None, None, 1, 9], "int64")
    with pytest.raises(capi.BowGpuError) as e:
        capi.argsort(key)
    assert e.value.code == -16 and e.value.message == "column to sort by has 3 nil values"
    sl = capi.Column(key.values, key.validity, capi.INT64, offset=3, length=4, null_count=-1)
    with pytest.raises(capi.BowGpuError) as e:
        capi.sort_by_col([sl], 0)
    assert e.value.code == -16 and e.value.message == "column to sort by has 2 nil values"


def test_validation_on_host_columns_needs_no_gpu():
    ts = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    boolean = capi.Column.from_list([True, False, True], "bool")
    with pytest.raises(capi.BowGpuError) as e:     # key of a type Less is not served for
        capi.sort_by_col([boolean, val], 0)
    assert e.value.code == -7
    with pytest.raises(capi.BowGpuError) as e:
        capi.argsort(boolean)
    assert e.value.code == -7
    for bad in (-1, 2, 7):
        with pytest.raises(capi.BowGpuError) as e:
            capi.sort_by_col([ts, val], bad)
        assert e.value.code == -6, bad
    with pytest.raises(capi.BowGpuError) as e:     # unequal lengths
        capi.sort_by_col([ts, capi.Column.from_list([1.0, 2.0], "float64")], 0, outs=[capi.OutColumn(3), capi.OutColumn(3)])
    assert e.value.code == -10
    with pytest.raises(capi.BowGpuError) as e:     # a value column the device path does not move
        capi.sort_by_col([ts, boolean], 0)
    assert e.value.code == -9
    with pytest.raises(capi.BowGpuError) as e:     # output too small
        capi.sort_by_col([ts, val], 0, outs=[capi.OutColumn(3), capi.OutColumn(2)])
    assert e.value.code == -10
    with pytest.raises(capi.BowGpuError) as e:
        capi.take(boolean, np.array([0], np.int64))
    assert e.value.code == -9
    with pytest.raises(capi.BowGpuError) as e:     # any index into a column without rows is out of range
        capi.take(capi.Column.from_list([], "int64"), np.array([0], np.int64))
    assert e.value.code == -10


def test_nothing_to_sort_returns_the_receiver_without_a_device():
    """0 or 1 rows: sort.IsSorted is true, the reference returns the receiver (bowsort.go:19-21); no device is needed to say so"""
    for data in ([], [7]):
        outs, unchanged = capi.sort_by_col([capi.Column.from_list(data, "int64"), capi.Column.from_list([1.5] * len(data), "float64")], 0)
        assert unchanged
        for o in outs:   # untouched
            assert o.null_count == -1 and (o.values == 0x5A5A5A5A5A5A5A5A).all() and (o.validity == 0xA5).all()
        perm, is_sorted = capi.argsort(capi.Column.from_list(data, "float64"))
        assert is_sorted and perm is None
    out = capi.take(capi.Column.from_list([1, 2], "int64"), np.zeros(0, np.int64))
    assert out.length == 0 and out.null_count == 0 and out.type == capi.INT64


def test_no_cpu_fallback_without_gpu():
    if _gpu_count() > 0:
        pytest.skip("a GPU is present")
    ts = capi.Column.from_list([10, 16, 15], "int64")
    val = capi.Column.from_list([1.0, 2.0, 3.0], "float64")
    with pytest.raises(capi.BowGpuError) as e:
        capi.sort_by_col([ts, val], 0)
    assert e.value.code == -11
    with pytest.raises(capi.BowGpuError) as e:
        capi.argsort(ts)
    assert e.value.code == -11
    with pytest.raises(capi.BowGpuError) as e:
        capi.take(val, np.array([2, 0], np.int64))
    assert e.value.code == -11
