"""Bow.InnerJoin / OuterJoin through the C ABI without a GPU: the fixture of the reference's own test literals is well-formed - every
expected frame follows from its inputs by a plain-Python restatement of getCommonRows (bowjoin.go:161-186) and the fill rules - and
everything bowgpu_join / bowgpu_join_rows decide about host-resident arguments before they touch the device is answered on a box that
has none, with the outputs untouched.  A valid call with rows to look at is BOWGPU_ERR_NO_DEVICE there: the path has no CPU fallback."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A
ERR_BAD_COL, ERR_TYPE, ERR_UNSUPPORTED, ERR_ARG, ERR_NO_DEVICE = -6, -7, -9, -10, -11
KINDS = {"inner": capi.JOIN_INNER, "outer": capi.JOIN_OUTER}
TYPE_TEXT = "left and right bow on join columns are of incompatible types"


def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "join_vectors.json")) as f:
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


def common_rows(lkey, rkey):
    """getCommonRows (bowjoin.go:161-186): the double loop; Go's == on the boxed value, nil == nil"""
    return [(l, r) for l in range(len(lkey)) for r in range(len(rkey)) if lkey[l] == rkey[r]]


def plain_join(left, right, lk, rk, kind):
    """the expected frame (column-based lists) and the pair list, from the definition"""
    nl = len(left[0]["data"]) if left else 0
    nr = len(right[0]["data"]) if right else 0
    pairs = common_rows(left[lk]["data"], right[rk]["data"]) if lk >= 0 else []
    out_rows = list(pairs)
    if kind == "outer":
        out_rows = []
        for l in range(nl):
            mine = [p for p in pairs if p[0] == l]
            out_rows += mine if mine else [(l, -1)]
        hit = {r for _, r in pairs}
        out_rows += [(-1, r) for r in range(nr) if r not in hit]
    cols = []
    for i, c in enumerate(left):
        data = [c["data"][l] if l >= 0 else (right[rk]["data"][r] if i == lk else None) for l, r in out_rows]
        cols.append({"name": c["name"], "type": c["type"], "data": data})
    for i, c in enumerate(right):
        if i != rk or rk < 0:
            cols.append({"name": c["name"], "type": c["type"], "data": [c["data"][r] if r >= 0 else None for _, r in out_rows]})
    return cols, pairs, out_rows


def test_fixture_is_well_formed():
    doc = vectors()
    names = [c["name"] for c in doc["cases"]]
    assert len(names) == len(set(names)) == 19
    assert "bowjoin_test.go" in doc["source"]
    for word in ("String", "Boolean", "metadata", "declined"):
        assert word in doc["note"]
    for must in ("outer with only nils in common rows", "inner with only nils in common rows", "outer timeSeries like", "inner time series like",
                 "outer with one common column", "outer no common rows", "inner no common rows", "outer no common columns", "inner no common columns",
                 "outer two empty bows", "outer empty right bow", "outer empty left bow"):
        assert "expected" in next(c for c in doc["cases"] if c["name"] == must), must
    for c in doc["cases"]:
        assert c["kind"] in KINDS and c["source"].startswith("bowjoin_test.go:"), c["name"]
        lo, hi = (int(x) for x in c["source"].split(":")[1].split("-"))
        assert 0 < lo < hi
        for frame in (c["left"], c["right"]):
            assert len({len(col["data"]) for col in frame}) <= 1
            assert all(col["type"] in ("int64", "float64") for col in frame)
        common = [n for n in (x["name"] for x in c["left"]) if n in {y["name"] for y in c["right"]}]
        if "declined" in c:
            assert len(common) == 2 and "expected" not in c and "error" not in c and "left_key" not in c
            continue
        lk, rk = c["left_key"], c["right_key"]
        if common:      # the single common column is the key
            assert len(common) == 1 and c["left"][lk]["name"] == c["right"][rk]["name"] == common[0]
        else:
            assert lk == rk == -1
        if "error" in c:
            assert c["error"] == TYPE_TEXT and c["left"][lk]["type"] != c["right"][rk]["type"] and "expected" not in c
            continue
        want, _, _ = plain_join(c["left"], c["right"], lk, rk, c["kind"])
        assert c["expected"] == want, c["name"]


def test_join_validation_on_host_arguments_needs_no_gpu():
    key = capi.Column.from_list([3, 1, 2], "int64")
    fkey = capi.Column.from_list([3.0, 1.0, 2.0], "float64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    boolean = capi.Column.from_list([True, False, True], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)
    short = capi.Column.from_list([1.0, 2.0], "float64")

    def outs(k, slots=8):
        return [capi.OutColumn(slots) for _ in range(k)]

    o = outs(3)
    for kind in KINDS.values():
        # key types that differ: the reference's text up to the column name
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join([key, val], 0, [fkey, val], 0, kind, outs=o))
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join_rows(key, fkey, kind, count_only=True))
        # Boolean / String anywhere, as a key too
        for bad in (boolean, string):
            raises(ERR_UNSUPPORTED, lambda: capi.join([key, bad], 0, [key, val], 0, kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join([key, val], 0, [key, bad], 0, kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join([bad, val], 0, [key, val], 0, kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join_rows(bad, key, kind, count_only=True))
            raises(ERR_UNSUPPORTED, lambda: capi.join_rows(key, bad, kind, count_only=True))
        # unequal lengths within a frame
        raises(ERR_ARG, lambda: capi.join([key, short], 0, [key, val], 0, kind, outs=o))
        raises(ERR_ARG, lambda: capi.join([key, val], 0, [key, short], 0, kind, outs=o))
        # a key index outside its frame; one side keyed and the other not
        for lk, rk in ((2, 0), (0, 2), (-2, 0), (0, -1), (-1, 0), (5, 5)):
            raises(ERR_BAD_COL, lambda: capi.join([key, val], lk, [key, val], rk, kind, outs=o))
        # 2^31 rows on a side: the limit is named (nothing is read: the column claims a length it does not have)
        huge = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 31, 0)
        assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.join([huge], 0, [key, val], 0, kind, outs=o[:2]))
        assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.join_rows(key, huge, kind, count_only=True))
    half = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 30, 0)
    assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.join([half], -1, [half], -1, capi.JOIN_OUTER, outs=o[:2]))
    # an unknown kind; null arguments; outputs with an unknown residency or without a buffer
    raises(ERR_ARG, lambda: capi.join([key, val], 0, [key, val], 0, 2, outs=o))
    raises(ERR_ARG, lambda: capi.join_rows(key, key, 7, count_only=True))
    rows = C.c_int64(0)
    la, ra = capi._cols([key, val]), capi._cols([key, val])
    oarr = (capi.Out * 3)(*[x.c() for x in o])
    L = capi.lib()
    assert L.bowgpu_join(la, 2, 0, ra, 2, 0, 0, oarr, None) == ERR_ARG
    assert L.bowgpu_join(None, 2, 0, ra, 2, 0, 0, oarr, C.byref(rows)) == ERR_ARG
    assert L.bowgpu_join(la, 2, 0, ra, 2, 0, 0, None, C.byref(rows)) == ERR_ARG
    for spoil in ("values", "residency"):
        oarr = (capi.Out * 3)(*[x.c() for x in o])
        if spoil == "values":
            oarr[2].values = None
        else:
            oarr[2].residency = 9
        assert L.bowgpu_join(la, 2, 0, ra, 2, 0, 1, oarr, C.byref(rows)) == ERR_ARG, spoil
    k = key.c()
    pairs, buf = C.c_int64(0), np.zeros(8, np.int64)
    assert L.bowgpu_join_rows(C.byref(k), C.byref(k), 0, None, None, C.c_int64(0), 0, None, C.byref(pairs)) == ERR_ARG
    assert L.bowgpu_join_rows(C.byref(k), C.byref(k), 0, buf.ctypes.data_as(C.c_void_p), None, C.c_int64(8), 0, C.byref(rows), C.byref(pairs)) == ERR_ARG
    assert untouched(o)


def test_capacity_too_small_where_the_count_needs_no_device():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    # OuterJoin with an empty side: 3 rows; without a common column: 3 + 3
    for left, lk, right, rk, need in (([key, val], 0, none, 0, 3), (none, 0, [key, val], 0, 3), ([key, val], -1, [key, val], -1, 6)):
        n_outs = 4 if lk < 0 else 3
        o = [capi.OutColumn(need) for _ in range(n_outs - 1)] + [capi.OutColumn(need - 1)]
        assert "%d needed" % need in raises(ERR_ARG, lambda: capi.join(left, lk, right, rk, capi.JOIN_OUTER, outs=o))
        assert untouched(o)
    # the index buffers of bowgpu_join_rows
    k, e = key.c(), none[0].c()
    rows, pairs = C.c_int64(0), C.c_int64(0)
    li, ri = np.full(3, -7, np.int64), np.full(3, -7, np.int64)
    rc = capi.lib().bowgpu_join_rows(C.byref(k), C.byref(e), 1, li.ctypes.data_as(C.c_void_p), ri.ctypes.data_as(C.c_void_p), C.c_int64(2), 0,
                                     C.byref(rows), C.byref(pairs))
    assert rc == ERR_ARG and b"3 needed" in capi.lib().bowgpu_last_error()
    assert (li == -7).all() and (ri == -7).all()


def test_joins_without_rows_need_no_device():
    key = capi.Column.from_list([3, 1, 2], "int64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    nullable = [capi.Column(np.zeros(0, np.int64), np.zeros(1, np.uint8), capi.INT64, 0, 0, -1), capi.Column.from_list([], "float64")]

    def empty(outs, types):
        assert [(o.length, o.null_count, o.type) for o in outs] == [(0, 0, t) for t in types]
        assert all((o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)

    i64, f64 = capi.INT64, capi.FLOAT64
    for kind in KINDS.values():      # both sides empty
        for left, right in ((none, none), (nullable, none), (none, nullable)):
            outs, rows = capi.join(left, 0, right, 0, kind, capacity=4)
            assert rows == 0
            empty(outs, [i64, f64, f64])
            assert capi.join_rows(left[0], right[0], kind, count_only=True)[2:] == (0, 0)
            assert capi.join_rows(left[0], right[0], kind)[2:] == (0, 0)
    for left, right in (([key, val], none), (none, [key, val])):      # InnerJoin with one side empty
        outs, rows = capi.join(left, 0, right, 0, capi.JOIN_INNER, capacity=4)
        assert rows == 0
        empty(outs, [i64, f64, f64])
        assert capi.join_rows(left[0], right[0], capi.JOIN_INNER)[2:] == (0, 0)
        # ... and the COUNT of the OuterJoin: the other side's rows, no pair
        assert capi.join_rows(left[0], right[0], capi.JOIN_OUTER, count_only=True)[2:] == (3, 0)
    outs, rows = capi.join([key, val], -1, [key, val], -1, capi.JOIN_INNER, capacity=2)      # no common column
    assert rows == 0
    empty(outs, [i64, f64, i64, f64])
    assert capi.join_rows(None, None, capi.JOIN_OUTER, count_only=True)[2:] == (0, 0)
    for kind in (capi.JOIN_INNER, capi.JOIN_OUTER):      # one key alone: declined, not the rows of the side that is given
        assert "NULL" in raises(ERR_ARG, lambda: capi.join_rows(key, None, kind, count_only=True))
        assert "NULL" in raises(ERR_ARG, lambda: capi.join_rows(None, key, kind, count_only=True))
    # the fixture's cases that look at no row
    for c in vectors()["cases"]:
        if "declined" in c:
            continue
        left, right = case_cols(c["left"]), case_cols(c["right"])
        nl = len(c["left"][0]["data"]) if c["left"] else 0
        nr = len(c["right"][0]["data"]) if c["right"] else 0
        n_outs = len(left) + len(right) - (1 if c["left_key"] >= 0 else 0)
        if "error" in c:
            o = [capi.OutColumn(nl + nr) for _ in range(n_outs)]
            assert c["error"] in raises(ERR_TYPE, lambda: capi.join(left, c["left_key"], right, c["right_key"], KINDS[c["kind"]], outs=o))
            assert untouched(o)
        elif c["kind"] == "inner" and c["left_key"] < 0 or nl + nr == 0:
            outs, rows = capi.join(left, c["left_key"], right, c["right_key"], KINDS[c["kind"]], capacity=2)
            assert rows == 0 and [o.length for o in outs] == [0] * n_outs == [len(e["data"]) for e in c["expected"]]
            assert [o.type for o in outs] == [capi.TYPE_NAMES[e["type"]] for e in c["expected"]]


def test_no_cpu_fallback_without_gpu():
    """valid calls with rows to look at or to move: served where there is a GPU, BOWGPU_ERR_NO_DEVICE where there is none"""
    key = capi.Column.from_list([10, 16, 15, 16], "int64")
    val = capi.Column.from_list([1.0, None, 3.0, 4.5], "float64")
    rkey = capi.Column.from_list([16, 11, 16], "int64")
    rval = capi.Column.from_list([7.0, 8.0, None], "float64")
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    calls = ((lambda: capi.join([key, val], 0, [rkey, rval], 0, capi.JOIN_INNER)[1], 4),
             (lambda: capi.join([key, val], 0, [rkey, rval], 0, capi.JOIN_OUTER)[1], 7),
             (lambda: capi.join_rows(key, rkey, capi.JOIN_OUTER, count_only=True)[2:], (7, 4)),
             (lambda: capi.join_rows(key, rkey, capi.JOIN_INNER)[0].tolist(), [1, 1, 3, 3]),
             (lambda: capi.join([key, val], 0, none, 0, capi.JOIN_OUTER)[0][2].null_count, 4),      # the other side's rows padded with nulls: the gather
             (lambda: capi.join([key, val], -1, [rkey, rval], -1, capi.JOIN_OUTER)[1], 7))
    if _gpu_count() > 0:
        for call, want in calls:
            assert call() == want
        return
    for call, _ in calls:
        raises(ERR_NO_DEVICE, call)
