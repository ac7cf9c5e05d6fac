"""The join on several common columns (bowgpu_join_keys / bowgpu_join_keys_rows) without a GPU: the fixture of the five reference cases
with two common columns is well formed, the model of tests/join_keys_model.py - which judges the device in tests/test_gpu_join_keys.py -
equals a literal nested-loop restatement of getCommonRows (bowjoin.go:161-186) plus the fills on seeded frames and reproduces both
fixtures, and everything the two entry points decide about host-resident arguments before they touch the device is answered on a box
that has none, with the outputs untouched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import join_keys_model as model
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0x5A5A5A5A5A5A5A5A
ERR_BAD_COL, ERR_TYPE, ERR_UNSUPPORTED, ERR_ARG, ERR_NO_DEVICE = -6, -7, -9, -10, -11
INNER, OUTER = capi.JOIN_INNER, capi.JOIN_OUTER
KINDS = {"inner": INNER, "outer": OUTER}
TYPE_TEXT = "left and right bow on join columns are of incompatible types"
FIVE = ["outer left and right without rows", "outer left and right bow without rows", "outer with two common columns", "outer advanced",
        "inner simple"]


def load(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def untouched(outs):
    return all(o.null_count == -1 and o.type == 0 and (o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)


def raises(code, call):
    with pytest.raises(capi.BowGpuError) as e:
        call()
    assert e.value.code == code, e.value.message
    return e.value.message


def model_frame(left, lks, right, rks, kind):
    """the model's answer as the fixture writes a frame"""
    li, ri, pairs = model.join_rows(left, lks, right, rks, kind)
    return model.to_lists(model.expected_columns(left, lks, right, rks, li, ri)), li, ri, pairs


# ------------------------------------------------------------------ the fixture
def test_fixture_is_well_formed_and_the_model_gives_its_expected_frames():
    doc = load("join_keys_vectors.json")
    assert "bowjoin_test.go" in doc["source"]
    for word in ("Data only", "nil", "left_keys", "expected_swapped", "String", "metadata"):
        assert word in doc["note"]
    assert [c["name"] for c in doc["cases"]] == FIVE
    declined = {c["name"]: c for c in load("join_vectors.json")["cases"] if "declined" in c}
    assert sorted(declined) == sorted(FIVE)
    for c in doc["cases"]:
        old = declined[c["name"]]      # the same inputs join_vectors.json records, now with keys and the expected frame
        assert (c["kind"], c["source"], c["left"], c["right"]) == (old["kind"], old["source"], old["left"], old["right"])
        assert c["kind"] in KINDS and c["source"].startswith("bowjoin_test.go:")
        lnames, rnames = [x["name"] for x in c["left"]], [x["name"] for x in c["right"]]
        common = [n for n in lnames if n in rnames]
        assert len(common) == 2      # exactly two common names, found in the left frame's order (getCommonCols)
        assert c["left_keys"] == [lnames.index(n) for n in common] and c["right_keys"] == [rnames.index(n) for n in common]
        for frame in (c["left"], c["right"], c["expected"]):
            assert len({len(col["data"]) for col in frame}) == 1
            assert all(col["type"] in ("int64", "float64") for col in frame)
        assert [e["name"] for e in c["expected"]] == lnames + [n for n in rnames if n not in common]
        assert [e["type"] for e in c["expected"]] == [x["type"] for x in c["left"]] + [x["type"] for x in c["right"] if x["name"] not in common]
        left, right = model.case_frame(c["left"]), model.case_frame(c["right"])
        got, _, _, _ = model_frame(left, c["left_keys"], right, c["right_keys"], KINDS[c["kind"]])
        assert repr(got) == repr([e["data"] for e in c["expected"]]), c["name"]
        if "expected_swapped" in c:
            got, _, _, _ = model_frame(right, c["right_keys"], left, c["left_keys"], KINDS[c["kind"]])
            assert repr(got) == repr([e["data"] for e in c["expected_swapped"]]), c["name"]
    adv = next(c for c in doc["cases"] if c["name"] == "outer advanced")
    assert adv["left_keys"] != adv["right_keys"]      # keys at different positions in the two frames
    assert [col["data"][1] for col in adv["expected"]] == [None] * 7      # the all-nil rows pair up: one row, not two


def test_with_one_key_the_model_reproduces_the_one_key_fixture():
    ran = 0
    for c in load("join_vectors.json")["cases"]:
        if "expected" not in c:
            continue
        lks, rks = ([c["left_key"]], [c["right_key"]]) if c["left_key"] >= 0 else ([], [])
        got, _, _, _ = model_frame(model.case_frame(c["left"]), lks, model.case_frame(c["right"]), rks, KINDS[c["kind"]])
        assert repr(got) == repr([e["data"] for e in c["expected"]]), c["name"]
        ran += 1
    assert ran == 12


# ------------------------------------------------------------------ the model against the reference's loops
def brute_join(left, lks, right, rks, kind):
    """bowjoin.go:161-186 as it stands - the double loop, a pair common when it agrees on every common column - then the fills; frames
    are lists of python lists, None for nil"""
    nl, nr = len(left[0]), len(right[0])
    pairs = []
    for l in range(nl):
        for r in range(nr):
            is_common = True
            for lk, rk in zip(lks, rks):
                if left[lk][l] != right[rk][r]:
                    is_common = False
                    break
            if is_common:
                pairs.append((l, r))
    out_rows = list(pairs)
    if kind == OUTER:
        out_rows = []
        for l in range(nl):
            mine = [p for p in pairs if p[0] == l]
            out_rows += mine if mine else [(l, -1)]
        hit = {r for _, r in pairs}
        out_rows += [(-1, r) for r in range(nr) if r not in hit]
    cols = []
    for i, c in enumerate(left):
        own = right[rks[lks.index(i)]] if i in lks else None      # a key column's own right partner
        cols.append([c[l] if l >= 0 else (own[r] if own is not None else None) for l, r in out_rows])
    for i, c in enumerate(right):
        if i not in rks:
            cols.append([c[r] if r >= 0 else None for _, r in out_rows])
    return cols, out_rows, len(pairs)


def seeded_frames(seed):
    """two frames of at most 40 rows, 1 to 3 key pairs at shuffled positions, key values from small ranges (tuples agree on one key and
    differ on another), nulls in any subset of the keys, -0.0 / +0.0 among the float keys"""
    rng = np.random.default_rng(seed)
    n_keys = 1 + seed % 3
    nl, nr = int(rng.integers(0, 41)), int(rng.integers(0, 41))
    ncl, ncr = n_keys + int(rng.integers(0, 3)), n_keys + int(rng.integers(0, 3))
    lks, rks = rng.permutation(ncl)[:n_keys].tolist(), rng.permutation(ncr)[:n_keys].tolist()
    key_float = [bool(rng.integers(0, 2)) for _ in range(n_keys)]
    p_null = [0.0, 0.15, 0.5][(seed // 3) % 3]      # every key count meets every null rate

    def column(n, as_float, key):
        if as_float:
            vals = rng.choice(np.array([-0.0, 0.0, 1.5, -2.0] if key else [-0.0, 0.0, 1.5, -2.0, 7.25, 1e300]), n)
        else:
            vals = rng.integers(-1, 3 if key else 1000, n)
        valid = rng.random(n) >= p_null
        return model.ModelCol(vals.astype(np.float64 if as_float else np.int64), None if valid.all() else valid)

    def frame(n, ncols, keys):
        return [column(n, key_float[keys.index(i)], True) if i in keys else column(n, bool(rng.integers(0, 2)), False) for i in range(ncols)]

    return frame(nl, ncl, lks), lks, frame(nr, ncr, rks), rks


def as_lists(frame):
    return [[x if ok else None for x, ok in zip(c.values.tolist(), model.valid_of(c).tolist())] for c in frame]


def test_the_model_equals_the_nested_loops_on_seeded_frames():
    seen_keys, both, some_match_one_key_only = set(), 0, 0
    for seed in range(240):
        left, lks, right, rks = seeded_frames(seed)
        seen_keys.add(len(lks))
        for kind in (INNER, OUTER):
            got, li, ri, pairs = model_frame(left, lks, right, rks, kind)
            want, out_rows, n_pairs = brute_join(as_lists(left), lks, as_lists(right), rks, kind)
            assert repr(got) == repr(want), seed      # repr: -0.0 and 0.0 are told apart - a key column keeps the LEFT row's zero
            assert list(zip(li.tolist(), ri.tolist())) == out_rows and pairs == n_pairs, seed
        if len(lks) >= 2:
            both += pairs > 0
            some_match_one_key_only += model.join_rows(left, lks[:1], right, rks[:1], INNER)[2] > pairs
    assert seen_keys == {1, 2, 3} and both > 40 and some_match_one_key_only > 40      # the frames are no empty exercise


# ------------------------------------------------------------------ what needs no device
def test_validation_on_host_arguments_needs_no_gpu():
    key = capi.Column.from_list([3, 1, 2], "int64")
    key2 = capi.Column.from_list([7, 7, 8], "int64")
    fkey = capi.Column.from_list([3.0, 1.0, 2.0], "float64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    boolean = capi.Column.from_list([True, False, True], "bool")
    string = capi.Column(np.zeros(3, np.uint8), None, capi.STRING, 0, 3, 0)
    short = capi.Column.from_list([1, 2], "int64")
    o = [capi.OutColumn(8) for _ in range(4)]
    frame = [key, key2, val]
    L = capi.lib()
    rows, pairs = C.c_int64(0), C.c_int64(0)
    la, ra = capi._cols(frame), capi._cols(frame)
    k01 = (C.c_int32 * 9)(0, 1, 2, 0, 1, 2, 0, 1, 2)
    oarr = (capi.Out * 4)(*[x.c() for x in o])
    for kind in KINDS.values():
        # n_keys < 0; more than BOWGPU_JOIN_MAX_KEYS, naming the limit
        assert L.bowgpu_join_keys(la, 3, k01, ra, 3, k01, -1, kind, oarr, C.byref(rows)) == ERR_ARG
        assert L.bowgpu_join_keys(la, 3, k01, ra, 3, k01, 9, kind, oarr, C.byref(rows)) == ERR_UNSUPPORTED
        assert b"BOWGPU_JOIN_MAX_KEYS = 8" in L.bowgpu_last_error()
        assert L.bowgpu_join_keys_rows(la, ra, -1, kind, None, None, C.c_int64(0), 0, C.byref(rows), C.byref(pairs)) == ERR_ARG
        assert L.bowgpu_join_keys_rows(la, ra, 9, kind, None, None, C.c_int64(0), 0, C.byref(rows), C.byref(pairs)) == ERR_UNSUPPORTED
        assert b"BOWGPU_JOIN_MAX_KEYS = 8" in L.bowgpu_last_error()
        # a key index outside its frame, in either key pair, with one key and with two
        for lks, rks in (([0, 3], [0, 1]), ([0, 1], [0, 3]), ([-1, 1], [0, 1]), ([0, 1], [1, -1]), ([3], [0]), ([0], [-1]), ([-1], [-1])):
            raises(ERR_BAD_COL, lambda: capi.join_keys(frame, lks, frame, rks, kind, outs=o))
        # a column listed twice among one side's keys
        assert "twice" in raises(ERR_ARG, lambda: capi.join_keys(frame, [0, 0], frame, [0, 1], kind, outs=o))
        assert "twice" in raises(ERR_ARG, lambda: capi.join_keys(frame, [0, 1], frame, [1, 1], kind, outs=o))
        # key pair types that differ: the one-key join's text, for any key pair and for one key alone
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join_keys(frame, [0, 1], [key, fkey, val], [0, 1], kind, outs=o))
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join_keys([fkey, key2, val], [0, 1], frame, [0, 1], kind, outs=o))
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join_keys(frame, [0], [fkey, val], [0], kind, outs=o[:3]))
        assert TYPE_TEXT in raises(ERR_TYPE, lambda: capi.join_keys_rows([key, key2], [key, fkey], kind, count_only=True))
        # Boolean / String anywhere, as a key too
        for bad in (boolean, string):
            raises(ERR_UNSUPPORTED, lambda: capi.join_keys([key, key2, bad], [0, 1], frame, [0, 1], kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join_keys(frame, [0, 1], [key, key2, bad], [0, 1], kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join_keys([key, bad, val], [0, 1], [key, bad, val], [0, 1], kind, outs=o))
            raises(ERR_UNSUPPORTED, lambda: capi.join_keys_rows([key, bad], [key, key2], kind, count_only=True))
            raises(ERR_UNSUPPORTED, lambda: capi.join_keys_rows([key, key2], [bad, key2], kind, count_only=True))
        # unequal lengths within a frame / among one side's keys
        raises(ERR_ARG, lambda: capi.join_keys([key, short, val], [0, 1], frame, [0, 1], kind, outs=o))
        raises(ERR_ARG, lambda: capi.join_keys(frame, [0, 1], [key, key2, short], [0, 1], kind, outs=o))
        raises(ERR_ARG, lambda: capi.join_keys_rows([key, short], [key, key2], kind, count_only=True))
        raises(ERR_ARG, lambda: capi.join_keys_rows([key, key2], [short, key2], kind, count_only=True))
        # row limits, named: 2^31 rows on a side, and L + R of 2^31 with two keys (nothing is read: the columns claim the length)
        huge = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 31, 0)
        half = capi.Column(np.zeros(1, np.int64), None, capi.INT64, 0, 1 << 30, 0)
        assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.join_keys([huge, huge], [0, 1], [key, key2], [0, 1], kind, outs=o[:2]))
        assert "2^31" in raises(ERR_UNSUPPORTED, lambda: capi.join_keys_rows([key, key2], [huge, huge], kind, count_only=True))
        msg = raises(ERR_UNSUPPORTED, lambda: capi.join_keys([half, half], [0, 1], [half, half], [0, 1], kind, outs=o[:2]))
        assert "2^31" in msg and "together" in msg
        msg = raises(ERR_UNSUPPORTED, lambda: capi.join_keys_rows([half, half], [half, half], kind, count_only=True))
        assert "2^31" in msg and "together" in msg
    # an unknown kind; null arguments; outputs with an unknown residency or without a buffer
    raises(ERR_ARG, lambda: capi.join_keys(frame, [0, 1], frame, [0, 1], 2, outs=o))
    raises(ERR_ARG, lambda: capi.join_keys_rows([key, key2], [key, key2], 7, count_only=True))
    assert L.bowgpu_join_keys(la, 3, k01, ra, 3, k01, 2, 0, oarr, None) == ERR_ARG
    assert L.bowgpu_join_keys(la, 3, None, ra, 3, k01, 2, 0, oarr, C.byref(rows)) == ERR_ARG
    assert L.bowgpu_join_keys(la, 3, k01, ra, 3, None, 2, 0, oarr, C.byref(rows)) == ERR_ARG
    assert L.bowgpu_join_keys(None, 3, k01, ra, 3, k01, 2, 0, oarr, C.byref(rows)) == ERR_ARG
    assert L.bowgpu_join_keys(la, 3, k01, ra, 3, k01, 2, 0, None, C.byref(rows)) == ERR_ARG
    assert L.bowgpu_join_keys_rows(None, ra, 2, 0, None, None, C.c_int64(0), 0, C.byref(rows), C.byref(pairs)) == ERR_ARG
    assert L.bowgpu_join_keys_rows(la, ra, 2, 0, None, None, C.c_int64(0), 0, None, C.byref(pairs)) == ERR_ARG
    buf = np.full(8, -7, np.int64)
    assert L.bowgpu_join_keys_rows(la, ra, 2, 0, buf.ctypes.data_as(C.c_void_p), None, C.c_int64(8), 0, C.byref(rows), C.byref(pairs)) == ERR_ARG
    assert (buf == -7).all()
    for spoil in ("values", "residency"):
        oarr = (capi.Out * 4)(*[x.c() for x in o])
        if spoil == "values":
            oarr[3].values = None
        else:
            oarr[3].residency = 9
        assert L.bowgpu_join_keys(la, 3, k01, ra, 3, k01, 2, 1, oarr, C.byref(rows)) == ERR_ARG, spoil
    assert untouched(o)


def test_joins_without_rows_need_no_device():
    key, key2 = capi.Column.from_list([3, 1, 2], "int64"), capi.Column.from_list([1.5, None, 1.5], "float64")
    val = capi.Column.from_list([1.0, None, 3.0], "float64")
    full = [key, key2, val]
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64"), capi.Column.from_list([], "float64")]
    i64, f64 = capi.INT64, capi.FLOAT64

    def empty(outs, types):
        assert [(o.length, o.null_count, o.type) for o in outs] == [(0, 0, t) for t in types]
        assert all((o.values == POISON).all() and (o.validity == 0xA5).all() for o in outs)

    for kind in KINDS.values():      # both frames empty
        outs, rows = capi.join_keys(none, [0, 1], none, [0, 1], kind, capacity=4)
        assert rows == 0
        empty(outs, [i64, f64, f64, f64])
        assert capi.join_keys_rows(none[:2], none[:2], kind, count_only=True)[2:] == (0, 0)
        assert capi.join_keys_rows(none[:2], none[:2], kind)[2:] == (0, 0)
    for left, right in ((full, none), (none, full)):      # InnerJoin with one side empty; the COUNT of the OuterJoin
        outs, rows = capi.join_keys(left, [0, 1], right, [0, 1], INNER, capacity=4)
        assert rows == 0
        empty(outs, [i64, f64, f64, f64])
        assert capi.join_keys_rows(left[:2], right[:2], INNER)[2:] == (0, 0)
        assert capi.join_keys_rows(left[:2], right[:2], OUTER, count_only=True)[2:] == (3, 0)
        # ... whose outputs, one slot short, are declined naming the size, untouched
        o = [capi.OutColumn(3) for _ in range(3)] + [capi.OutColumn(2)]
        assert "3 needed" in raises(ERR_ARG, lambda: capi.join_keys(left, [0, 1], right, [0, 1], OUTER, outs=o))
        assert untouched(o)
    # no key: exactly the -1 / -1 join
    outs, rows = capi.join_keys(full[:2], [], full[1:], [], INNER, capacity=2)
    assert rows == 0
    empty(outs, [i64, f64, f64, f64])
    assert capi.join_keys_rows([], [], OUTER, count_only=True)[2:] == (0, 0)
    # the fixture's case without any row
    c = next(c for c in load("join_keys_vectors.json")["cases"] if c["name"] == "outer left and right bow without rows")
    left = [capi.Column.from_list(x["data"], x["type"]) for x in c["left"]]
    right = [capi.Column.from_list(x["data"], x["type"]) for x in c["right"]]
    outs, rows = capi.join_keys(left, c["left_keys"], right, c["right_keys"], OUTER, capacity=2)
    assert rows == 0 and [o.type for o in outs] == [capi.TYPE_NAMES[e["type"]] for e in c["expected"]] and [o.length for o in outs] == [0] * 4


def test_symbols_are_exported_and_listed():
    L = capi.lib()
    for name in ("bowgpu_join_keys_rows", "bowgpu_join_keys"):
        assert hasattr(L, name) and name in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    assert "#define BOWGPU_JOIN_MAX_KEYS %d" % capi.JOIN_MAX_KEYS in header and "#define BOWGPU_ABI_VERSION 14" in header


def test_no_cpu_fallback_without_gpu():
    """valid calls on two keys with rows to look at or to move: served where there is a GPU, BOWGPU_ERR_NO_DEVICE where there is none"""
    t, s = capi.Column.from_list([10, 10, 20, 20], "int64"), capi.Column.from_list([1, 2, 1, None], "int64")
    val = capi.Column.from_list([1.0, None, 3.0, 4.5], "float64")
    rt, rs = capi.Column.from_list([20, 10, 20], "int64"), capi.Column.from_list([None, 2, 1], "int64")
    rval = capi.Column.from_list([7.0, 8.0, None], "float64")
    none = [capi.Column.from_list([], "int64"), capi.Column.from_list([], "int64"), capi.Column.from_list([], "float64")]
    calls = ((lambda: capi.join_keys([t, s, val], [0, 1], [rt, rs, rval], [0, 1], INNER)[1], 3),
             (lambda: capi.join_keys([t, s, val], [0, 1], [rt, rs, rval], [0, 1], OUTER)[1], 4),
             (lambda: capi.join_keys_rows([t, s], [rt, rs], OUTER, count_only=True)[2:], (4, 3)),
             (lambda: capi.join_keys_rows([t, s], [rt, rs], INNER)[1].tolist(), [1, 2, 0]),
             (lambda: capi.join_keys([t, s, val], [0, 1], none, [0, 1], OUTER)[0][3].null_count, 4))      # padded with nulls: the gather
    try:
        n_gpu = capi.device_count()
    except capi.BowGpuError:
        n_gpu = 0
    if n_gpu > 0:
        for call, want in calls:
            assert call() == want
        return
    for call, _ in calls:
        raises(ERR_NO_DEVICE, call)
