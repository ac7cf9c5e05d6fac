"""The numpy model of Bow.Convert (tests/convert_model.py) proved without a GPU, in three ways: element by element against Python's own
arithmetic (math.trunc, the correctly rounded float(int), x != 0); by coverage of the seeded fuzz cases tests/test_gpu_convert_fuzz.py
runs by default (every pair, every special value in a valid row and in a null row, every offset class); and by deliberately wrong
variants of the model that those cases must notice."""
import math
import struct

import numpy as np
import pytest

import convert_model as cm
from convert_model import B, F, I

DEFAULT_SEEDS = range(64)   # test_gpu_convert_fuzz.SEEDS without BOW_FUZZ_SEEDS


def python_convert(x, from_t, to_t):
    """one valid value by Python's own arithmetic; Float64 values travel as their bits"""
    if from_t == to_t:
        return x
    if from_t == I:
        return struct.unpack("<Q", struct.pack("<d", float(x)))[0] if to_t == F else x != 0   # float(int) is correctly rounded (nearest even)
    if from_t == F:
        v = struct.unpack("<d", struct.pack("<Q", x))[0]
        if to_t == B:
            return v != 0      # NaN != 0 is True, -0.0 != 0 is False
        if v != v or v in (math.inf, -math.inf):
            return cm.INT64_MIN
        t = math.trunc(v)      # an exact Python int
        return t if cm.INT64_MIN <= t <= cm.INT64_MAX else cm.INT64_MIN
    if to_t == I:
        return 1 if x else 0
    return struct.unpack("<Q", struct.pack("<d", 1.0 if x else 0.0))[0]


def as_python(arr, typ):
    if typ == F:
        return [int(b) for b in np.ascontiguousarray(arr).view(np.uint64)]
    return [bool(b) for b in arr] if typ == B else [int(b) for b in arr]


@pytest.mark.parametrize("from_t,to_t", cm.PAIRS, ids=["%s-%s" % (cm.NAMES[a], cm.NAMES[b]) for a, b in cm.PAIRS])
def test_model_equals_python_arithmetic(from_t, to_t):
    rng = np.random.default_rng(from_t * 10 + to_t)
    parts = [cm.specials(from_t)]
    while sum(len(p) for p in parts) < 10_000 + len(parts[0]):
        parts.append(cm.random_slots(rng, from_t, 2500))
    slots = np.concatenate(parts)
    got = as_python(cm.convert_slots(slots, from_t, to_t), to_t)
    want = [python_convert(x, from_t, to_t) for x in as_python(slots, from_t)]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:5], [(as_python(slots, from_t)[i], got[i], want[i]) for i in bad[:5]])


def test_the_values_the_issue_names():
    f = cm.float_specials()
    want = [0, 0, 0, 0, 0, 0, -1, 0, 2 ** 52, 2 ** 53, 2 ** 63 - 1024, cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MIN,
            cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MIN]
    assert [int(x) for x in cm.float_to_int(f)] == want
    assert [bool(x) for x in cm.float_to_bool(f)] == [False, False] + [True] * 18
    i = cm.int_specials()
    assert [float(x) for x in cm.int_to_float(i)] == [0.0, 1.0, -1.0, 2.0 ** 53, 2.0 ** 53 + 4, -(2.0 ** 53 + 4), 2.0 ** 54, 2.0 ** 54 + 8, 2.0 ** 63, -2.0 ** 63]
    # round toward zero differs at 2^53 + 3 and 2^63 - 1, and not at 2^53 + 1
    rtz = cm.int_to_float(i, "rtz")
    assert [float(x) for x in rtz] == [0.0, 1.0, -1.0, 2.0 ** 53, 2.0 ** 53 + 2, -(2.0 ** 53 + 2), 2.0 ** 54, 2.0 ** 54 + 4, 2.0 ** 63 - 1024, -2.0 ** 63]
    # a same-type conversion keeps a NaN's payload
    assert np.array_equal(cm.convert_slots(f, F, F).view(np.uint64), f.view(np.uint64))


def test_expected_column_zeroes_null_slots_and_padding():
    slots = np.array([cm._f(cm.QNAN), 2.5, -0.0, 7.0, 1e30], np.float64)
    valid = np.array([False, True, True, False, True])
    e = cm.Expected(slots, valid, F, I)
    assert [int(x) for x in e.values.view(np.int64)] == [0, 2, 0, 0, cm.INT64_MIN] and e.null_count == 2
    assert list(e.validity) == [0b10110]
    e = cm.Expected(slots, valid, F, B)
    assert list(e.values) == [0b10010] and list(e.validity) == [0b10110]
    e = cm.Expected(slots, None, F, B)
    assert list(e.values) == [0b11011] and list(e.validity) == [0b11111] and e.null_count == 0
    assert list(cm.Expected(np.array([True, False, True]), np.array([True, True, False]), B, F).values.view(np.float64)) == [1.0, 0.0, 0.0]


def test_make_column_hides_nothing():
    slots = np.array([5, 0, -3], np.int64)
    col = cm.make_column(I, slots, np.array([True, False, True]), offset=13, null_count=1)
    assert (col.offset, col.length, col.null_count) == (13, 3, 1)
    assert list(col.values[13:16]) == [5, 0, -3] and col.values[12] == cm.GARBAGE[I] and col.values[16] == cm.GARBAGE[I]
    bits = np.unpackbits(col.validity, bitorder="little")
    assert list(bits[13:16]) == [1, 0, 1] and bits[:13].all() and bits[16:21].all()
    col = cm.make_column(B, np.array([True, False]), None, offset=7)
    assert col.null_count == 0 and list(np.unpackbits(col.values, bitorder="little")[7:9]) == [1, 0]


@pytest.fixture(scope="module")
def seeded():
    return [cm.fuzz_case(s) for s in DEFAULT_SEEDS]


def test_seeded_cases_cover_the_ground(seeded):
    pairs, offsets, out_res, in_res, nulls, ncols = set(), set(), set(), set(), set(), set()
    valid_seen = {t: set() for t in cm.TYPES}
    null_seen = {t: set() for t in cm.TYPES}
    lengths = set()
    for cols, res in seeded:
        out_res.add(res)
        ncols.add(len(cols))
        for c in cols:
            pairs.add((c.from_t, c.to_t))
            offsets.add(c.offset)
            in_res.add(c.residency)
            lengths.add(len(c.slots))
            nulls.add("none" if c.valid is None else "all" if not c.valid.any() else "some")
            nulls.add("counted" if c.null_count < 0 else "given")
            valid = np.ones(len(c.slots), bool) if c.valid is None else c.valid
            key = as_python(c.slots, c.from_t)
            for row in np.flatnonzero(valid):
                valid_seen[c.from_t].add((c.to_t, key[row]))
            for row in c.null_rows_special:
                assert not c.valid[row]
                null_seen[c.from_t].add((c.to_t, key[row]))
    assert pairs == set(cm.PAIRS)
    assert set(cm.OFFSETS) <= offsets and any(o not in cm.OFFSETS for o in offsets)
    assert out_res == in_res == {0, 1, 2}
    assert nulls == {"none", "all", "some", "counted", "given"}
    assert 9 in ncols and 1 in ncols and any(4 < k for k in ncols)
    assert {0, 1, 63, 64, 65, 511, 512, 513} <= lengths and max(lengths) > 60_000
    for from_t, to_t in cm.PAIRS:   # every special value of the source type, in a valid row and in a null row, for every pair
        want = set(as_python(cm.specials(from_t), from_t))
        assert want <= {k for t, k in valid_seen[from_t] if t == to_t}, (from_t, to_t, "valid")
        assert want <= {k for t, k in null_seen[from_t] if t == to_t}, (from_t, to_t, "null")


@pytest.mark.parametrize("variant", cm.VARIANTS)
def test_seeded_cases_notice_a_wrong_model(seeded, variant):
    noticed = 0
    for cols, _ in seeded:
        for c in cols:
            noticed += not c.expected().same_as(c.expected(variant))
    assert noticed >= 3, variant


def test_variants_are_wrong_where_the_issue_says():
    f = cm.float_specials()
    assert [int(x) for x in cm.float_to_int(f, "saturate")][11:17] == [cm.INT64_MAX, cm.INT64_MIN, cm.INT64_MIN, cm.INT64_MAX, cm.INT64_MAX, cm.INT64_MIN]
    assert int(cm.float_to_int(f, "saturate")[17]) == 0                         # NaN
    assert not cm.float_to_bool(f, "nan_false")[17:].any() and cm.float_to_bool(f, "nan_false")[2:17].all()
    assert cm.float_to_bool(f, "negzero_true")[1] and not cm.float_to_bool(f, "negzero_true")[0]
    leak = cm.Expected(np.array([3, 4], np.int64), np.array([True, False]), I, I, "leak")
    assert list(leak.values) == [3, 4]
    pad = cm.Expected(np.array([True]), None, B, B, "padding")
    assert list(pad.values) == [0xFF] and list(pad.validity) == [0xFF]
