"""AppendBows and Bow.Find / FindNext / Contains on the device (bowgpu_append / bowgpu_find_next) against numpy concatenation and a
scan in Python, which are exact, and against the fixture of the reference's own tests: every comparison is bit for bit - values as
uint64, validity bytes, null_count, length and type, 0 in the null slots, clear padding bits, and the sentinels of the output buffers
intact past the slots produced (or everywhere, when a call says unchanged or returns an error)."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from bow_amd import capi
from test_gpu_filter import DEVICE, GROUP, HOST, I64_MAX, I64_MIN, PINNED, POISON, T, Col, assert_untouched, make_outs, pack, place, raw, release

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
OFFSETS = [0, 1, 7, 8, 63, 64, 65]
ERR_TYPE, ERR_ARG = -7, -10


# ------------------------------------------------------------------ oracles (numpy: exact) and the comparison
def valid_of(col):
    return np.ones(len(col.values), bool) if col.valid is None else col.valid


def assert_appended(frames, outs, cap):
    """outs against the concatenation of the pieces (lists of Col), column by column"""
    total = sum(len(f[0].values) for f in frames)
    nb = (total + 7) // 8
    assert len(outs) == len(frames[0])
    for i, o in enumerate(outs):
        bits = np.concatenate([f[i].bits() for f in frames])
        valid = np.concatenate([valid_of(f[i]) for f in frames])
        v, b = raw(o, cap)
        assert o.length == total and o.type == frames[0][i].typ and o.null_count == total - int(valid.sum())
        assert np.array_equal(v[:total], np.where(valid, bits, np.uint64(0)))      # raw payloads; null slots hold 0
        assert np.array_equal(b[:nb], pack(valid))                                 # validity; the padding bits of the last byte clear
        assert (v[total:cap] == POISON).all() and (b[nb:] == 0xA5).all()           # nothing past slot total - 1 / byte ceil(total/8) - 1


def place_piece(col, residency):
    """place(), for pieces that may have no row: a registered buffer has at least one element, whatever the piece holds"""
    c = col.column()
    if residency != PINNED or (c.values.size and (c.validity is None or c.validity.size)):
        return place(col, residency)
    vals = capi.page_aligned(len(c.values), c.values.dtype, 0)
    vals[:len(c.values)] = c.values
    bm = None
    if c.validity is not None:
        bm = capi.page_aligned(len(c.validity), np.uint8, 0)
        bm[:len(c.validity)] = c.validity
    return capi.Column(vals, bm, c.type, c.offset, c.length, c.null_count).pin()


def run_append(frames, in_res=HOST, out_res=HOST, cap=None):
    """in_res: one residency, or a function of (piece, column)"""
    total = sum(len(f[0].values) for f in frames)
    cap = total if cap is None else cap
    res = in_res if callable(in_res) else (lambda f, i: in_res)
    placed = [[place_piece(c, res(f, i)) for i, c in enumerate(fr)] for f, fr in enumerate(frames)]
    try:
        outs, unchanged = capi.append(placed, outs=make_outs(len(frames[0]), cap, out_res))
        assert not unchanged
        if total:
            assert_appended(frames, outs, cap)
        else:
            assert [(o.length, o.null_count, o.type) for o in outs] == [(0, 0, c.typ) for c in frames[0]]
            for o in outs:
                v, b = raw(o, cap)
                assert (v == POISON).all() and (b == 0xA5).all()
    finally:
        for fr in placed:
            release(fr)
    return outs


def piece(n, seed, offset=0, known=True, p_null=0.3):
    """two columns: Int64 without a bitmap, Float64 with nulls (random payloads under them)"""
    rng = np.random.default_rng(seed)
    return [Col(rng.integers(I64_MIN, I64_MAX, n)), Col(rng.standard_normal(n), rng.random(n) >= p_null, offset=offset, null_count_known=known)]


def find_want(col, value, start=0):
    valid = valid_of(col)
    if value is None:
        rows = np.flatnonzero(~valid)      # from row 0, whatever `start` says (bowfind.go:12-19)
        return int(rows[0]) if len(rows) else -1
    with np.errstate(invalid="ignore"):
        hit = valid & (col.values == col.values.dtype.type(value))      # IEEE == for float64, exact for int64
    rows = np.flatnonzero(hit[start:])
    return start + int(rows[0]) if len(rows) else -1


def run_find(col, value, start=0, res=HOST, placed=None):
    c = placed if placed is not None else place(col, res)
    try:
        got = capi.find_next(c, value, start)
    finally:
        if placed is None:
            release([c])
    assert got == find_want(col, value, start), (value, start, got)
    return got


# ------------------------------------------------------------------ append
@pytest.mark.parametrize("n0", LENGTHS)
def test_two_and_three_pieces(n0):
    """boundaries inside a word, on a word, on a tile"""
    for k, n1 in enumerate(LENGTHS):
        run_append([piece(n0, 1, offset=3), piece(n1, 2, offset=65, known=bool(k % 2))], DEVICE if k % 3 == 0 else HOST)
    for n1, n2 in ((1, 63), (T - 1, 0), (64, T + 1), (0, 0)):
        run_append([piece(n0, 3), piece(n1, 4, offset=1), piece(n2, 5, offset=7, known=False)])


@pytest.mark.parametrize("in_res", [HOST, DEVICE], ids=["in-host", "in-device"])
def test_many_small_pieces_in_one_word(in_res):
    """300 pieces of 1 to 3 rows: one output word holds bits of more than 20 pieces; empty pieces sprinkled in, first and last included"""
    rng = np.random.default_rng(300)
    frames = []
    for f in range(300):
        n = 0 if f in (0, 299) or f % 17 == 5 else int(rng.integers(1, 4))
        frames.append([Col(rng.integers(-9, 9, n), (rng.random(n) < 0.6) if f % 3 else None, offset=f % 9, null_count_known=bool(f % 2)),
                       Col(rng.standard_normal(n), rng.random(n) < 0.5, offset=f % 5)])
    run_append(frames, in_res, HOST)


@pytest.mark.parametrize("offset", OFFSETS)
def test_source_arrow_offsets(offset):
    """pieces sliced at bit offsets that are no multiple of 8 / 32 / 64, stray bits in front of and behind the slice"""
    frames = [piece(T + 65, 10 + offset, offset=offset), piece(67, 20 + offset, offset=offset, known=False), piece(2 * T - 1, 30, offset=(offset * 5) % 67)]
    run_append(frames)
    run_append(frames, DEVICE, DEVICE)


def test_pieces_with_and_without_a_bitmap_and_null_counts():
    """one column whose pieces have a bitmap or none, null_count stated or -1, all null, all valid"""
    rng = np.random.default_rng(7)
    n = T // 2 + 9

    def col(valid, known=True, offset=0):
        return [Col(rng.integers(I64_MIN, I64_MAX, n), valid, offset=offset, null_count_known=known)]

    frames = [col(None), col(rng.random(n) < 0.5), col(rng.random(n) < 0.5, known=False, offset=5), col(np.zeros(n, bool)),
              col(np.ones(n, bool), known=False), col(np.zeros(n, bool), known=False, offset=63), col(None), col(np.ones(n, bool))]
    for in_res in (HOST, DEVICE, lambda f, i: DEVICE if f % 2 else HOST):
        run_append(frames, in_res)
    # every piece states its nulls: nothing to count; none has nulls to look at: no bitmap is read
    run_append([frames[0], frames[1], frames[3]], DEVICE, DEVICE)
    run_append([frames[0], frames[6], frames[7]], DEVICE, DEVICE)


def test_payloads_survive():
    nan_bits = np.array([0x7FF8DEADBEEF0001, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000,
                         0x8000000000000000, 0, 1, 0x000FFFFFFFFFFFFF], np.uint64)
    flt = nan_bits.view(np.float64)
    ints = np.array([I64_MAX, I64_MIN, -1, 0, 1, I64_MIN + 1, I64_MAX - 1, 42, -42], np.int64)
    valid = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    frames = [[Col(ints), Col(flt, valid)], [Col(ints[::-1].copy(), valid, offset=1), Col(flt[::-1].copy())], [Col(ints[:2].copy()), Col(flt[:2].copy(), valid[:2])]]
    outs = run_append(frames)
    got = outs[1].host_arrays()[0].view(np.uint64)
    assert got[0] == 0x7FF8DEADBEEF0001 and got[5] == 0x8000000000000000 and got[2] == 0      # a NaN's bits, -0.0, a null slot
    run_append(frames, DEVICE, PINNED)


@pytest.mark.parametrize("ncols", [GROUP + 1, 2 * GROUP + 1])
def test_more_columns_than_a_launch_takes(ncols):
    rng = np.random.default_rng(ncols)

    def frame(n, f):
        return [Col(rng.integers(-9, 9, n) if i % 2 else rng.standard_normal(n), (rng.random(n) < 0.8) if (i + f) % 3 else None, offset=i + f,
                    null_count_known=bool((i + f) % 2)) for i in range(ncols)]

    frames = [frame(T + 77, 0), frame(0, 1), frame(65, 2), frame(T - 3, 3)]
    run_append(frames)
    run_append(frames, lambda f, i: (HOST, DEVICE)[(f + i) % 2], DEVICE)


@pytest.mark.parametrize("out_res", [HOST, DEVICE, PINNED], ids=["out-host", "out-device", "out-pinned"])
def test_residencies_mixed_within_one_call(out_res):
    """host, device and pinned pieces of the same column in one call"""
    frames = [piece(n, 40 + k, offset=k, known=bool(k % 2)) for k, n in enumerate((65, T + 1, 0, 63, 2 * T, 1))]
    run_append(frames, lambda f, i: (HOST, DEVICE, PINNED)[(f + i) % 3], out_res)
    for in_res in (HOST, DEVICE, PINNED):
        run_append(frames[:3], in_res, out_res)


def test_piece_boundary_past_2_pow_24_rows_device_resident():
    n0 = (1 << 24) + 5
    rng = np.random.default_rng(24)
    frames = [[Col(rng.standard_normal(n0), rng.random(n0) >= 0.3, offset=1)], [Col(rng.standard_normal(T + 3), rng.random(T + 3) >= 0.3, offset=7, null_count_known=False)]]
    run_append(frames, DEVICE, DEVICE)


@pytest.mark.parametrize("out_res", [HOST, DEVICE], ids=["out-host", "out-device"])
def test_capacity_exact_and_too_small(out_res):
    frames = [piece(T + 1, 1), piece(70, 2)]
    total = T + 71
    run_append(frames, HOST, out_res, cap=total)              # exact
    run_append(frames, HOST, out_res, cap=total + 9)          # spare slots stay as they were
    outs = make_outs(2, total, out_res)
    outs[1] = make_outs(1, total - 1, out_res)[0]
    with pytest.raises(capi.BowGpuError) as e:                # one slot short: the size needed is named and nothing is written
        capi.append([[c.column() for c in f] for f in frames], outs=outs)
    assert e.value.code == ERR_ARG and "%d needed" % total in e.value.message
    assert_untouched(outs[:1], total)
    assert_untouched(outs[1:], total - 1)
    # a type mismatch in the last piece: the reference's text, nothing written
    outs = make_outs(2, total, out_res)
    bad = [frames[0], [frames[1][0], Col(np.arange(70, dtype=np.int64))]]
    with pytest.raises(capi.BowGpuError) as e:
        capi.append([[c.column() for c in f] for f in bad], outs=outs)
    assert e.value.code == ERR_TYPE and "incompatible types 'float64' and 'int64'" in e.value.message
    assert_untouched(outs, total)
    # one piece: the reference returns its argument
    outs, unchanged = capi.append([[c.column() for c in frames[0]]], outs=make_outs(2, total, out_res))
    assert unchanged
    assert_untouched(outs, total)


@pytest.mark.parametrize("cut", [0, 1, 64, T + 5, 2 * T + 16, 2 * T + 17])
def test_split_halves_give_back_the_frame(cut):
    """the two halves of a frame split at an arbitrary row (slices of the same buffers, by Arrow offset)"""
    n = 2 * T + 17
    whole = piece(n, 9, offset=5)
    cols = [c.column().to_device() for c in whole]
    halves = [[capi.Column(c.values, c.validity, c.type, c.offset + lo, hi - lo, -1 if c.validity is not None else 0) for c in cols]
              for lo, hi in ((0, cut), (cut, n))]
    outs, unchanged = capi.append(halves, outs=make_outs(2, n, DEVICE))
    assert not unchanged
    assert_appended([whole], outs, n)


def test_drop_nils_outputs_go_straight_in_as_a_piece():
    a, b = piece(T + 9, 1, known=False), piece(3 * T, 2)
    dropped, first, count, contiguous = capi.drop_nils([place(c, DEVICE) for c in a], outs=make_outs(2, T + 9, DEVICE))
    assert not contiguous
    keep = a[1].valid
    kept = [Col(a[0].values[keep]), Col(a[1].values[keep], np.ones(count, bool))]
    outs, _ = capi.append([[capi.out_as_column(o) for o in dropped], [place(c, DEVICE) for c in b]], outs=make_outs(2, count + 3 * T, DEVICE))
    assert_appended([kept, b], outs, count + 3 * T)


# ------------------------------------------------------------------ find
@pytest.mark.parametrize("n", [1, 64, 65, T, T + 1, 3 * T + 17])
def test_find_target_rows(n):
    rng = np.random.default_rng(n)
    for dt in (np.int64, np.float64):
        for r in sorted({r for r in (0, 63, 64, T - 1, T, n - 1) if r < n}):
            vals = (np.arange(n) * 3 + 1).astype(dt)
            valid = rng.random(n) < 0.8
            valid[r] = True
            col = Col(vals, valid, offset=3, null_count_known=bool(r % 2))
            c = place(col, DEVICE)
            assert run_find(col, vals[r], 0, placed=c) == r
            assert run_find(col, vals[r], r, placed=c) == r
            assert run_find(col, vals[r], r + 1, placed=c) == -1
            assert run_find(col, vals[r] + 1, 0, placed=c) == -1          # absent
            vals[n - 1] = vals[r]                                           # the value once more, in the last row
            col = Col(vals, None)
            assert run_find(col, vals[r], r + 1) == (n - 1 if r + 1 < n else -1)
            assert run_find(col, vals[r], n) == -1 and run_find(col, vals[r], n + 5) == -1      # past the end


def test_find_lowest_of_many_matches():
    n = 5 * T + 3
    assert run_find(Col(np.full(n, 7, np.int64)), 7) == 0                          # every row matches
    assert run_find(Col(np.full(n, 7, np.int64)), 7, 2 * T + 1, DEVICE) == 2 * T + 1
    vals = np.arange(n, dtype=np.int64)
    vals[[70, T + 1, 2 * T, 3 * T + 5, n - 1]] = -5                                # matches in many tiles at once
    valid = np.ones(n, bool)
    valid[70] = False                                                              # a matching value in a NULL slot is not found
    col = Col(vals, valid, offset=1)
    for res in (HOST, DEVICE):
        assert run_find(col, -5, 0, res) == T + 1
        assert run_find(col, -5, T + 2, res) == 2 * T
        assert run_find(col, -5, 3 * T + 6, res) == n - 1
    for _ in range(5):                                                             # the same call gives the same row
        assert run_find(col, -5, 0, DEVICE) == T + 1


def test_find_nil_is_the_first_null_and_ignores_row_start():
    n = 3 * T + 17
    for first in (0, 63, 64, T - 1, T, 2 * T + 70, n - 1):
        valid = np.ones(n, bool)
        valid[first] = False
        valid[first + 1::1000] = False
        for known in (True, False):
            col = Col(np.arange(n, dtype=np.int64), valid, offset=7, null_count_known=known)
            for res in (HOST, DEVICE):
                assert run_find(col, None, 0, res) == first
                assert run_find(col, None, first + 1, res) == first      # row_start is ignored, as the reference ignores it
    # a bitmap without a null: counted by the caller or not
    for known in (True, False):
        assert run_find(Col(np.arange(n, dtype=np.int64), np.ones(n, bool), offset=1, null_count_known=known), None, 0, DEVICE) == -1
    assert run_find(Col(np.arange(n, dtype=np.int64)), None, 0, DEVICE) == -1


def test_find_float_zeros_nan_inf():
    vals = np.array([1.5, -0.0, np.nan, 0.0, np.inf, -np.inf, np.nan, 2.5], np.float64)
    col = Col(vals, np.array([1, 1, 1, 1, 1, 1, 1, 0], bool))
    for res in (HOST, DEVICE):
        assert run_find(col, 0.0, 0, res) == 1 and run_find(col, -0.0, 0, res) == 1      # -0.0 equals +0.0
        assert run_find(col, -0.0, 2, res) == 3
        assert run_find(col, np.inf, 0, res) == 4 and run_find(col, -np.inf, 0, res) == 5
        assert run_find(col, np.nan, 0, res) == -1                                       # a NaN equals nothing
        assert run_find(col, 2.5, 0, res) == -1                                          # under a null
        assert run_find(col, None, 0, res) == 7
    n = T + 70
    wide = np.random.default_rng(2).integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64).copy()      # NaNs of every kind among them
    wide[T + 3] = 6.25
    assert run_find(Col(wide, None, offset=65), 6.25, 0, DEVICE) == find_want(Col(wide), 6.25)


@pytest.mark.parametrize("offset", OFFSETS)
def test_find_arrow_offsets(offset):
    n = T + 65
    rng = np.random.default_rng(offset)
    vals = rng.integers(0, 1000, n)
    valid = rng.random(n) < 0.7
    col = Col(vals, valid, offset=offset, null_count_known=False)
    for res in (HOST, DEVICE):
        c = place(col, res)
        for value in (int(vals[5]), int(vals[T + 3]), int(vals[n - 1]), 1000):
            for start in (0, 6, T + 4):
                run_find(col, value, start, placed=c)
        run_find(col, None, 0, placed=c)


@pytest.mark.parametrize("res", [HOST, DEVICE, PINNED], ids=["host", "device", "pinned"])
def test_find_residencies(res):
    n = 2 * T + 9
    rng = np.random.default_rng(3)
    for col in (Col(rng.integers(-40, 40, n), rng.random(n) < 0.9, offset=1), Col(rng.integers(-40, 40, n).astype(np.float64) / 4)):
        for value, start in ((col.values[T + 2], 0), (col.values[T + 2], T + 3), (1000, 0), (None, 9)):
            run_find(col, value, start, res)


# ------------------------------------------------------------------ the reference's tests
def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "append_find_vectors.json")) as f:
        return json.load(f)["cases"]


def _col(c):
    dt = np.int64 if c["type"] == "int64" else np.float64
    data = c["data"]
    return Col(np.array([0 if x is None else x for x in data], dt), np.array([x is not None for x in data], bool))


@pytest.mark.parametrize("residency", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("case", _vectors(), ids=[c["name"] for c in _vectors()])
def test_golden_vectors(case, residency):
    if case["op"] == "find":
        col = _col(case["col"])
        c = place(col, residency)
        empty = capi.Column(c.values, c.validity, c.type, 0, 0, 0)      # NewEmptySlice
        for lookups, target in ((case["lookups"], c), (case["empty_lookups"], empty)):
            for lk in lookups:
                if isinstance(lk["value"], str):      # a value of another type: answered without a call
                    assert lk["expect"] == -1
                    continue
                assert capi.find_next(target, lk["value"], lk["row_start"]) == lk["expect"], lk
        return
    frames = [[_col(c) for c in f] for f in case["frames"]]
    total = sum(len(f[0].values) for f in frames)
    placed = [[place(c, residency) for c in f] for f in frames]
    outs = make_outs(len(frames[0]), max(total, 1), residency)
    if case.get("error"):
        with pytest.raises(capi.BowGpuError) as e:
            capi.append(placed, outs=outs)
        assert e.value.code == ERR_TYPE and case["error"] in e.value.message
        assert_untouched(outs, max(total, 1))
        return
    outs, unchanged = capi.append(placed, outs=outs)
    assert unchanged == case["unchanged"]
    want = [_col(c) for c in case["expected"]]
    if unchanged:
        assert_untouched(outs, max(total, 1))
        assert all(np.array_equal(a.bits(), w.bits()) for a, w in zip(frames[0], want))
    elif total:
        assert_appended([want], outs, max(total, 1))
    else:
        assert [(o.length, o.null_count) for o in outs] == [(0, 0)] * len(outs)


def test_cpp_mirror_replays_the_fixture():
    exe = os.path.join(ROOT, "tests", "cpp", "test_append_find")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures, 7 cases" in p.stdout


def test_four_threads_different_calls():
    """four OS threads at once, each its own call on its own context and stream: the results are those of the same calls made one by one"""
    frames = [piece(n, 60 + k, offset=k) for k, n in enumerate((T + 1, 65, 2 * T + 17))]
    total = sum(len(f[0].values) for f in frames)
    placed = [[c.column() for c in f] for f in frames]
    vals = np.arange(total, dtype=np.int64) % 5000
    hay = Col(vals, np.random.default_rng(0).random(total) < 0.9, offset=3).column()

    def snapshot(outs):
        return [(o.length, o.null_count, o.type) + tuple(x.tobytes() for x in raw(o, total)) for o in outs]

    calls = [lambda: snapshot(capi.append(placed, outs=make_outs(2, total, HOST))[0]),
             lambda: snapshot(capi.append(placed[::-1], outs=make_outs(2, total, DEVICE))[0]),
             lambda: [capi.find_next(hay, 4999, s) for s in (0, 5000, total - 1)],
             lambda: capi.find_next(hay, None)]
    serial = [call() for call in calls]
    got, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = calls[k]()
        except Exception as e:      # noqa: BLE001 - reported below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == serial
