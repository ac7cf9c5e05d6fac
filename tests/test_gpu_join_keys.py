"""Bow.InnerJoin / OuterJoin on several common columns on the device (bowgpu_join_keys / bowgpu_join_keys_rows) against the model of
tests/join_keys_model.py - proved on the CPU in tests/test_join_keys_cpu.py - and against the fixture of the reference's own cases with
two common columns.  Every comparison is bit for bit: values as uint64, validity bytes, null_count, length and type, 0 in the null slots,
clear padding bits, and the sentinels of the output buffers intact past the slots produced (or everywhere, when a call returns an
error).  There is no tolerance anywhere: every step of the method is an integer count."""
import json
import os
import subprocess

import numpy as np
import pytest

import join_keys_model as model
from bow_amd import capi
from test_gpu_filter import DEVICE, HOST, I64_MAX, I64_MIN, PINNED, T, Col, assert_untouched, make_outs, place, raw, release
from test_gpu_join import LENGTHS, assert_joined

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, OUTER = capi.JOIN_INNER, capi.JOIN_OUTER
KINDS = {"inner": INNER, "outer": OUTER}
ERR_UNSUPPORTED, ERR_ARG = -9, -10


# ------------------------------------------------------------------ one call, judged by the model
def run_keys(left, lks, right, rks, kind, in_res=HOST, out_res=HOST, extra=0, rows_too=True):
    """in_res: one residency, or a function of (side, column); extra: capacity beyond the rows needed"""
    li, ri, pairs = model.join_rows(left, lks, right, rks, kind)
    rows = len(li)
    res = in_res if callable(in_res) else (lambda side, i: in_res)
    pl = [place(c, res(0, i)) for i, c in enumerate(left)]
    pr = [place(c, res(1, i)) for i, c in enumerate(right)]
    try:
        if lks:
            lk, rk = [pl[k] for k in lks], [pr[k] for k in rks]
            assert capi.join_keys_rows(lk, rk, kind, count_only=True)[2:] == (rows, pairs)
            if rows_too:
                gl, gr, grows, gpairs = capi.join_keys_rows(lk, rk, kind, capacity=rows + 3)
                assert (grows, gpairs) == (rows, pairs)
                assert np.array_equal(gl[:rows], li) and np.array_equal(gr[:rows], ri)
                assert (gl[rows:] == -7).all() and (gr[rows:] == -7).all()      # the sentinel past `rows`
        cap = rows + extra
        outs, got = capi.join_keys(pl, lks, pr, rks, kind, outs=make_outs(len(left) + len(right) - len(lks), cap, out_res))
        assert got == rows
        assert_joined(model.expected_columns(left, lks, right, rks, li, ri), outs, rows, cap)
    finally:
        release(pl + pr)
    return outs, li, ri


def icol(values, valid=None, **kw):
    return Col(np.asarray(values, np.int64), valid, **kw)


def fcol(values, valid=None, **kw):
    return Col(np.asarray(values, np.float64), valid, **kw)


def values(n, seed, p_null=0.3, offset=0):
    """two value columns: Float64 with nulls (random payloads under them), Int64 without a bitmap"""
    rng = np.random.default_rng(seed)
    return [Col(rng.standard_normal(n), rng.random(n) >= p_null, offset=offset), Col(rng.integers(I64_MIN, I64_MAX, n))]


def series_frames(nl, nr, seed, n_series=5, p_null=0.0, span=None):
    """(time, series id, values ...) on the left, (values, series id, time) on the right: keys (0, 1) and (2, 1)"""
    rng = np.random.default_rng(seed)
    span = span or max(4, (nl + nr) // (2 * n_series))

    def keys(n):
        t, s = rng.integers(0, span, n), rng.integers(0, n_series, n)
        vt = rng.random(n) >= p_null if p_null else None
        vs = rng.random(n) >= p_null if p_null else None
        return icol(t, vt), icol(s, vs)

    lt, ls = keys(nl)
    rt, rs = keys(nr)
    lv, rv = values(nl, seed + 1), values(nr, seed + 2, offset=3)
    return [lt, ls, lv[0]], [0, 1], [rv[0], rs, rt, rv[1]], [2, 1]


# ------------------------------------------------------------------ the reference's own cases
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "join_keys_vectors.json")) as f:
        return json.load(f)


def test_fixture_cases_through_join_keys_and_join_keys_rows():
    ran = 0
    for c in fixture()["cases"]:
        left, right = model.case_frame(c["left"], Col), model.case_frame(c["right"], Col)
        lks, rks = c["left_keys"], c["right_keys"]
        for kind in (INNER, OUTER):
            outs, li, ri = run_keys(left, lks, right, rks, kind, extra=2)
            if kind == KINDS[c["kind"]]:      # the reference's expected frame, literally
                assert repr([o.to_list() for o in outs]) == repr([e["data"] for e in c["expected"]]), c["name"]
                assert [o.type for o in outs] == [capi.TYPE_NAMES[e["type"]] for e in c["expected"]]
                ran += 1
        if "expected_swapped" in c:
            outs, li, ri = run_keys(right, rks, left, lks, KINDS[c["kind"]])
            assert repr([o.to_list() for o in outs]) == repr([e["data"] for e in c["expected_swapped"]]), c["name"]
            ran += 1
    assert ran == 6


def test_cpp_mirror_replays_the_fixture():
    exe = os.path.join(ROOT, "tests", "cpp", "test_join_keys")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures, 5 cases" in p.stdout


# ------------------------------------------------------------------ no key and one key: the one-key join itself
def same_bytes(a, b, cap):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x.length, x.type, x.null_count) == (y.length, y.type, y.null_count)
        (xv, xb), (yv, yb) = raw(x, cap), raw(y, cap)
        assert np.array_equal(xv, yv) and np.array_equal(xb, yb)


@pytest.mark.parametrize("out_res", [HOST, DEVICE], ids=["out-host", "out-device"])
def test_one_key_and_no_key_give_the_bytes_of_join_and_join_rows(out_res):
    rng = np.random.default_rng(17)
    nl, nr = T + 70, 2 * T + 3
    left = [Col(rng.standard_normal(nl), rng.random(nl) < 0.8), icol(rng.integers(0, 900, nl), rng.random(nl) < 0.95, offset=5)] + values(nl, 1)
    right = [icol(rng.integers(0, 900, nr), rng.random(nr) < 0.95, null_count_known=False)] + values(nr, 2, offset=1)
    pl, pr = [place(c, DEVICE) for c in left], [place(c, HOST) for c in right]
    for kind in (INNER, OUTER):
        al, ar, arows, apairs = capi.join_rows(pl[1], pr[0], kind)
        bl, br, brows, bpairs = capi.join_keys_rows([pl[1]], [pr[0]], kind)
        assert (arows, apairs) == (brows, bpairs) and np.array_equal(al, bl) and np.array_equal(ar, br)
        cap = arows + 9
        a, ra = capi.join(pl, 1, pr, 0, kind, outs=make_outs(6, cap, out_res))
        b, rb = capi.join_keys(pl, [1], pr, [0], kind, outs=make_outs(6, cap, out_res))
        assert ra == rb == arows
        same_bytes(a, b, cap)
        # no key: the -1 / -1 join (small frames: an OuterJoin of every row of both)
        cap = (nl + nr if kind == OUTER else 0) + 5
        a, ra = capi.join(pl, -1, pr, -1, kind, outs=make_outs(7, cap, out_res))
        b, rb = capi.join_keys(pl, [], pr, [], kind, outs=make_outs(7, cap, out_res))
        assert ra == rb == cap - 5
        same_bytes(a, b, cap)
        assert capi.join_keys_rows([], [], kind, count_only=True)[2:] == capi.join_rows(None, None, kind, count_only=True)[2:] == (0, 0)
    run_keys(left, [1], right, [0], OUTER, DEVICE, out_res)      # ... and the model agrees with both


# ------------------------------------------------------------------ the surrogate keeps every key
def test_both_keys_matter():
    """rows that agree on key 0 and not on key 1, and the other way round: the join on either key alone has another row count, so a
    surrogate that drops or swaps a rank cannot pass"""
    n = 600
    a, b = np.arange(n) % 20, np.arange(n) // 20      # every (a, b) once
    rng = np.random.default_rng(2)
    lp, rp = rng.permutation(n)[:400], rng.permutation(n)[:450]
    left = [icol(a[lp]), icol(b[lp])] + values(400, 1)
    right = [icol(b[rp]), icol(a[rp])] + values(450, 2)      # the keys the other way round in the right frame
    for kind in (INNER, OUTER):
        outs, li, ri = run_keys(left, [0, 1], right, [1, 0], kind, DEVICE)
        both = len(li)
        only0 = model.join_rows(left, [0], right, [1], kind)
        only1 = model.join_rows(left, [1], right, [0], kind)
        swapped = model.join_rows(left, [0, 1], right, [0, 1], kind)      # a with b, b with a
        assert len({both, len(only0[0]), len(only1[0]), len(swapped[0])}) == 4
    # tuples (x, y) and (y, x) are different keys
    run_keys([icol([1, 2, 1, 2]), icol([2, 1, 1, 2])], [0, 1], [icol([2, 1]), icol([1, 2])], [0, 1], OUTER)


def test_neighbouring_tuples_groups_of_equals_and_a_long_expansion_across_an_output_tile():
    rng = np.random.default_rng(5)
    # distinct tuples whose packed ranks are neighbours: (a, b) over a small grid, so that (a, last b) and (a + 1, first b) sit side by
    # side in the sorted surrogate.  On the right: T - 30 tuples once, one tuple 1500 times (a group across the sorted tile at T and longer
    # than a wave's 1024 output rows), one tuple twice, 700 tuples once - in shuffled row order
    grid = [(a, b) for a in range(80) for b in range(64)]
    once, X, twice, above = grid[:T - 30], grid[T - 30], grid[T - 29], grid[T - 28:T - 28 + 700]
    rt = np.array(once + [X] * 1500 + [twice] * 2 + above)
    rt = rt[rng.permutation(len(rt))]
    # left: 3500 rows that match once each, the row that becomes 1500 rows (output rows 3500 .. 4999: across the output tile at 4096),
    # 600 count-1 rows, the tuple with two matches, misses that are neighbours of hits in ONE key, X once more
    lt = np.array(once[:3500] + [X] + above[:600] + [twice, (X[0], 9999), (9999, X[1]), (-1, -1)] + [X])
    right = [icol(rt[:, 0]), fcol(rt[:, 1])] + values(len(rt), 11)
    for kind in (INNER, OUTER):
        outs, li, ri = run_keys([icol(lt[:, 0]), fcol(lt[:, 1])] + values(len(lt), 10), [0, 1], right, [0, 1], kind, DEVICE, DEVICE)
        assert (li[3500:5000] == 3500).all() and (np.diff(ri[3500:5000]) > 0).all()      # one left row, ascending right rows
    lsh = lt[rng.permutation(len(lt))]      # the left rows shuffled: the output keeps left order
    run_keys([icol(lsh[:, 0]), fcol(lsh[:, 1])] + values(len(lsh), 12), [0, 1], right, [0, 1], OUTER)


# ------------------------------------------------------------------ sizes
# L + R around the sort's tile and the filter tile (both T rows), the scan's block of 4096 counts (the marks are L + R + 1 counts) and
# twice that
TOTALS = [2, 65, T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17]


@pytest.mark.parametrize("total", TOTALS)
def test_sizes_of_both_sides_together(total):
    for k, nl in enumerate(sorted({1, total // 3, total - 1})):
        nr = total - nl
        left, lks, right, rks = series_frames(nl, nr, total + k, p_null=0.05 if k % 2 else 0.0)
        for kind in (INNER, OUTER):
            run_keys(left, lks, right, rks, kind, DEVICE if (k + total) % 2 else HOST, DEVICE if k == 1 else HOST, rows_too=k != 1)


@pytest.mark.parametrize("nl", LENGTHS)
def test_lengths_of_a_side_empty_sides_included(nl):
    for k, nr in enumerate(LENGTHS):
        if k % 3 != LENGTHS.index(nl) % 3 and nl and nr:      # every length meets 0 and a third of the others
            continue
        left, lks, right, rks = series_frames(nl, nr, 100 * nl + nr, n_series=3, span=max(4, nl * nr // 30000 + 1))
        for kind in (INNER, OUTER):
            run_keys(left, lks, right, rks, kind, HOST if k % 2 else DEVICE)


# ------------------------------------------------------------------ key counts, types and positions
@pytest.mark.parametrize("n_keys", [2, 3, 8])
def test_key_counts_types_and_positions(n_keys):
    """Int64 and Float64 keys mixed, at different positions in the two frames, one key constant, one key pair already in order on both
    sides; with 8 keys of two values each a tuple is a byte, and every key decides some pair"""
    rng = np.random.default_rng(n_keys)
    nl, nr = T + 300, T - 100
    ncl, ncr = n_keys + 3, n_keys + 2
    lks, rks = rng.permutation(ncl)[:n_keys].tolist(), rng.permutation(ncr)[:n_keys].tolist()
    base = {2: 40, 3: 12, 8: 2}[n_keys]

    def key(n, k, side):
        if k == 0:      # in order on both sides
            return icol(np.sort(rng.integers(0, base, n)))
        if k == 1 and n_keys > 2:      # constant
            return fcol(np.full(n, 2.5))
        v = rng.integers(0, base, n)
        return fcol(v * 0.5, rng.random(n) < 0.97) if k % 2 else icol(v - 1, rng.random(n) < 0.97 if side else None)

    def frame(n, ncols, keys, side):
        fill = values(n, 7 + side) + values(n, 9 + side)
        return [key(n, keys.index(i), side) if i in keys else fill[i % 4] for i in range(ncols)]

    left, right = frame(nl, ncl, lks, 0), frame(nr, ncr, rks, 1)
    for kind in (INNER, OUTER):
        outs, li, ri = run_keys(left, lks, right, rks, kind, DEVICE if kind == OUTER else HOST)
    rows = len(li)
    for drop in range(n_keys):      # without any one key pair (but the constant one) the join is another
        if drop == 1 and n_keys > 2:
            continue
        fewer = model.join_rows(left, lks[:drop] + lks[drop + 1:], right, rks[:drop] + rks[drop + 1:], OUTER)
        assert len(fewer[0]) != rows, drop


@pytest.mark.parametrize("lks", [[10, 5], [0, 1]], ids=["keys-at-5-and-10", "keys-at-0-and-1"])
def test_a_key_column_anywhere_within_its_piece_of_the_left_frame(lks):
    """The left frame is gathered in pieces cut after every key column but the last.  11 columns, 4 to a launch.  Keys at 5 and 10: piece
    0 is columns 0-5 with its key in the second group of four at slot 1, piece 1 is columns 6-10 with its key in the second group at slot
    0 - and the pairs are listed [10, 5], not in frame order.  Keys at 0 and 1: a piece of one column, then a piece that starts with its
    key.  A key column's right partner is read through the second index on right-only rows alone: an OuterJoin that has some, nulls in
    both keys, one Int64 and one Float64 key, one left key host-resident and one device-resident"""
    rng = np.random.default_rng(11)
    nl, nr = 300, 200
    rks = [2, 0]

    def keys(n, span):
        return icol(rng.integers(0, span, n), rng.random(n) < 0.9), fcol(rng.integers(0, span - 2, n) * 0.5, rng.random(n) < 0.9)

    lkeys, rkeys = keys(nl, 6), keys(nr, 9)      # right tuples beyond the left's: right-only rows
    fill = [c for seed in range(6) for c in values(nl, 20 + seed)]
    left = [lkeys[lks.index(i)] if i in lks else fill[i] for i in range(11)]
    right = [rkeys[1], values(nr, 30)[0], rkeys[0], values(nr, 31)[1]]
    mix = [HOST, PINNED, DEVICE]

    def res(side, i):
        if side == 0 and i in lks:
            return HOST if i == lks[0] else DEVICE
        return mix[(side + i) % 3]

    for kind in (INNER, OUTER):
        outs, li, ri = run_keys(left, lks, right, rks, kind, res, DEVICE if kind == OUTER else HOST)
    right_only = ri[li == -1]
    assert len(right_only) > 0 and (li >= 0).sum() > nl      # right-only rows, and left rows with several partners
    for k in range(2):      # ... some of them with a null in each key: the right partner's validity is read there too
        assert not model.valid_of(right[rks[k]])[right_only].all() and model.valid_of(right[rks[k]])[right_only].any()


# ------------------------------------------------------------------ nulls and NaN
@pytest.mark.parametrize("which", ["none-null", "key0", "key1", "both", "all-null"])
def test_nulls_in_every_subset_of_the_keys(which):
    rng = np.random.default_rng(3)
    nl, nr = (T + 65, 2 * T + 1) if which != "all-null" else (130, 257)
    p0 = {"none-null": 1.0, "key0": 0.9, "key1": 1.0, "both": 0.9, "all-null": 0.0}[which]
    p1 = {"none-null": 1.0, "key0": 1.0, "key1": 0.9, "both": 0.9, "all-null": 0.0}[which]

    def keys(n, off):
        # random payloads, NaN and the bits of real keys included, under the nulls: never declined, never matched
        f = rng.integers(0, 6, n).astype(np.float64)
        v1 = rng.random(n) < p1
        f = np.where(v1 | (rng.random(n) < 0.5), f, np.nan)
        return icol(rng.integers(0, 40, n), rng.random(n) < p0, offset=off), fcol(f, v1, offset=off + 2, null_count_known=False)

    l0, l1 = keys(nl, 7)
    r0, r1 = keys(nr, 1)
    left, right = [l0, l1] + values(nl, 1), [r1] + values(nr, 2) + [r0]
    for kind in (INNER, OUTER):
        outs, li, ri = run_keys(left, [0, 1], right, [3, 0], kind)
        if which == "all-null":
            assert len(li) == nl * nr      # nil == nil in every key: every pair
    if which == "both":      # tuples null in key 0 alone, in key 1 alone and in both are three different keys, and each matches its like
        lt, rt = model.key_tuples([l0, l1]), model.key_tuples([r0, r1])
        inner = model.join_rows(left, [0, 1], right, [3, 0], INNER)
        for shape in ((True, False), (False, True), (True, True)):
            hit = [(lt[l][0] is None, lt[l][1] is None) == shape for l in inner[0].tolist()]
            assert any(hit)
        assert all((lt[l][0] is None, lt[l][1] is None) == (rt[r][0] is None, rt[r][1] is None) for l, r in zip(inner[0].tolist(), inner[1].tolist()))


def test_float_zeros_match_and_a_nan_among_valid_keys_is_declined():
    inf = np.inf
    l0, l1 = fcol([-0.0, 0.0, inf, -inf, 1.5, -0.0, 0.0]), fcol([0.0, -0.0, 1.0, 1.0, -0.0, 7.0, 0.0])
    r0, r1 = fcol([0.0, -inf, -0.0, inf, 1.5, inf]), fcol([-0.0, 1.0, 0.0, 1.0, 0.0, 2.0])
    payload = np.array([0x7FF8000000000001, 0xFFF0000000000005, 0x7FF4000000000000, 1, 2, 3, 4], np.uint64).view(np.float64)
    left, right = [l0, Col(payload), l1], [r0, r1, Col(np.array([0xFFF8DEADBEEF0001, 5, 6, 7, 8, 9], np.uint64).view(np.float64))]
    for kind in (INNER, OUTER):
        outs, li, ri = run_keys(left, [0, 2], right, [0, 1], kind)      # (bit for bit: each zero keeps the LEFT row's sign)
    assert [int(x) for x in ri[li == 0]] == [0, 2] and [int(x) for x in ri[li == 1]] == [0, 2] and [int(x) for x in ri[li == 6]] == [0, 2]
    assert [int(x) for x in ri[li == 2]] == [3] and [int(x) for x in ri[li == 3]] == [1] and [int(x) for x in ri[li == 4]] == [4]
    v, _ = raw(outs[0], len(li))
    assert v[0] == v[1] == 0x8000000000000000 and v[2] == v[3] == 0      # left rows 0 (-0.0) and 1 (+0.0), twice each
    # a NaN among the valid keys of either side, in any key pair, is declined naming side and pair; under a null it is not a key
    good, ok = fcol([1.0, 2.0, 3.0]), fcol([1.0, np.nan, 2.0], np.array([True, False, True]))
    bad = fcol([1.0, np.nan, 2.0])
    for pair in (0, 1):
        for side in ("left", "right"):
            lk = [good, good]
            rk = [good, good]
            (lk if side == "left" else rk)[pair] = bad
            (rk if side == "left" else lk)[pair] = ok
            for kind in (INNER, OUTER):
                for res in (HOST, DEVICE):
                    outs = make_outs(2, 8, res)
                    pl, pr = [place(c, res) for c in lk], [place(c, res) for c in rk]
                    with pytest.raises(capi.BowGpuError) as e:
                        capi.join_keys(pl, [0, 1], pr, [0, 1], kind, outs=outs)
                    assert e.value.code == ERR_UNSUPPORTED and "NaN" in e.value.message
                    assert e.value.message.startswith(side) and "key pair %d" % pair in e.value.message
                    assert_untouched(outs, 8)
                    with pytest.raises(capi.BowGpuError) as e:
                        capi.join_keys_rows(pl, pr, kind, count_only=True)
                    assert e.value.code == ERR_UNSUPPORTED and e.value.message.startswith(side)
    for kind in (INNER, OUTER):
        run_keys([ok, good], [0, 1], [good, ok], [1, 0], kind)


# ------------------------------------------------------------------ layout, residency, capacity
@pytest.mark.parametrize("offset", [0, 1, 7, 8, 63, 65])
def test_arrow_offsets_and_null_counts(offset):
    rng = np.random.default_rng(offset)
    nl, nr = T + 3, 777
    l0 = icol(rng.integers(0, 30, nl), rng.random(nl) < 0.9, offset=offset, null_count_known=bool(offset % 2))
    l1 = icol(rng.integers(0, 30, nl), rng.random(nl) < 0.9, offset=(offset * 3) % 65, null_count_known=not offset % 2)
    r0 = icol(rng.integers(0, 30, nr), rng.random(nr) < 0.9, offset=(offset * 5) % 67, null_count_known=not offset % 2)
    r1 = icol(rng.integers(0, 30, nr), rng.random(nr) < 0.9, offset=(offset + 13) % 64, null_count_known=bool(offset % 2))
    left, right = [l0] + values(nl, 1, offset=offset) + [l1], [r1, r0] + values(nr, 2, offset=(offset * 3) % 65)
    for kind in (INNER, OUTER):
        run_keys(left, [0, 3], right, [1, 0], kind)
    run_keys(left, [0, 3], right, [1, 0], OUTER, DEVICE, DEVICE)


@pytest.mark.parametrize("out_res", [HOST, PINNED, DEVICE], ids=["out-host", "out-pinned", "out-device"])
def test_residencies_mixed_within_a_frame(out_res):
    left, lks, right, rks = series_frames(300, 500, 21, p_null=0.05)
    mix = [HOST, PINNED, DEVICE]
    for shift in range(3):
        for kind in (INNER, OUTER):
            run_keys(left, lks, right, rks, kind, lambda side, i: mix[(side + i + shift) % 3], out_res, extra=70)


def test_capacity_exact_larger_and_one_too_small():
    left, lks, right, rks = series_frames(200, 180, 4, n_series=3, span=12)
    n_outs = len(left) + len(right) - 2
    for kind in (INNER, OUTER):
        for out_res in (HOST, DEVICE):
            run_keys(left, lks, right, rks, kind, HOST, out_res, extra=0)
            outs, li, ri = run_keys(left, lks, right, rks, kind, HOST, out_res, extra=129)
            rows = len(li)
            small = make_outs(n_outs, rows, out_res)[:n_outs - 1] + make_outs(1, rows - 1, out_res)
            with pytest.raises(capi.BowGpuError) as e:
                capi.join_keys([c.column() for c in left], lks, [c.column() for c in right], rks, kind, outs=small)
            assert e.value.code == ERR_ARG and "%d needed" % rows in e.value.message
            assert_untouched(small[:n_outs - 1], rows)
            assert_untouched(small[n_outs - 1:], rows - 1)
        lk, rk = [left[k].column() for k in lks], [right[k].column() for k in rks]
        with pytest.raises(capi.BowGpuError) as e:
            capi.join_keys_rows(lk, rk, kind, capacity=rows - 1)
        assert e.value.code == ERR_ARG and "%d needed" % rows in e.value.message
        gl, gr, grows, _ = capi.join_keys_rows(lk, rk, kind, out_residency=DEVICE)      # device-resident index buffers
        assert grows == rows and np.array_equal(gl.to_numpy(np.int64, rows), li) and np.array_equal(gr.to_numpy(np.int64, rows), ri)


def test_same_call_same_bytes():
    left, lks, right, rks = series_frames(2 * T + 100, T + 17, 77, p_null=0.03)
    a, li, _ = run_keys(left, lks, right, rks, OUTER, DEVICE, HOST)
    b, _, _ = run_keys(left, lks, right, rks, OUTER, DEVICE, HOST)
    same_bytes(a, b, len(li))


# ------------------------------------------------------------------ routing
def test_a_call_on_two_keys_ends_in_a_kernel_of_the_join_path():
    left, lks, right, rks = series_frames(500, 400, 9)
    pl, pr = [place(c, DEVICE) for c in left], [place(c, DEVICE) for c in right]
    capi.join_keys(pl, lks, pr, rks, OUTER)
    assert capi.last_kernel_name() == "gather_kernel"
    capi.join_keys_rows([pl[k] for k in lks], [pr[k] for k in rks], OUTER)
    assert capi.last_kernel_name() == "join_expand_kernel"
    capi.join_keys_rows([pl[k] for k in lks], [pr[k] for k in rks], OUTER, count_only=True)
    assert capi.last_kernel_name() == "join_probe_kernel"
