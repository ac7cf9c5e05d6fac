"""Bow.InnerJoin / OuterJoin on the device (bowgpu_join / bowgpu_join_rows) against the pair list by its definition - a Python dict from
key to ascending right rows, outputs assembled with numpy - which is exact and independent of the library, and against the fixture of the
reference's own tests.  Every comparison is bit for bit: values as uint64, validity bytes, null_count, length and type, 0 in the null
slots, clear padding bits, and the sentinels of the output buffers intact past the slots produced (or everywhere, when a call returns
an error)."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from bow_amd import capi
from test_gpu_filter import DEVICE, HOST, I64_MAX, I64_MIN, PINNED, POISON, T, Col, assert_untouched, make_outs, pack, place, raw, release

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
OFFSETS = [0, 1, 7, 8, 63, 64, 65]
INNER, OUTER = capi.JOIN_INNER, capi.JOIN_OUTER
KINDS = {"inner": INNER, "outer": OUTER}
ERR_UNSUPPORTED, ERR_ARG = -9, -10


# ------------------------------------------------------------------ the oracle (the definition: exact) and the comparison
def valid_of(col):
    return np.ones(len(col.values), bool) if col.valid is None else np.asarray(col.valid, bool)


def pair_rows(lkey, rkey, kind):
    """(l_idx, r_idx, pairs): getCommonRows ordered by l then r, then the fill order of the kind; Go's == (a float key of a dict: -0.0
    and +0.0 are one key; None is nil)"""
    lv, rv = valid_of(lkey), valid_of(rkey)
    where = {}
    for r, (x, ok) in enumerate(zip(rkey.values.tolist(), rv.tolist())):
        where.setdefault(x if ok else None, []).append(r)
    li, ri, pairs, hit = [], [], 0, np.zeros(len(rv), bool)
    for l, (x, ok) in enumerate(zip(lkey.values.tolist(), lv.tolist())):
        rows = where.get(x if ok else None, ())
        pairs += len(rows)
        if rows:
            li += [l] * len(rows)
            ri += rows
            hit[rows] = True
        elif kind == OUTER:
            li.append(l)
            ri.append(-1)
    if kind == OUTER:
        tail = np.flatnonzero(~hit).tolist()
        li += [-1] * len(tail)
        ri += tail
    return np.array(li, np.int64), np.array(ri, np.int64), pairs


def identity_rows(nl, nr, kind):
    if kind == INNER:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    return np.concatenate([np.arange(nl), np.full(nr, -1)]).astype(np.int64), np.concatenate([np.full(nl, -1), np.arange(nr)]).astype(np.int64), 0


def take(col, idx):
    """(bits, valid) of col at idx, -1: null"""
    ok = idx >= 0
    if len(col.values) == 0:
        return np.zeros(len(idx), np.uint64), np.zeros(len(idx), bool)
    safe = np.where(ok, idx, 0)
    valid = ok & valid_of(col)[safe]
    return np.where(valid, col.bits()[safe], np.uint64(0)), valid


def expected_columns(left, lk, right, rk, li, ri):
    want = []
    for i, c in enumerate(left):
        bits, valid = take(c, li)
        if i == lk:      # a right-only row: the RIGHT key's value and validity
            b2, v2 = take(right[rk], ri)
            bits, valid = np.where(li >= 0, bits, b2), np.where(li >= 0, valid, v2)
        want.append((c.typ, bits, valid))
    for i, c in enumerate(right):
        if lk < 0 or i != rk:
            want.append((c.typ,) + take(c, ri))
    return want


def assert_joined(want, outs, rows, cap):
    nb = (rows + 7) // 8
    assert len(outs) == len(want)
    for (typ, bits, valid), o in zip(want, outs):
        v, b = raw(o, cap)
        assert o.length == rows and o.type == typ and o.null_count == rows - int(valid.sum())
        assert np.array_equal(v[:rows], bits)                                  # raw payloads; null slots hold 0
        assert np.array_equal(b[:nb], pack(valid))                             # validity; the padding bits of the last byte clear
        if rows:
            assert (v[rows:cap] == POISON).all() and (b[nb:] == 0xA5).all()    # nothing past slot rows - 1 / byte ceil(rows/8) - 1
        else:
            assert (v == POISON).all() and (b == 0xA5).all()


def run_join(left, lk, right, rk, kind, in_res=HOST, out_res=HOST, extra=0, rows_too=True):
    """in_res: one residency, or a function of (side, column); extra: capacity beyond the rows needed"""
    nl = len(left[0].values) if left else 0
    nr = len(right[0].values) if right else 0
    li, ri, pairs = pair_rows(left[lk], right[rk], kind) if lk >= 0 else identity_rows(nl, nr, kind)
    rows = len(li)
    res = in_res if callable(in_res) else (lambda side, i: in_res)
    pl = [place(c, res(0, i)) for i, c in enumerate(left)]
    pr = [place(c, res(1, i)) for i, c in enumerate(right)]
    try:
        if lk >= 0:
            assert capi.join_rows(pl[lk], pr[rk], kind, count_only=True)[2:] == (rows, pairs)
            if rows_too:
                gl, gr, grows, gpairs = capi.join_rows(pl[lk], pr[rk], kind, capacity=rows + 3)
                assert (grows, gpairs) == (rows, pairs)
                assert np.array_equal(gl[:rows], li) and np.array_equal(gr[:rows], ri)
                assert (gl[rows:] == -7).all() and (gr[rows:] == -7).all()
        n_outs = len(left) + len(right) - (1 if lk >= 0 else 0)
        cap = rows + extra
        outs, got = capi.join(pl, lk, pr, rk, kind, outs=make_outs(n_outs, cap, out_res))
        assert got == rows
        assert_joined(expected_columns(left, lk, right, rk, li, ri), outs, rows, cap)
    finally:
        release(pl + pr)
    return outs, li, ri


def frame(key, seed, p_null=0.3, offset=0, known=True):
    """key + two value columns: Float64 with nulls (random payloads under them), Int64 without a bitmap"""
    rng = np.random.default_rng(seed)
    n = len(key.values)
    return [key, Col(rng.standard_normal(n), rng.random(n) >= p_null, offset=offset, null_count_known=known), Col(rng.integers(I64_MIN, I64_MAX, n))]


def ikey(values, valid=None, **kw):
    return Col(np.asarray(values, np.int64), valid, **kw)


# ------------------------------------------------------------------ the reference's own cases
def case_frame(cols):
    out = []
    for c in cols:
        data = c["data"]
        valid = np.array([x is not None for x in data], bool)
        vals = np.array([0 if x is None else x for x in data], np.int64 if c["type"] == "int64" else np.float64)
        out.append(Col(vals, None if valid.all() else valid))
    return out


def test_fixture_cases_through_join_and_join_rows():
    with open(os.path.join(ROOT, "tests", "golden", "join_vectors.json")) as f:
        doc = json.load(f)
    ran = 0
    for c in doc["cases"]:
        if "declined" in c or "error" in c:
            continue
        left, right, lk, rk = case_frame(c["left"]), case_frame(c["right"]), c["left_key"], c["right_key"]
        for kind in (INNER, OUTER):
            outs, li, ri = run_join(left, lk, right, rk, kind, extra=2)
            if kind == KINDS[c["kind"]]:      # the reference's expected frame, literally
                assert [o.to_list() for o in outs] == [e["data"] for e in c["expected"]], c["name"]
                assert [o.type for o in outs] == [capi.TYPE_NAMES[e["type"]] for e in c["expected"]]
                ran += 1
        if lk < 0:      # no common column through bowgpu_join_rows: NULL keys, no pair, no rows; one key alone is declined
            assert capi.join_rows(None, None, OUTER, count_only=True)[2:] == (0, 0)
            if left:
                with pytest.raises(capi.BowGpuError) as e:
                    capi.join_rows(place(left[0], HOST), None, OUTER)
                assert e.value.code == ERR_ARG
    assert ran == 12


# ------------------------------------------------------------------ lengths
@pytest.mark.parametrize("nl", LENGTHS)
def test_lengths_both_kinds_both_key_types(nl):
    rng = np.random.default_rng(nl)
    for k, nr in enumerate(LENGTHS):
        span = max(8, nl * nr // 40000 + 1)      # a small range: matches, duplicates and misses; fewer than 1e5 output rows
        i = LENGTHS.index(nl)
        as_float = (k + i) % 2 == 1      # every L and every R meets both key types; join_rows meets both, too
        lv, rv = rng.integers(-2, span, nl), rng.integers(0, span + 2, nr)
        lkey = Col(lv.astype(np.float64)) if as_float else Col(lv)
        rkey = Col(rv.astype(np.float64), rng.random(nr) < 0.9) if as_float else Col(rv)
        in_res = DEVICE if (k + i) % 3 == 0 else HOST
        for kind in (INNER, OUTER):
            run_join(frame(lkey, 1)[:2], 0, frame(rkey, 2, offset=3), 0, kind, in_res, DEVICE if (k + 2 * i) % 4 == 1 else HOST,
                     rows_too=(k // 2 + i) % 2 == 0)


# ------------------------------------------------------------------ boundaries
def test_group_of_equals_across_a_sorted_tile_and_a_long_expansion_across_an_output_tile():
    rng = np.random.default_rng(5)
    # right: T - 30 distinct keys below X, then 1500 rows of X - a group that crosses the tile boundary of the sorted order (at T) and is
    # longer than a wave's 1024 output rows - then distinct keys above X; in shuffled row order
    X = 100000
    below, above = np.arange(T - 30), X + 1 + np.arange(700)
    rvals = np.concatenate([below, np.full(1500, X), above])
    rvals = rvals[rng.permutation(len(rvals))]
    # left: 3500 rows that match once each (a run of count-1 rows), the row that becomes 1500 rows (output rows 3500 .. 4999: across the
    # output tile at 4096), 600 count-1 rows behind it, two misses and X once more
    lvals = np.concatenate([below[:3500], [X], above[:600], [-5, X + 5000], [X]])
    right = frame(ikey(rvals), 11)
    for kind in (INNER, OUTER):
        outs, li, ri = run_join(frame(ikey(lvals), 10), 0, right, 0, kind, DEVICE, DEVICE)
        assert (li[3500:5000] == 3500).all() and (np.diff(ri[3500:5000]) > 0).all()      # one left row, ascending right rows
    # the same with the left key shuffled: the output keeps left order
    lsh = lvals[rng.permutation(len(lvals))]
    run_join(frame(ikey(lsh), 12), 0, right, 0, OUTER)


@pytest.mark.parametrize("start", [1, 7, 8, 63, 64, 64 + 63, T + 1])
def test_outer_tail_start_within_a_validity_word(start):
    """the right-only rows start at output row `start` (mod 64: 1, 7, 8, 63, 0): the word they share with the left part is stored whole"""
    rng = np.random.default_rng(start)
    lkey = ikey(-1 - np.arange(start))                                  # no left row matches
    rkey = ikey(rng.integers(0, 50, 300), rng.random(300) < 0.8)        # every right row is right-only, null keys included
    outs, li, ri = run_join(frame(lkey, 1, p_null=0.5), 0, frame(rkey, 2, p_null=0.5, offset=5), 0, OUTER)
    assert (li[:start] >= 0).all() and (li[start:] == -1).all() and ri[start:].tolist() == list(range(300))
    # ... and with one matched left row in front, whose right rows leave the tail
    lkey = ikey(np.concatenate([[7], -1 - np.arange(start - 1)]))
    run_join(frame(lkey, 3), 0, frame(rkey, 4), 0, OUTER, DEVICE)


# ------------------------------------------------------------------ null keys
@pytest.mark.parametrize("which", ["both", "left", "right", "all-null"])
def test_null_keys(which):
    rng = np.random.default_rng(3)
    nl, nr = T + 65, 2 * T + 1
    lv = rng.random(nl) < 0.97 if which in ("both", "left") else None
    rv = rng.random(nr) < 0.98 if which in ("both", "right") else None
    if which == "all-null":
        nl, nr = 130, 257      # nil == nil: every pair
        lv, rv = np.zeros(nl, bool), np.zeros(nr, bool)
    lkey = ikey(rng.integers(0, 3000, nl), lv, offset=7)
    rkey = ikey(rng.integers(0, 3000, nr), rv, offset=1, null_count_known=False)
    for kind in (INNER, OUTER):
        outs, li, ri = run_join(frame(lkey, 1), 0, frame(rkey, 2), 0, kind)
        if which == "right" and kind == OUTER:      # null right keys match nothing: right-only rows whose key stays null
            tail = ri[li < 0]
            assert set(np.flatnonzero(~rv)) <= set(tail.tolist())
            assert outs[0].null_count == int((~rv).sum())
        if which == "all-null":
            assert len(li) == nl * nr


# ------------------------------------------------------------------ Float64 edge values
def test_float_zeros_infinities_and_nan_payloads_in_value_columns():
    inf = np.inf
    lkey = Col(np.array([-0.0, 0.0, inf, -inf, 1.5, 5e-324, -0.0]))
    rkey = Col(np.array([0.0, -inf, -0.0, inf, 2.5, inf]))
    payload = np.array([0x7FF8000000000001, 0xFFF0000000000005, 0x7FF4000000000000, 1, 2, 3, 4], np.uint64).view(np.float64)
    left = [lkey, Col(payload)]
    right = [rkey, Col(np.array([0xFFF8DEADBEEF0001, 0x7FF0000000000009, 5, 6, 7, 8], np.uint64).view(np.float64))]
    for kind in (INNER, OUTER):
        outs, li, ri = run_join(left, 0, right, 0, kind)      # (bit for bit: each zero keeps its own sign, NaN payloads survive)
    assert [int(x) for x in ri[li == 0]] == [0, 2] and [int(x) for x in ri[li == 2]] == [3, 5] and [int(x) for x in ri[li == 3]] == [1]
    # a NaN among the valid keys of either side is declined, outputs untouched; under a null it is not a key
    nan_l = Col(np.array([1.0, np.nan, 2.0]))
    nan_r = Col(np.array([2.0, np.nan]))
    ok_l = Col(np.array([1.0, np.nan, 2.0]), np.array([True, False, True]))
    ok_r = Col(np.array([2.0, np.nan]), np.array([True, False]))
    for lk_, rk_ in ((nan_l, ok_r), (ok_l, nan_r), (nan_l, nan_r)):
        for kind in (INNER, OUTER):
            outs = make_outs(1, 8, HOST)
            with pytest.raises(capi.BowGpuError) as e:
                capi.join([lk_.column()], 0, [rk_.column()], 0, kind, outs=outs)
            assert e.value.code == ERR_UNSUPPORTED and "NaN" in e.value.message
            assert_untouched(outs, 8)
            with pytest.raises(capi.BowGpuError) as e:
                capi.join_rows(lk_.column(), rk_.column(), kind, count_only=True)
            assert e.value.code == ERR_UNSUPPORTED
    for kind in (INNER, OUTER):
        run_join([ok_l], 0, [ok_r], 0, kind)


# ------------------------------------------------------------------ key order
@pytest.mark.parametrize("order", ["sorted", "reversed", "shuffled"])
def test_right_key_order_and_left_order_kept(order):
    rng = np.random.default_rng(8)
    n = 2 * T + 9
    base = np.arange(n) * 3
    rvals = {"sorted": base, "reversed": base[::-1].copy(), "shuffled": base[rng.permutation(n)]}[order]
    right = frame(ikey(rvals), 2)
    # the time-series case: every row matches once; half the instants shared; no match at all
    for lvals in (base, base[rng.permutation(n)], base[: n // 2] * 2, base + 1):
        for kind in (INNER, OUTER):
            outs, li, ri = run_join(frame(ikey(lvals), 1), 0, right, 0, kind, DEVICE, HOST, rows_too=False)
            assert (np.diff(li[li >= 0]) >= 0).all()
    # duplicates in a sorted right key: ties come out in ascending right row
    dup = np.sort(rng.integers(0, 40, 500))
    run_join(frame(ikey(rng.integers(0, 45, 70)), 3), 0, frame(ikey(dup if order != "reversed" else dup[::-1].copy()), 4), 0, OUTER)


# ------------------------------------------------------------------ layout and residency
@pytest.mark.parametrize("offset", OFFSETS)
def test_arrow_offsets_and_null_counts(offset):
    rng = np.random.default_rng(offset)
    nl, nr = T + 3, 777
    lkey = ikey(rng.integers(0, 900, nl), rng.random(nl) < 0.9, offset=offset, null_count_known=bool(offset % 2))
    rkey = ikey(rng.integers(0, 900, nr), rng.random(nr) < 0.9, offset=(offset * 5) % 67, null_count_known=not offset % 2)
    left, right = frame(lkey, 1, offset=offset, known=False), frame(rkey, 2, offset=(offset * 3) % 65)
    for kind in (INNER, OUTER):
        run_join(left, 0, right, 0, kind)
    run_join(left, 0, right, 0, OUTER, DEVICE, DEVICE)


@pytest.mark.parametrize("out_res", [HOST, PINNED, DEVICE], ids=["out-host", "out-pinned", "out-device"])
def test_residencies_mixed_within_a_frame(out_res):
    rng = np.random.default_rng(21)
    lkey, rkey = ikey(rng.integers(0, 200, 300), rng.random(300) < 0.95), ikey(rng.integers(0, 200, 500), rng.random(500) < 0.95)
    mix = [HOST, PINNED, DEVICE]
    for shift in range(3):
        for kind in (INNER, OUTER):
            run_join(frame(lkey, 1), 0, frame(rkey, 2), 0, kind, lambda side, i: mix[(side + i + shift) % 3], out_res, extra=70)


@pytest.mark.parametrize("ncols,key", [(1, 0), (9, 0), (9, 4), (9, 5), (9, 8)])
def test_frames_of_one_and_nine_columns_key_anywhere(ncols, key):
    """nine columns: more than two launch groups of four; the key first, in the middle (the first and the second column of the second
    group: a right-only row reads the right key into either slot), last - at a different place in each frame"""
    rng = np.random.default_rng(ncols * 10 + key)
    nl, nr = 333, 411

    def wide(n, k, seed):
        r = np.random.default_rng(seed)
        cols = [Col(r.standard_normal(n), r.random(n) < 0.7) if i % 2 else Col(r.integers(I64_MIN, I64_MAX, n), r.random(n) < 0.8 if i % 4 == 0 else None)
                for i in range(ncols)]
        cols[k] = ikey(r.integers(0, 150, n), r.random(n) < 0.95)
        return cols

    rk = (ncols - 1) - key
    for kind in (INNER, OUTER):
        outs, li, ri = run_join(wide(nl, key, 1), key, wide(nr, rk, 2), rk, kind, DEVICE if key else HOST)
    assert (li < 0).any() and (ri < 0).any()      # OUTER: right-only rows (the key column's second source) and left-only rows
    run_join(wide(nl, key, 1), -1, wide(nr, rk, 2), -1, OUTER)      # no common column: all columns of both


def test_outer_join_into_the_second_round_of_the_gather_grid():
    """the gather's grid is capped at 2048 workgroups of 256 threads, so 524 288 output rows are one round of its grid-stride loop; the
    65 rows behind them hold left rows with a pair, left rows without one and right-only rows"""
    rng = np.random.default_rng(41)
    rows, n_tail = 2048 * 256 + 65, 20
    nl = rows - n_tail
    rvals = np.concatenate([np.arange(0, nl, 2), nl + np.arange(n_tail)])      # every second left key, and keys no left row has
    left = frame(ikey(np.arange(nl)), 1)[:2]
    right = frame(ikey(rvals[rng.permutation(len(rvals))]), 2, offset=3)[:2]
    outs, li, ri = run_join(left, 0, right, 0, OUTER, DEVICE, HOST, rows_too=False)
    assert len(li) == rows
    last = slice(2048 * 256, rows)
    assert ((li[last] >= 0) & (ri[last] >= 0)).any() and ((li[last] >= 0) & (ri[last] < 0)).any() and (li[last] < 0).sum() == n_tail


# ------------------------------------------------------------------ capacity and count
def test_capacity_exact_larger_and_one_too_small():
    rng = np.random.default_rng(4)
    left, right = frame(ikey(rng.integers(0, 60, 200)), 1), frame(ikey(rng.integers(0, 70, 180)), 2)
    for kind in (INNER, OUTER):
        for out_res in (HOST, DEVICE):
            run_join(left, 0, right, 0, kind, HOST, out_res, extra=0)
            outs, li, ri = run_join(left, 0, right, 0, kind, HOST, out_res, extra=129)
            rows = len(li)
            small = make_outs(5, rows, out_res)[:4] + make_outs(1, rows - 1, out_res)
            with pytest.raises(capi.BowGpuError) as e:
                capi.join([c.column() for c in left], 0, [c.column() for c in right], 0, kind, outs=small)
            assert e.value.code == ERR_ARG and "%d needed" % rows in e.value.message
            assert_untouched(small[:4], rows)
            assert_untouched(small[4:], rows - 1)
        lk, rk = left[0].column(), right[0].column()
        with pytest.raises(capi.BowGpuError) as e:
            capi.join_rows(lk, rk, kind, capacity=rows - 1)
        assert e.value.code == ERR_ARG and "%d needed" % rows in e.value.message
        gl, gr, grows, _ = capi.join_rows(lk, rk, kind, out_residency=DEVICE)      # device-resident index buffers
        assert grows == rows and np.array_equal(gl.to_numpy(np.int64, rows), li) and np.array_equal(gr.to_numpy(np.int64, rows), ri)


# ------------------------------------------------------------------ determinism and threads
def test_same_call_same_bytes_and_four_threads_at_once():
    rng = np.random.default_rng(77)
    jobs = []
    for t in range(4):
        nl, nr = 2 * T + 100 * t, T + 17 * t
        left = frame(ikey(rng.integers(0, 2500, nl), rng.random(nl) < 0.97), 10 + t)
        right = frame(ikey(rng.integers(0, 2500, nr), rng.random(nr) < 0.97), 20 + t)
        jobs.append((left, right, OUTER if t % 2 else INNER))
    left, right, kind = jobs[1]
    a, _, _ = run_join(left, 0, right, 0, kind, DEVICE, HOST)
    b, _, _ = run_join(left, 0, right, 0, kind, DEVICE, HOST)
    for x, y in zip(a, b):
        assert np.array_equal(raw(x, x.length)[0], raw(y, y.length)[0]) and np.array_equal(raw(x, x.length)[1], raw(y, y.length)[1])
    errors = []

    def work(job):
        try:
            for _ in range(3):
                run_join(job[0], 0, job[1], 0, job[2], DEVICE, HOST)
        except BaseException as e:      # noqa: BLE001 - handed to the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ------------------------------------------------------------------ the C++ mirror
def test_cpp_mirror_replays_the_fixture():
    exe = os.path.join(ROOT, "tests", "cpp", "test_join")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures, 19 cases" in p.stdout
