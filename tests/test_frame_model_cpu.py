"""tests/frame_model.py without a GPU: the model of the frame operations against the reference's own test tables (tests/golden) and
against brute-force definitions written out here; the coverage conditions of the plans tests/test_gpu_frame_fuzz.py executes - a fuzz
that silently skips cases hides failures, so they are asserted, for the seeds that test runs by default; and the sensitivity of the
comparison - each deliberately wrong model below must give a different result in at least one step of every block of 8 seeds, which
shows that a kernel wrong in that way would be seen."""
import json
import os
from collections import Counter

import numpy as np
import pytest

import frame_model as fm
from frame_model import FLOAT64, INT64, M, MCol, declined, from_list, rows_of, to_list, vals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_SEEDS = range(64 // 2)          # test_gpu_frame_fuzz.SEEDS without BOW_FUZZ_SEEDS


def table(name):
    with open(os.path.join(GOLDEN, name + "_vectors.json")) as f:
        return json.load(f)["cases"]


def frame_of(cols):
    return [from_list(c["data"], c["type"]) for c in cols]


def same_frame(name, got, expected):
    assert len(got) == len(expected), name
    for g, e in zip(got, expected):
        assert g.typ == {"int64": INT64, "float64": FLOAT64}[e["type"]], name
        assert to_list(g) == e["data"], (name, to_list(g), e["data"])
        assert not g.bits[~g.valid].any(), name             # null slots hold 0


# ------------------------------------------------------------------ the model against the reference's own tables
def test_model_reproduces_the_sort_table():
    for c in table("sort"):
        r = M.sort_by_col(frame_of(c["cols"]), c["key_col"])
        if "error" in c:
            assert r == (c["error"]["code"],) == (fm.ERR_SORT_NULLS,), c["name"]
        elif c.get("unchanged"):
            assert r.unchanged and r.cols is None, c["name"]
        else:
            assert not r.unchanged, c["name"]
            same_frame(c["name"], r.cols, c["expected"])


def converted(values):
    """Type.Convert on a Float64 column: a number, or nil for a string that is none - the predicate then holds on null rows"""
    nums, nil = [], False
    for v in values:
        try:
            nums.append(float(v))
        except ValueError:
            nil = True
    return np.array(nums, np.float64), nil


def test_model_reproduces_the_filter_table():
    for c in table("filter"):
        frame = frame_of(c["cols"])
        preds = [(p["col"],) + converted(p["values"]) for p in c["preds"]]
        r = M.filter(frame, preds)
        assert bool(r.contiguous) == c["contiguous"] and r.count == c["count"], c["name"]
        if c["contiguous"]:
            assert r.first == c["first"] and r.cols is None, c["name"]
        else:
            same_frame(c["name"], r.cols, c["expected"])
        m = M.filter_mask(frame, preds)
        assert m.selected == c["count"] and (M.compact(frame, m.mask).cols is None) == c["contiguous"], c["name"]


def settled(frame):
    return [M.out(c.typ, c.bits, c.valid) for c in frame]


def test_model_reproduces_the_frame_ops_table():
    for c in table("frame_ops"):
        frame, name = frame_of(c["cols"]), c["name"]
        if c["op"] == "drop_nils":
            r = M.drop_nils(frame, c["col_idx"])
            # the reference returns the receiver exactly when nothing is dropped
            assert c["unchanged"] == bool(r.contiguous and r.count == rows_of(frame)), name
            same_frame(name, settled(fm.slice_frame(frame, r.first, r.count)) if r.contiguous else r.cols, c["expected"])
        elif c["op"] == "diff":
            r = M.diff(frame, c["col_idx"])
            if c.get("error"):
                assert r == (fm.ERR_BAD_COL,), name
                continue
            whole = list(frame)                               # unselected columns pass through
            for i, d in zip(M.select_cols(len(frame), c["col_idx"]), r.cols):
                whole[i] = d
            same_frame(name, whole, c["expected"])
            assert not any(g.any() for g in r.gen_nan), name
        else:
            r = M.distinct(frame[c["col"]])
            assert r.n_distinct == len(c["expected"][0]["data"]), name
            same_frame(name, r.cols, c["expected"])


def test_model_reproduces_the_append_and_find_table():
    for c in table("append_find"):
        name = c["name"]
        if c["op"] == "append":
            frames = [frame_of(f) for f in c["frames"]]
            r = M.append(frames)
            if "error" in c:
                assert r == (fm.ERR_TYPE,), name
            elif c["unchanged"]:
                assert r.unchanged and r.cols is None, name
                same_frame(name, frames[0], c["expected"])
            else:
                assert not r.unchanged, name
                same_frame(name, r.cols, c["expected"])
            continue
        col = from_list(c["col"]["data"], c["col"]["type"])
        for lookups, on in ((c["lookups"], col), (c["empty_lookups"], from_list([], c["col"]["type"]))):
            for q in lookups:
                if isinstance(q["value"], str):               # a value boxed as another type: answered without a call
                    assert q["expect"] == -1
                    continue
                assert M.find_next(on, q["value"], q["row_start"]).row == q["expect"], (name, q)


def test_model_reproduces_the_join_table():
    """(the cases marked "declined" have two common columns: one key per side cannot state them, so there is nothing to run)"""
    ran = 0
    for c in table("join"):
        if "declined" in c:
            continue
        kind = {"inner": fm.INNER, "outer": fm.OUTER}[c["kind"]]
        left, right = frame_of(c["left"]), frame_of(c["right"])
        r = M.join(left, c["left_key"], right, c["right_key"], kind)
        ran += 1
        if "error" in c:
            assert r == (fm.ERR_TYPE,), c["name"]
            continue
        same_frame(c["name"], r.cols, c["expected"])
        assert r.rows == (len(c["expected"][0]["data"]) if c["expected"] else 0), c["name"]
        if c["left_key"] >= 0:
            rows = M.join_rows(left[c["left_key"]], right[c["right_key"]], kind)
            assert rows.rows == r.rows and len(rows.idx[0]) == len(rows.idx[1]) == r.rows, c["name"]
    assert ran == 14


# ------------------------------------------------------------------ the model against brute force
def small_frames(seed, count, **kw):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        yield rng, fm.gen_frame(rng, int(rng.integers(0, 41)), int(rng.integers(1, 5)), **kw)[0]


def go_equal(typ, a, b):
    """Go's == on two boxed values of a column's type (bits as Python ints)"""
    if typ == INT64:
        return a == b
    x, y = np.uint64(a).view(np.float64).item(), np.uint64(b).view(np.float64).item()
    return x == y


def test_sort_against_sorted_with_a_stable_key():
    for rng, frame in small_frames(1, 300, clean=True):
        n = rows_of(frame)
        key = vals(frame[0]).tolist()
        perm = sorted(range(n), key=lambda i: key[i])        # stable; -0.0 == 0.0 under Python's float order
        r = M.sort_by_col(frame, 0)
        if n < 2 or all(not key[i] < key[i - 1] for i in range(1, n)):
            assert r.unchanged
            continue
        assert M.argsort(frame[0]).idx[0].tolist() == perm
        for c, o in zip(frame, r.cols):
            assert o.bits.tolist() == [c.bits[i] for i in perm] and o.valid.all()
        assert M.take(frame[-1], perm).cols[0].bits.tolist() == r.cols[-1].bits.tolist()
    assert M.take(frame[0], [rows_of(frame)]) == (fm.ERR_ARG,) and M.take(frame[0], [-1]) == (fm.ERR_ARG,)
    nulls = MCol(INT64, np.arange(3, dtype=np.uint64), np.array([True, False, True]))
    assert M.argsort(nulls) == (fm.ERR_SORT_NULLS,) and M.sort_by_col([nulls], 0) == (fm.ERR_SORT_NULLS,)
    assert M.argsort(fm.mcol(np.array([1.0, np.nan, 0.0]))) == (fm.ERR_UNSUPPORTED,)


def test_sharded_sort_is_the_sort_of_the_concatenation():
    for rng, frame in small_frames(2, 200, clean=True):
        cuts = fm.rank_cuts(rng, rows_of(frame))
        one, r = M.sort_by_col(frame, 0), M.sort_by_col_sharded(fm.cut(frame, cuts), 0)
        assert bool(one.unchanged) == bool(r.unchanged)
        if one.unchanged:
            continue
        assert [rows_of(f) for f in r.ranks] == cuts
        assert fm.signature(M, fm.R(cols=fm.concat_frames(r.ranks))) == fm.signature(M, fm.R(cols=one.cols))
        # merged_ranks by its definition: a destination rank takes a run of each source rank; two runs overlap when a later source
        # rank's run starts below an earlier one's end
        key, ends, merged = vals(frame[0]).tolist(), np.cumsum(cuts), 0
        perm = sorted(range(len(key)), key=lambda i: key[i])
        for e, m in zip(ends, cuts):
            src = [int(np.searchsorted(ends, i, side="right")) for i in perm[e - m:e]]
            runs = {s: [key[i] for i, t in zip(perm[e - m:e], src) if t == s] for s in src}
            order = sorted(runs)
            merged += any(runs[a][-1] > runs[b][0] for a, b in zip(order, order[1:]))
        assert r.merged_ranks == merged


def test_filter_drop_nils_and_diff_against_row_loops():
    for rng, frame in small_frames(3, 300, nan_ok=True):
        n, nc = rows_of(frame), len(frame)
        a = fm.args_filter(rng, frame)
        keep = []
        for i in range(n):
            ok = a["and_mask"] is None or bool(a["and_mask"][i])
            for col, values, match_null in a["preds"]:
                c = frame[col]
                hit = any(go_equal(c.typ, int(c.bits[i]), int(v)) for v in np.asarray(values, fm.DTYPE[c.typ]).view(np.uint64)) \
                    if c.valid[i] else match_null
                ok = ok and hit
            keep.append(ok)
        rows = [i for i in range(n) if keep[i]]
        m, r = M.filter_mask(frame, a["preds"], a["and_mask"]), M.filter(frame, a["preds"], a["and_mask"])
        assert m.mask.tolist() == keep and (m.selected, m.first, m.last) == (len(rows), rows[0] if rows else -1, rows[-1] if rows else -1)
        check_rows(frame, rows, r)
        assert fm.signature(M, M.compact(frame, np.array(keep, bool))) == fm.signature(M, r)
        # DropNils
        idx = fm.args_col_idx(rng, frame)
        sel = set(idx) if idx else set(range(nc))
        rows = [i for i in range(n) if all(frame[j].valid[i] for j in sel)]
        check_rows(frame, rows, M.drop_nils(frame, idx))
        v = M.valid_mask(frame, idx)
        assert np.flatnonzero(v.mask).tolist() == rows and v.selected == len(rows)
        # Diff
        d = M.diff(frame, idx)
        assert len(d.cols) == len(sel)
        for j, o, g in zip(sorted(sel), d.cols, d.gen_nan):
            c = frame[j]
            for i in range(n):
                if i == 0 or not (c.valid[i] and c.valid[i - 1]):
                    assert not o.valid[i] and o.bits[i] == 0
                    continue
                assert o.valid[i]
                if c.typ == INT64:
                    assert int(o.bits[i]) == (int(c.bits[i]) - int(c.bits[i - 1])) & ((1 << 64) - 1)
                else:
                    x, y = vals(c)[i].item(), vals(c)[i - 1].item()
                    want = x - y                                  # (Python's float: one IEEE subtraction, inf - inf a NaN)
                    if want != want:
                        assert np.isnan(vals(o)[i]) and bool(g[i]) == (x == x and y == y)
                    else:
                        assert vals(o)[i] == want and np.signbit(vals(o)[i]) == np.signbit(want) and not g[i]
    assert M.drop_nils(frame, [len(frame)]) == (fm.ERR_BAD_COL,) and M.diff(frame, [-1]) == (fm.ERR_BAD_COL,)


def check_rows(frame, rows, r):
    """r (compact's answer) says exactly `rows`"""
    assert r.count == len(rows)
    if not rows or rows[-1] - rows[0] + 1 == len(rows):
        assert r.contiguous and r.cols is None and r.first == (rows[0] if rows else 0)
        return
    assert not r.contiguous
    for c, o in zip(frame, r.cols):
        assert o.valid.tolist() == [bool(c.valid[i]) for i in rows]
        assert o.bits.tolist() == [int(c.bits[i]) if c.valid[i] else 0 for i in rows]
    assert M.compact(frame, np.isin(np.arange(rows_of(frame)), rows), capacity=len(rows) - 1) == (fm.ERR_ARG,)


def test_distinct_and_find_against_a_scan():
    for rng, frame in small_frames(4, 400, nan_ok=False):
        c = frame[0]
        seen = {}                                             # value -> bits of its LAST row (a float key: -0.0 and 0.0 are one)
        for x, b, ok in zip(vals(c).tolist(), c.bits.tolist(), c.valid.tolist()):
            if ok:
                seen[x] = b
        r = M.distinct(c)
        assert r.n_distinct == len(seen)
        if seen:
            assert r.cols[0].bits.tolist() == [seen[x] for x in sorted(seen)] and r.cols[0].valid.all()
            assert M.distinct(c, capacity=len(seen) - 1) == (fm.ERR_ARG,)
        else:
            assert r.cols is None
        for value in [None] + [float("nan")] * (c.typ == FLOAT64) + fm.sample_values(rng, c, 2, misses=False).tolist() + [424242]:
            start = int(rng.integers(0, len(c.bits) + 2))
            want = -1
            for i in range(0 if value is None else start, len(c.bits)):
                if (not c.valid[i]) if value is None else (c.valid[i] and vals(c)[i].item() == fm.DTYPE[c.typ](value).item()):
                    want = i
                    break
            assert M.find_next(c, value, start).row == want
    assert M.distinct(fm.mcol(np.array([1.0, np.nan]))) == (fm.ERR_UNSUPPORTED,)
    assert M.distinct(MCol(FLOAT64, np.array([fm.NAN_BITS, 5], np.uint64), np.array([False, True]))).n_distinct == 1


def test_append_is_concatenation():
    for rng, frame in small_frames(5, 100):
        cuts = fm.rank_cuts(rng, rows_of(frame))
        r = M.append(fm.cut(frame, cuts))
        if len(cuts) == 1:
            assert r.unchanged and r.cols is None
            continue
        assert fm.signature(M, r) == fm.signature(M, fm.R(unchanged=0, cols=[M.out(c.typ, c.bits, c.valid) for c in frame]))
        assert M.append(fm.cut(frame, cuts), capacity=rows_of(frame) - 1) == (fm.ERR_ARG,)
    other = [MCol(INT64 + FLOAT64 - frame[0].typ, frame[0].bits, frame[0].valid)] + frame[1:]
    assert M.append([frame, other]) == (fm.ERR_TYPE,)


def test_join_against_the_double_loop_of_get_common_rows():
    for rng, left in small_frames(6, 300, nan_ok=False):
        right, _, rk = fm.gen_right(rng, left, 0, right_rows=int(rng.integers(0, 30)))
        lk, rkey = left[0], right[rk]
        common = [(l, r) for l in range(len(lk.bits)) for r in range(len(rkey.bits))
                  if (go_equal(lk.typ, int(lk.bits[l]), int(rkey.bits[r])) if lk.valid[l] and rkey.valid[r] else not lk.valid[l] and not rkey.valid[r])]
        for kind in (fm.INNER, fm.OUTER):
            li, ri = [], []
            if kind == fm.INNER:
                li, ri = [p[0] for p in common], [p[1] for p in common]
            else:
                for l in range(len(lk.bits)):
                    mine = [p for p in common if p[0] == l] or [(l, -1)]
                    li += [p[0] for p in mine]
                    ri += [p[1] for p in mine]
                tail = [r for r in range(len(rkey.bits)) if r not in {p[1] for p in common}]
                li, ri = li + [-1] * len(tail), ri + tail
            rows = M.join_rows(lk, rkey, kind)
            assert (rows.rows, rows.pairs) == (len(li), len(common))
            assert rows.idx[0].tolist() == li and rows.idx[1].tolist() == ri
            j = M.join(left, 0, right, rk, kind)
            assert len(j.cols) == len(left) + len(right) - 1
            for o, (c, idx) in zip(j.cols, [(c, li) for c in left] + [(c, ri) for i, c in enumerate(right) if i != rk]):
                for row, i in enumerate(idx):
                    src, at = (c, i) if i >= 0 or o is not j.cols[0] else (rkey, ri[row])      # a right-only row: the right key
                    ok = at >= 0 and bool(src.valid[at])
                    assert (bool(o.valid[row]), int(o.bits[row])) == (ok, int(src.bits[at]) if ok else 0)
            if len(li):
                assert M.join(left, 0, right, rk, kind, capacity=len(li) - 1) == (fm.ERR_ARG,)
        none = M.join(left, -1, right, -1, fm.OUTER)
        assert none.rows == rows_of(left) + rows_of(right) and len(none.cols) == len(left) + len(right) and none.pairs == 0
        assert M.join(left, -1, right, -1, fm.INNER).rows == 0
    a, b = fm.mcol(np.array([1.0, np.nan])), fm.mcol(np.array([1.0]))
    assert M.join_rows(a, b, fm.INNER) == M.join_rows(b, a, fm.OUTER) == (fm.ERR_UNSUPPORTED,)
    assert M.join_rows(b, fm.mcol(np.array([1])), fm.INNER) == (fm.ERR_TYPE,)
    hidden = MCol(FLOAT64, np.array([fm.NAN_BITS, 5], np.uint64), np.array([False, True]))      # a NaN under a null is no key
    assert M.join_rows(hidden, hidden, fm.INNER).pairs == 2


# ------------------------------------------------------------------ what the plans cover
@pytest.fixture(scope="module")
def planned():
    """every step of the default seeds: [(seed, step)], and the chains"""
    steps, chains = [], []
    for seed in DEFAULT_SEEDS:
        for kind, p in fm.plans(seed):
            steps += [(seed, s) for s in ([p] if kind == "op" else p["steps"])]
            if kind == "chain":
                chains.append(p)
    return steps, chains


def test_plans_are_a_function_of_the_seed():
    a, b = [[fm.signature(M, s["expect"]) for k, p in fm.plans(5) for s in ([p] if k == "op" else p["steps"])] for _ in range(2)]
    assert a == b


def test_coverage_conditions_of_the_plans(planned):
    steps, chains = planned
    tags = Counter(t for _, s in steps for t in s["tags"])
    for op in fm.ENTRY_POINTS:
        assert tags["op:" + op] >= 40, (op, tags["op:" + op])
    kinds = Counter(s["decline"] for _, s in steps if s.get("decline"))
    for kind in fm.DECLINES:
        assert kinds[kind] >= 3, (kind, kinds)
    n_declined = sum(declined(s["expect"]) for _, s in steps)
    assert n_declined <= 0.15 * len(steps), (n_declined, len(steps))
    assert tags["contiguous"] >= 10 and tags["fed by contiguous"] >= 5 and tags["fed by unchanged"] >= 3, tags
    assert sum(c["complete"] for c in chains) >= 0.6 * len(chains), (sum(c["complete"] for c in chains), len(chains))
    assert all(3 <= c["length"] <= 6 for c in chains) and len(chains) == fm.CHAINS * len(DEFAULT_SEEDS)
    five = ["join null keys both sides kind %d" % fm.INNER, "join null keys both sides kind %d" % fm.OUTER, "distinct both zeros",
            "diff generates NaN", "sharded merge", "third launch group"]
    five += ["offset:%d" % o for o in fm.OFFSETS]
    # a residency triple: where the first column of a call's first frame lies, where the last column of its last frame lies, and
    # where its outputs go
    five += ["res:%d%d%d" % (a, b, c) for a in fm.RESIDENCIES for b in fm.RESIDENCIES for c in fm.RESIDENCIES]
    for t in five:
        assert tags[t] >= 5, (t, tags[t])
    for _, s in steps:      # a plan can be laid out in memory: a column without a bitmap has no nulls, frames are rectangular
        for f in s["inputs"]:
            assert len({len(c.bits) for c in f["cols"]} | {len(c.valid) for c in f["cols"]}) <= 1
            assert f["phys"] is None or all(p["bitmap"] or c.valid.all() for c, p in zip(f["cols"], f["phys"])), s["op"]
    sizes = Counter(rows_of(f) for _, s in steps for f in s["frames"])
    assert all(sizes[n] for n in fm.ROW_COUNTS) and sizes[fm.BIG_ROWS] >= 1
    assert max(Counter(seed for seed, s in steps if any(rows_of(f) == fm.BIG_ROWS for f in s["frames"])).values()) == 1


# ------------------------------------------------------------------ sensitivity: a model that is wrong in one way is seen
class UnstableSort(fm.Model):
    def order(self, c):
        v = vals(c)
        return np.lexsort((-np.arange(len(v)), v + 0.0 if c.typ == FLOAT64 else v))       # ties in reverse row order


class FirstZeroSurvives(fm.Model):
    def distinct_survivor(self, perm, heads):
        return perm[heads]


class NullSlotsKeepTheirPayload(fm.Model):
    def settle(self, bits, valid):
        return MCol(None, bits, valid)


class RightRowsDescending(fm.Model):
    def right_rows(self, rows):
        return rows[::-1]


class RightOnlyNullKeyBecomesZero(fm.Model):
    def right_only_key(self, bits, valid):
        return bits, np.ones(len(valid), bool)


class FindNilHonoursRowStart(fm.Model):
    def nil_search_start(self, row_start):
        return row_start


class RepeatedIndicesCancel(fm.Model):
    """a repeated index is counted twice and so drops out; when none is left the call is taken for n_idx == 0: every column"""
    def select_cols(self, ncols, col_idx):
        if any(i < 0 or i >= ncols for i in col_idx):
            return (fm.ERR_BAD_COL,)
        odd = sorted(i for i, k in Counter(col_idx).items() if k % 2)
        return odd or list(range(ncols))


class NanInTheSetMatchesNan(fm.Model):
    def equal(self, v, x):
        return (v == x) | ((v != v) & (x != x))


class PaddingBitsSet(fm.Model):
    def pack(self, valid):
        b = fm.Model.pack(self, valid)
        if len(valid) % 8:
            b[-1] |= (0xFF << (len(valid) % 8)) & 0xFF
        return b


MUTANTS = [UnstableSort, FirstZeroSurvives, NullSlotsKeepTheirPayload, RightRowsDescending, RightOnlyNullKeyBecomesZero,
           FindNilHonoursRowStart, RepeatedIndicesCancel, NanInTheSetMatchesNan, PaddingBitsSet]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_a_wrong_model_is_seen_in_every_block_of_eight_seeds(planned, mutant):
    steps, _ = planned
    wrong = mutant()
    for block in range(0, len(DEFAULT_SEEDS), 8):
        seen = None
        for seed, s in steps:
            if block <= seed < block + 8 and fm.signature(wrong, fm.run_step(wrong, s)) != fm.signature(M, s["expect"]):
                seen = (seed, s["op"])
                break
        assert seen is not None, "seeds %d..%d would not notice %s" % (block, block + 7, mutant.__name__)
