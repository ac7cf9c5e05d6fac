"""tests/whole_model.py without a GPU: the proof that the model may stand in for the oracle where tests/test_gpu_whole_fuzz.py uses it.
(a) the reference's own vectors (tests/golden) and every seeded case against the oracle, bit for bit, Sum and the integrals included (the
oracle runs the same left-to-right loop).  The cases are cut to their first ORACLE_ROWS = 1 500 rows: the oracle counts Mode's
occurrences again from row 0 for every row and walks to the next valid point from every row, both O(n^2) - 1 500 rows keep a case at a
few milliseconds and the file at seconds; medium frames (20 000 rows, i.i.d. nulls, no Mode) check the index arithmetic beyond that.
(b) what the cases of the default seeds cover, asserted: a fuzz that silently misses a shape hides failures.  (c) deliberately wrong
models, each of which the default seeds must tell from the right one: a kernel wrong in that way would be seen.  (d) the integer-exact
class - at least a third of the order-sensitive comparisons, so that the bound cannot hide a failure there - and, for the rest, that
the reference's own result lies within the bound of the exact value: the bound can never reject the reference."""
from collections import Counter

import numpy as np
import pytest

import whole_model as wm
from bow_amd import capi
from interp_model import go_f64_to_i64
from oracle import pyoracle as orc
from whole_model import FLOAT64, INT64, M, MCol

DEFAULT_SEEDS = range(64 // 2)          # test_gpu_whole_fuzz.SEEDS without BOW_FUZZ_SEEDS
ORACLE_ROWS = 1500
AT_LEAST = 3                            # occurrences of every shape over the default seeds


def same(label, res, want):
    """a Res against an oracle Column: type, length, validity, the slot's bits (but the payload of a NaN both sides computed)"""
    assert res.typ == want.type and res.length == want.length, (label, res.typ, want.type, res.length, want.length)
    if res.length == 0:
        return
    assert res.valid == bool(want.valid_mask()[0]), (label, res.valid)
    if res.valid:
        w = want.values[:1].view(np.uint64)[0]
        if res.bits != w:
            assert res.typ == FLOAT64 and np.isnan(res.as_float()) and np.isnan(want.values[0]), (label, hex(int(res.bits)), hex(int(w)))


@pytest.fixture(scope="module")
def drawn():
    return [c for seed in DEFAULT_SEEDS for c in wm.cases(seed)]


@pytest.fixture(scope="module")
def results(drawn):
    """[(case, [Res])] of the cases inside the domain, full size"""
    return [(c, M.aggregate(wm.mcols(c), 0, c["aggs"])) for c in drawn if wm.outside(c) is None]


# ------------------------------------------------------------------ (a) golden vectors and the oracle
def test_cases_are_a_function_of_the_seed():
    a, b = [[(c["label"], [col[0].tobytes() for col in c["cols"]], repr(c["aggs"])) for c in wm.cases(5)] for _ in range(2)]
    assert a == b


def test_model_reproduces_the_golden_vectors(golden):
    for v in golden["whole"]:
        cols = []
        for data, typ in ((v["time"], INT64), (v["value"], FLOAT64)):
            valid = np.array([x is not None for x in data], bool)
            cols.append(MCol(np.array([0 if x is None else x for x in data], np.int64 if typ == INT64 else np.float64), valid, typ))
        aggs = [(a.split(":")[0], 0 if a.split(":")[1] == "time" else 1) for a in v["aggs"]]
        for a, r, exp in zip(aggs, M.aggregate(cols, 0, aggs), v["expect"]):
            got = [] if r.length == 0 else [None if not r.valid else r.as_int() if r.typ == INT64 else float(r.as_float())]
            assert got == exp, (v.get("name"), a, got, exp)


def test_cases_against_the_oracle(drawn):
    ran = Counter()
    for c in drawn:
        if wm.outside(c) is not None:
            continue
        c = wm.cut(c, ORACLE_ROWS)
        got = M.aggregate(wm.mcols(c), 0, c["aggs"])
        want = orc.aggregate_whole(wm.ocols(c), 0, c["aggs"])
        for a, g, w in zip(c["aggs"], got, want):
            same("%s %r" % (c["label"], a), g, w)
            ran[a[0]] += 1
    assert min(ran[k] for k in wm.KINDS) >= 100, ran


def test_medium_frames_against_the_oracle():
    rng = np.random.default_rng(91)
    kinds = [k for k in wm.KINDS if k != "Mode"]
    for i in range(6):
        n = 20_000 - i
        ts = wm.draw_ts(rng, n, wm.TS_KINDS[i % 4])
        valid = rng.random(n) >= [0.05, 0.3, 0.6][i % 3]
        for typ in (FLOAT64, INT64):
            v = wm.draw_values(rng, n, typ, ["normal", "int-exact", "special", "full"][i % 4] if typ == FLOAT64 or i % 2 else "full", 0)
            if typ == INT64:
                v = v.astype(np.int64) if v.dtype != np.int64 else v
            aggs = [(k, 1) for k in kinds] + [("Sum", 1, [0.1, -3.0]), ("Count", 1, [0.5]), ("First", 1, [1e-3]), ("WindowStart", 0, [0.5])]
            got = M.aggregate([MCol(ts, np.ones(n, bool), INT64), MCol(v, valid, typ)], 0, aggs)
            want = orc.aggregate_whole([orc.Column(ts, None, orc.INT64), orc.Column(v, np.packbits(valid, bitorder="little"), typ, 0, n)], 0, aggs)
            for a, g, w in zip(aggs, got, want):
                same("medium %d type=%d %r" % (i, typ, a), g, w)


def test_mode_of_a_small_mixed_frame():
    """mode.go by hand: -0 and +0 are one key and the row that REACHES the count is returned; NaNs never count up"""
    nan = float("nan")
    for vals, expect in (([0.0, -0.0, 1.0, 1.0], -0.0), ([nan, nan, nan, 2.0], nan), ([1.0, 2.0, 2.0, 1.0], 2.0), ([nan, 3.0, nan, 3.0], 3.0)):
        v = np.array(vals)
        r = M.aggregate([MCol(np.arange(len(v)), np.ones(len(v), bool), INT64), MCol(v, np.ones(len(v), bool), FLOAT64)], 0, [("Mode", 1)])[0]
        assert r.valid and (r.bits == wm.f2b(expect) or (np.isnan(expect) and r.bits == v[:1].view(np.uint64)[0])), (vals, r.as_float())


# ------------------------------------------------------------------ (b) what the cases cover
def test_coverage_of_the_default_seeds(drawn):
    tags = Counter()
    kinds_by_type = Counter()
    for c in drawn:
        out = wm.outside(c)
        assert (out is not None) == (c["decline"] is not None), c["label"]
        if out is not None:
            tags["decline " + c["decline"]] += 1
            continue
        n = c["n"]
        tags["rows %d" % n] += n in wm.SMALL + wm.MULTI + (wm.LARGE,)
        tags["random size below 3000"] += 0 < n < 3000 and n not in wm.SMALL
        tags["empty frame"] += n == 0
        if n == 0:
            continue
        for t in c["tags"]:
            tags[t] += 1
        nblocks, chunk = capi.whole_layout(n)
        blocks, quarters, steps = wm.edges(n)
        for (buf, bm, typ, off, valid), layout in zip(c["cols"][1:], c["layouts"]):
            rows = np.flatnonzero(valid)
            wg = rows // chunk
            # the planted layouts are what they say, by the kernel's own arithmetic
            if layout == "two-ends":
                assert list(wg) == [0, (n - 1) // chunk] and nblocks > 1, c["label"]
            if layout == "one-workgroup":
                assert len(set(wg)) == 1 and nblocks > 1, c["label"]
            if layout == "gap-blocks":
                assert (np.diff(wg) >= 3).any(), c["label"]
            if layout == "tail-nulls":
                assert n - 1 - rows[-1] > chunk, c["label"]
            if layout == "head-nulls":
                assert rows[0] > chunk, c["label"]
            for name, at in (("edge-block", blocks), ("edge-quarter", quarters), ("edge-step", steps)):
                if layout == name:
                    assert any(valid[r - 1] and valid[r] for r in at), c["label"]
                    tags[name + ", these two points only"] += len(rows) == 2
            tags["pair across two or more empty workgroups"] += bool(len(wg) > 1 and (np.diff(wg) >= 3).any())
            tags["arrow offset"] += off > 0
            tags["Int64 beyond 2^53"] += typ == INT64 and len(rows) > 0 and bool((np.abs(buf[off:off + n][rows].astype(np.float64)) > 2.0 ** 53).any())
        tags["null_count stated"] += any(s and col[1] is not None for s, col in zip(c["stated"], c["cols"]))
        tags["null_count -1"] += any(not s and col[1] is not None for s, col in zip(c["stated"], c["cols"]))
        tags["inputs " + c["residency"]] += 1
        tags["outputs " + ("device" if c["out_device"] else "host")] += 1
        tags["%d value columns" % (len(c["cols"]) - 1)] += 1
        per_col = Counter(a[1] for a in c["aggs"] if a[0] != "Mode")
        tags["more than 16 streaming reducers on one column"] += max(per_col.values(), default=0) > 16
        tags["64 reducers"] += len(c["aggs"]) == 64
        tags["Mode next to streaming reducers"] += len({a[0] == "Mode" for a in c["aggs"]}) == 2
        tags["interval column as a value column"] += any(a[1] == 0 and a[0] in ("First", "Last", "Mode", "Sum") for a in c["aggs"])
        tags["WindowStart over Float64"] += any(a[0] == "WindowStart" and c["cols"][a[1]][2] == FLOAT64 for a in c["aggs"])
        for a in c["aggs"]:
            typ = c["cols"][a[1]][2]
            kinds_by_type[a[0], typ] += 1
            if len(a) > 2:
                is_int = a[0] == "Count" or (a[0] in ("First", "Last", "Mode", "WindowStart") and typ == INT64)
                tags["Factor on an %s result" % ("Int64" if is_int else "Float64")] += 1
        ts = c["cols"][0][0][c["cols"][0][3]:][:n]
        for (buf, bm, typ, off, valid) in c["cols"][1:]:
            rows = np.flatnonzero(valid)
            tags["frame ends in nulls, IntegralStep asked"] += bool(len(rows) and rows[-1] < n - 1 and ts[rows[-1]] != ts[n - 1]
                                                                    and any(a[0] in ("IntegralStep", "WeightedAverageStep") for a in c["aggs"]))
        tags["nanosecond divisor"] += "ns" in c["tags"] and any(a[0].startswith("Weighted") for a in c["aggs"])
    want = ["rows %d" % n for n in wm.SMALL + wm.MULTI + (wm.LARGE,)] + ["random size below 3000", "empty frame"] + list(wm.LAYOUTS) + list(wm.TS_KINDS)
    want += ["f64 " + k for k in wm.F_KINDS] + ["i64 " + k for k in wm.I_KINDS] + ["decline " + d for d in wm.DECLINES]
    want += [e + ", these two points only" for e in ("edge-block", "edge-quarter", "edge-step")]
    want += ["pair across two or more empty workgroups", "arrow offset", "Int64 beyond 2^53", "null_count stated", "null_count -1", "inputs host",
             "inputs pinned", "inputs device", "outputs host", "outputs device", "1 value columns", "2 value columns", "3 value columns",
             "more than 16 streaming reducers on one column", "64 reducers", "Mode next to streaming reducers", "interval column as a value column",
             "WindowStart over Float64", "Factor on an Int64 result", "Factor on an Float64 result", "frame ends in nulls, IntegralStep asked",
             "nanosecond divisor"]
    for t in want:
        assert tags[t] >= AT_LEAST, (t, tags[t], sorted(tags.items()))
    for k in wm.KINDS:
        for typ in (INT64, FLOAT64):
            assert kinds_by_type[k, typ] >= AT_LEAST, (k, typ)


def test_at_most_a_tenth_of_a_seed_lies_outside_the_domain(drawn):
    per_seed = Counter(c["seed"] for c in drawn if wm.outside(c) is not None)
    assert max(per_seed.values()) <= 0.1 * wm.CASES, per_seed
    assert sum(per_seed.values()) >= len(wm.DECLINES), per_seed


# ------------------------------------------------------------------ (c) a model that is wrong in one way is seen
class PairWithTheNextRow(wm.Model):
    def pairs(self, rows):
        a = np.flatnonzero(np.diff(rows) == 1)
        return a, a + 1


class LastStepTermDropped(wm.Model):
    def step_tail(self, v_last, dt_last):
        return np.float64(0.0)


class LastValueFromTheLastValidRow(wm.Model):
    def last_value_row(self, n, valid):
        hits = np.flatnonzero(valid)
        return int(hits[-1]) if hits.size else n - 1


class NaNSeedSkipped(wm.Model):
    def seed_sticks(self, seed):
        return False


class LaterOfEqualExtremes(wm.Model):
    def extreme_of_equals(self, hits):
        return hits[-1]


class FirstFromRowZero(wm.Model):
    def first_row(self, valid):
        return 0


class MeanOverAllRows(wm.Model):
    def mean_divisor(self, count, n):
        return n


class Int64ThroughADouble(wm.Model):
    def own_bits(self, col, row):
        if col.typ != INT64:
            return super().own_bits(col, row)
        return go_f64_to_i64(col.values[row:row + 1].astype(np.float64)).view(np.uint64)[0]


class WindowStartOverFloat64Valid(wm.Model):
    def strict(self, typ, is_int):
        return True


class ModeTiesToTheLast(wm.Model):
    def mode_row(self, at_max):
        return at_max[-1]


class FactorWithoutTruncation(wm.Model):
    def factor_int(self, x, f):
        with np.errstate(all="ignore"):
            return int(go_f64_to_i64(np.round(np.float64(x) * np.float64(f))))


MUTANTS = [PairWithTheNextRow, LastStepTermDropped, LastValueFromTheLastValidRow, NaNSeedSkipped, LaterOfEqualExtremes, FirstFromRowZero,
           MeanOverAllRows, Int64ThroughADouble, WindowStartOverFloat64Valid, ModeTiesToTheLast, FactorWithoutTruncation]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_a_wrong_model_is_seen_by_the_default_seeds(drawn, results, mutant):
    """... in at least AT_LEAST cases, and by the GPU test's own comparison: bits, or the bound where the bound is what it asserts"""
    wrong, seen = mutant(), []
    for c, right in results:
        if c["n"] == 0 or c["n"] > 70_001 or len(seen) >= AT_LEAST:          # (keeps this test at a second)
            continue
        for a, g, w in zip(c["aggs"], wrong.aggregate(wm.mcols(c), 0, c["aggs"]), right):
            if differs(a, g, w):
                seen.append(c["label"])
                break
    assert len(seen) >= AT_LEAST, "the default seeds would not notice %s: %r" % (mutant.__name__, seen)


def differs(a, got, want):
    """what tests/test_gpu_whole_fuzz.py asserts, as a predicate: got is a Res here, a device result there"""
    if (got.typ, got.length, got.valid) != (want.typ, want.length, want.valid):
        return True
    if not want.valid or got.bits == want.bits:
        return False
    if a[0] not in wm.ORDER_SENSITIVE or want.int_exact:
        return not (want.typ == FLOAT64 and np.isnan(got.as_float()) and np.isnan(want.as_float()) and a[0] in wm.ORDER_SENSITIVE)
    g, e = got.as_float(), want.exact
    if not (np.isfinite(g) and np.isfinite(e)):
        return not ((np.isnan(g) and np.isnan(e)) or g == e)
    return abs(g - e) > wm.bound(want, a[0], a[2] if len(a) > 2 else [])


# ------------------------------------------------------------------ (d) the integer-exact class and the bound
def test_integer_exact_share_and_the_reference_within_the_bound(results):
    exact = rest = 0
    for c, res in results:
        for a, r in zip(c["aggs"], res):
            if a[0] not in wm.ORDER_SENSITIVE or not r.valid:
                continue
            ref = r.as_float()
            if r.int_exact:
                exact += 1
                if not a[2:]:
                    assert ref == r.exact, (c["label"], a, ref, r.exact)          # every order gives the same bits: so does the reference's
                continue
            rest += 1
            if np.isfinite(ref) and np.isfinite(r.exact):
                b = wm.bound(r, a[0], a[2] if len(a) > 2 else [])
                assert abs(ref - r.exact) <= b, (c["label"], a, ref, r.exact, b)
            else:
                assert (np.isnan(ref) and np.isnan(r.exact)) or ref == r.exact, (c["label"], a, ref, r.exact)
    assert exact >= (exact + rest) / 3 and rest >= (exact + rest) / 3, (exact, rest)
