"""tests/interp_model.py without a GPU: the proof that the model may stand in for the oracle where tests/test_gpu_interp_fuzz.py uses
it.  (a) every seeded case of at most 700 rows against the oracle, bit for bit - each interpolator, both window kinds, the four fills,
the chain; (b) medium sizes the oracle can still afford (20 000 rows at 30 % i.i.d. nulls, 5 000 rows around one run of 2 100 nulls),
so that the vectorised index arithmetic is checked across many windows and trips; (c) the reference's own vectors (tests/golden);
(d) the coverage conditions of the cases the GPU test runs by default - a fuzz that silently misses a shape hides failures, so they
are asserted - and the share of cases outside the device path's documented domain; (e) deliberately wrong models, each of which the
cases of the first eight seeds must tell from the right one: a kernel wrong in that way would be seen."""
import json
import os
from collections import Counter

import numpy as np
import pytest

import interp_model as im
from interp_model import FLOAT64, INT64, M, MCol
from oracle import pyoracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_vectors.json")
DEFAULT_SEEDS = range(64 // 2)          # test_gpu_interp_fuzz.SEEDS without BOW_FUZZ_SEEDS
KINDS = ("Linear", "StepPrevious", "None")
T = {"float64": FLOAT64, "int64": INT64}


def same(label, got, want):
    """an MCol against an oracle Column: tests/test_gpu_callers.cmp_out's comparison - lengths, validity, the bits of the valid values
    except the payload of a NaN both sides generated"""
    assert len(got.values) == want.length, (label, len(got.values), want.length)
    wm = want.valid_mask()
    assert np.array_equal(got.valid, wm), (label, np.flatnonzero(got.valid != wm)[:10])
    g, w = got.values[wm], want.values[:want.length][wm]
    diff = g.view(np.uint64) != w.view(np.uint64)
    if diff.any() and g.dtype == np.float64:
        diff &= ~(np.isnan(g) & np.isnan(w))
    assert not diff.any(), (label, np.flatnonzero(diff)[:10])


def interp_both(label, case, interps, inclusive):
    got = M.interpolate(case["ts"], im.mcols(case), case["interval"], interps, offset=case["offset"], inclusive=inclusive)
    want = orc.interpolate(im.ocols(case), 0, case["interval"], interps, offset=case["offset"], inclusive=inclusive)
    for k, (g, w) in enumerate(zip(got, want)):
        same("%s col %d" % (label, k), g, w)


def fills_both(label, col, ocol):
    for method in ("Previous", "Next", "Mean"):
        (g, gu), (w, wu) = M.fill(col, method), orc.fill(ocol, method)
        assert gu == wu, (label, method)
        same("%s Fill%s" % (label, method), g, w)


def fill_linear_both(label, ref, col, ocols_):
    r = M.fill_linear(ref, col)
    try:
        w, wu = orc.fill_linear(ocols_, 1, 0)
    except orc.OracleError as e:
        assert r == (e.code,), label
        return
    assert r[1] == wu, label
    same(label + " FillLinear", r[0], w)


@pytest.fixture(scope="module")
def drawn():
    """every case of the default seeds, by kind: [(seed, case)]"""
    return {kind: [(seed, c) for seed in DEFAULT_SEEDS for c in im.cases(seed, kind)] for kind in im.CASES}


# ------------------------------------------------------------------ (a) the small cases against the oracle
def test_cases_are_a_function_of_the_seed():
    a, b = [[(c["label"], c["ts"].tobytes() if "ts" in c else b"", [r[1].tobytes() if r[1] is not None else b"" for r in c["raw"]])
             for kind in im.CASES for c in im.cases(5, kind)] for _ in range(2)]
    assert a == b


def test_small_cases_against_the_oracle(drawn):
    ran = Counter()
    for kind in ("interp", "chain"):
        for _seed, c in drawn[kind]:
            if c["n"] > 700:
                continue
            interp_both(c["label"], c, c["interps"], c["inclusive"])
            ran[kind] += 1
            # ... and each interpolator on every value column, under both window kinds
            for k in KINDS:
                ip = [dict(i_, kind=k) if j else i_ for j, i_ in enumerate(c["interps"])]
                for inclusive in (False, True):
                    interp_both("%s all %s incl=%d" % (c["label"], k, inclusive), c, ip, inclusive)
            if kind == "chain":
                got, gnic = M.interpolate_aggregate(c["ts"], im.mcols(c), c["interval"], c["interps"], c["aggs"], offset=c["offset"], inclusive=c["inclusive"])
                mid = orc.interpolate(im.ocols(c), 0, c["interval"], c["interps"], offset=c["offset"], inclusive=c["inclusive"])
                want, wnic = orc.aggregate(mid, 0, c["interval"], c["aggs"], offset=c["offset"], inclusive=c["inclusive"])
                assert gnic == wnic, c["label"]
                for a, g, w in zip(c["aggs"], got, want):
                    same("%s %s" % (c["label"], a[0]), MCol(g.values[:g.length], g.valid_mask(), g.type), w)
    for _seed, c in drawn["fill"]:
        if c["n"] > 700:
            continue
        fills_both(c["label"], im.mcols(c)[0], im.ocols(c)[0])
        fill_linear_both(c["label"], im.ref_mcol(c), im.mcols(c)[0], im.ocols(c))
        ran["fill"] += 1
    assert min(ran["interp"], ran["chain"], ran["fill"]) >= 40, ran


# ------------------------------------------------------------------ (b) medium sizes the oracle can afford
def medium_frames():
    """(label, ts, interval, offset, values, valid, type): 20 000 rows at 0 .. 30 % i.i.d. nulls over thousands of windows, and 5 000 rows
    around one null run of up to 2 100 rows with a few dozen window starts inside it (the oracle walks the run from each of them)"""
    rng = np.random.default_rng(77)
    for i in range(6):
        n = 20_000 - i
        ts = (np.cumsum(rng.integers(0, 9, n)) - int(rng.integers(0, 40_000))).astype(np.int64)
        valid = rng.random(n) >= [0.0, 0.05, 0.3][i % 3]
        yield "iid %d" % i, ts, int([3, 10, 64][i % 3]), int(rng.integers(-100, 100)), valid
    for i in range(4):
        n = 5_000 - i
        ts = (np.cumsum(rng.integers(0, 5, n)) - int(rng.integers(0, 5_000))).astype(np.int64)
        valid = rng.random(n) >= 0.1
        run = int(rng.integers(2049, 2101))
        a = int(rng.integers(1, n - run))
        valid[a:a + run] = False
        yield "run %d" % i, ts, int(rng.integers(150, 250)), int(rng.integers(-100, 100)), valid


def test_medium_sizes_against_the_oracle():
    rng = np.random.default_rng(78)
    for label, ts, interval, offset, valid in medium_frames():
        n = len(ts)
        for typ in (FLOAT64, INT64):
            v = np.round(rng.standard_normal(n) * 100, 2) if typ == FLOAT64 else rng.integers(-2 ** 62, 2 ** 62, n).astype(np.int64)
            col, ocol = MCol(v, valid, typ), orc.Column(v, np.packbits(valid, bitorder="little"), typ, 0, n)
            octs = orc.Column(ts, None, orc.INT64)
            for kind in ("Linear", "StepPrevious"):
                ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1, "prev": (float(ts[0] - 3), True, 42.5, True, 42)}]
                for inclusive in (False, True):
                    got = M.interpolate(ts, [col], interval, ip, offset=offset, inclusive=inclusive)
                    want = orc.interpolate([octs, ocol], 0, interval, ip, offset=offset, inclusive=inclusive)
                    for k in range(2):
                        same("%s %s type=%d incl=%d col %d" % (label, kind, typ, inclusive, k), got[k], want[k])
            if label.startswith("iid"):      # (the oracle's fills walk from every null ROW: the long run is for Interpolate alone)
                fills_both(label, col, ocol)
                ref = MCol(ts, rng.random(n) >= 0.1, INT64)
                fill_linear_both(label, ref, col, [ocol, orc.Column(ts, np.packbits(ref.valid, bitorder="little"), orc.INT64, 0, n)])


# ------------------------------------------------------------------ (c) the reference's own vectors
def from_list(data, typ):
    valid = np.array([x is not None for x in data], bool)
    return MCol(np.array([0 if x is None else x for x in data], np.int64 if typ == INT64 else np.float64), valid, typ)


def to_list(c):
    return [(int(v) if c.typ == INT64 else float(v)) if ok else None for v, ok in zip(c.values, c.valid)]


def test_model_reproduces_the_golden_vectors():
    with open(GOLDEN) as f:
        golden = json.load(f)
    for v in golden["interpolate"]:
        ip = [{"kind": "Const", "col": i, "const": float(s.split(":")[1])} if s.startswith("Const:") else {"kind": s, "col": i}
              for i, s in enumerate(v["interps"])]
        out = M.interpolate(np.array(v["time"], np.int64), [from_list(v["value"], FLOAT64)], v["interval"], ip, offset=v["offset"])
        assert to_list(out[0]) == v["expect_time"] and to_list(out[1]) == v["expect_value"], v["name"]
    names = ["a", "b", "c", "d", "e"]
    bow = lambda typ: [from_list([None if x is None else (float(x) if typ == FLOAT64 else x) for x in golden["fill_bow"][n]], typ) for n in names]
    for v in golden["fill_linear"]:
        cols = bow(T[v["type"]])
        r = M.fill_linear(cols[names.index(v["ref"])], cols[names.index(v["fill"])])
        if v.get("error"):
            assert r == (-8,), v["name"]
            continue
        assert not r[1] and to_list(r[0]) == v["expect"], v["name"]
    m = golden["fill_linear_meta"]
    r = M.fill_linear(from_list(m["ref"], T[m["ref_type"]]), from_list(m["fill"], T[m["fill_type"]]))
    assert to_list(r[0]) == m["expect"]
    ran = 0
    for typ, methods in golden["fill_methods"].items():
        for method, expect in methods.items():
            for name, col in zip(names, bow(T[typ])):
                out, unchanged = M.fill(col, method)
                assert not unchanged and to_list(out) == expect[name], (typ, method, name)
                ran += 1
    assert ran == 30
    out, unchanged = M.fill(from_list([1, 2, 3], INT64), "Mean")
    assert unchanged and to_list(out) == [1, 2, 3]


# ------------------------------------------------------------------ (d) what the cases cover
class Probe(im.Model):
    """the model, counting what its steps were made of"""

    def __init__(self):
        self.tags = Counter()

    def note(self, **f):
        self.tags["PrevRow used"] += f.get("prev_row_used", 0) > 0
        self.tags["FillLinear row skipped for a null ref"] += f.get("skipped_for_a_null_ref", 0) > 0
        self.tags["FillLinear division by zero"] += f.get("ref_ties", 0) > 0
        if "mean" in f and f["is_int"]:
            x = f["mean"]
            self.tags["FillMean tie, away from zero differs from to even"] += bool((im.c_round(x) != np.round(x)).any())
        if "linear" in f:
            L = f["linear"]
            ok = L["ok"]
            self.tags["previous point beyond 2048 rows"] += bool((ok & (L["back"] > im.NEAR_BITS + 64)).any())
            self.tags["next point beyond 2048 rows"] += bool((ok & (L["ahead"] > im.NEAR_BITS + 64)).any())
            self.tags["Linear division by zero"] += bool((ok & (L["t2"] == L["t0"])).any())
            r = L["r"][ok & np.isfinite(L["r"])]
            self.tags["Int64 Linear result not an integer"] += bool(L["is_int"] and (r != np.trunc(r)).any())


def longest_run_of(flags):
    if not flags.any():
        return 0
    edges = np.flatnonzero(np.diff(np.concatenate(([0], flags.astype(np.int8), [0]))))
    return int((edges[1::2] - edges[::2]).max())


def test_coverage_conditions_of_the_cases(drawn):
    P = Probe()
    tags = P.tags
    for kind in ("interp", "chain"):
        for _seed, c in drawn[kind]:
            ts, n = c["ts"], c["n"]
            assert (np.diff(ts) >= 0).all() and len(ts) == n and all(len(r[4]) == n for r in c["raw"]), c["label"]
            assert [i_["col"] for i_ in c["interps"]] == list(range(1 + len(c["raw"]))) and c["interps"][0]["kind"] == "WindowStart"
            if im.outside(c):
                tags["outside " + kind] += 1
                continue
            P.interpolate(ts, im.mcols(c), c["interval"], c["interps"], offset=c["offset"], inclusive=c["inclusive"])
            w = M.windows(ts, c["interval"], c["offset"], c["inclusive"])
            for (v, bm, typ, off, valid, mode), ip in zip(c["raw"], c["interps"][1:]):
                tags["%s %s %s" % (ip["kind"], "Int64" if typ == INT64 else "Float64", "inclusive" if c["inclusive"] else "exclusive")] += kind == "interp"
                tags["null run across a 4096-bit edge of the bitmap"] += im.run_crosses_a_block_edge(valid, off)
                tags["validity " + mode] += 1
                tags["column without a bitmap"] += bm is None
            per_trip = np.bincount(w.first_index[w.synthetic] // im.TRIP, minlength=1) + im.TRIP
            tags["trip with more than 768 outputs"] += bool((per_trip > im.STAGE_OUTPUTS).any()) and n > im.TRIP
            tags["more than 4096 empty windows in a row"] += longest_run_of(w.length == 0) > im.GAP_LIST
            tags["rows below s0 ride in window 0"] += int(ts[0]) < w.s0 and im.rows_below_s0_ride(ts, c["interval"], c["offset"])
            tags["rows below s0 are dropped"] += int(ts[0]) < w.s0 and not im.rows_below_s0_ride(ts, c["interval"], c["offset"])
            tags["the -1 sentinel"] += bool(((w.start == -1) & (w.length == 0)).any())
            tags["duplicates on a window start"] += bool((w.length[~w.synthetic] > 1).any() and
                                                         (ts[np.minimum(w.begin[~w.synthetic] + 1, n - 1)] == w.start[~w.synthetic]).any())
            tags["nanosecond scale"] += "ns" in c["tags"]
            tags["a trip spans 2^31"] += bool((im.trip_figures(ts, w.s0, c["interval"])[0] >= 2 ** 31).any()) if int(ts[0]) >= w.s0 else False
            tags["device-resident"] += c["device"]
            tags["null_count stated"] += any(c["stated"])
            tags["arrow offset"] += c["pad"] > 0
            tags["%d columns" % len(c["raw"])] += 1
            tags["rows %s" % ("<= 512" if n <= 512 else "<= 4097" if n <= 4097 else "> 4097")] += 1
    for _seed, c in drawn["fill"]:
        col = im.mcols(c)[0]
        for method in ("Previous", "Next", "Mean"):
            P.fill(col, method)
        r = P.fill_linear(im.ref_mcol(c), col)
        tags["FillLinear unchanged"] += len(r) == 2 and r[1]
        tags["FillLinear descending ref"] += bool(c["n"] > 1 and (np.diff(im.ref_mcol(c).values.astype(np.float64)) < 0).any())
        tags["fill builds the neighbour index"] += im.fill_needs_the_index(col.valid)
        tags["fill: null run across a 4096-bit edge of the bitmap"] += im.run_crosses_a_block_edge(col.valid, c["pad"])
        tags["fill unchanged"] += bool(col.valid.all())
        tags["fill %s" % ("Int64" if col.typ == INT64 else "Float64")] += 1
    want = ["%s %s %s" % (k, t, i) for k in KINDS for t in ("Int64", "Float64") for i in ("inclusive", "exclusive")]
    want += ["previous point beyond 2048 rows", "next point beyond 2048 rows", "null run across a 4096-bit edge of the bitmap",
             "trip with more than 768 outputs", "more than 4096 empty windows in a row", "rows below s0 ride in window 0", "rows below s0 are dropped",
             "the -1 sentinel", "PrevRow used", "Linear division by zero", "Int64 Linear result not an integer",
             "FillMean tie, away from zero differs from to even", "FillLinear row skipped for a null ref", "FillLinear division by zero",
             "FillLinear unchanged", "FillLinear descending ref", "fill builds the neighbour index", "fill: null run across a 4096-bit edge of the bitmap",
             "fill unchanged", "fill Int64", "fill Float64", "duplicates on a window start", "nanosecond scale", "a trip spans 2^31", "device-resident",
             "null_count stated", "arrow offset", "column without a bitmap", "1 columns", "2 columns", "3 columns", "rows <= 512", "rows <= 4097", "rows > 4097"]
    want += ["validity " + m for m in im.VALIDITY if m != "own"]
    for t in want:
        assert tags[t] >= 3, (t, tags[t], sorted(tags.items()))


def test_at_most_a_tenth_of_a_seed_lies_outside_the_domain(drawn):
    """... so the GPU test cannot pass by declining; and the chain's share inside the fused kernel's documented shape, from which
    test_fuzz_interpolate_then_aggregate takes its floor"""
    fused = []
    for kind in ("interp", "chain"):
        per_seed = Counter(seed for seed, c in drawn[kind] if im.outside(c))
        assert max(per_seed.values()) <= 0.1 * im.CASES[kind], (kind, per_seed)
        assert sum(per_seed.values()) >= 3, (kind, per_seed)       # (and the declines are exercised at all)
    for seed in DEFAULT_SEEDS:
        fused.append(sum(im.in_the_fused_shape(c) for s, c in drawn["chain"] if s == seed))
    assert min(fused) >= im.FUSED_SHAPED_MIN, fused


# ------------------------------------------------------------------ (e) a model that is wrong in one way is seen
class PreviousFromFirstIndex(im.Model):
    def prev_from(self, first_index):
        return first_index


class NextFromBehindFirstIndex(im.Model):
    def next_from(self, first_index):
        return first_index + 1


class SentinelIgnored(im.Model):
    def empty_gets_a_row(self, start):
        return np.ones(len(start), bool)


class WindowZeroAtLowerBound(im.Model):
    def window0_first(self, lb0):
        return lb0


class HalfToEven(im.Model):
    def round_half(self, x):
        return np.round(x)


class StepPreviousThroughFloat64(im.Model):
    def step_int(self, v):
        return im.go_f64_to_i64(v.astype(np.float64))


class InclusiveRowNotDuplicated(im.Model):
    def inclusive_extra(self, on_end):
        return np.zeros(len(on_end), bool)


class PrevRowAlthoughARowExists(im.Model):
    def prev_row_first(self):
        return True


MUTANTS = [PreviousFromFirstIndex, NextFromBehindFirstIndex, SentinelIgnored, WindowZeroAtLowerBound, HalfToEven, StepPreviousThroughFloat64,
           InclusiveRowNotDuplicated, PrevRowAlthoughARowExists]


def signature(cols):
    return [(len(c.values), c.valid.tobytes(), c.values[c.valid].tobytes()) for c in cols]


def run_case(model, c):
    if c["kind"] == "fill":
        col = im.mcols(c)[0]
        r = model.fill_linear(im.ref_mcol(c), col)
        return signature([model.fill(col, m)[0] for m in ("Previous", "Next", "Mean")] + ([r[0]] if len(r) == 2 else []))
    return signature(model.interpolate(c["ts"], im.mcols(c), c["interval"], c["interps"], offset=c["offset"], inclusive=c["inclusive"]))


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_a_wrong_model_is_seen_in_the_first_eight_seeds(drawn, mutant):
    wrong = mutant()
    kinds = ("fill",) if mutant is HalfToEven else ("interp", "chain")
    seen = None
    for kind in kinds:
        for seed, c in drawn[kind]:
            if seed < 8 and seen is None and not im.outside(c) and run_case(wrong, c) != run_case(M, c):
                seen = c["label"]
    assert seen is not None, "seeds 0..7 would not notice %s" % mutant.__name__
