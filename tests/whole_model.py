"""A numpy MODEL of aggregation.Aggregate over the whole frame (reference rolling/aggregation/whole.go and the reducers it calls), in
O(n log n) - what tests/test_gpu_whole_fuzz.py compares bowgpu_aggregate_whole with.  The oracle (oracle/bow_oracle.c) walks to the next
valid point from every row and counts Mode's occurrences again for every row, so it cannot afford the frames in which a whole-frame
kernel goes wrong: valid points a workgroup or several apart.  tests/test_whole_model_cpu.py proves the model against the oracle and the
reference's vectors and asserts what cases() covers.

Domain: the device path's - an Int64 interval column without nulls, Int64 / Float64 value columns with or without nulls, every reducer
kind, transformation.Factor chains.  outside() names the error code of everything else from the inputs alone.

Row for row as the reference:
  * a POINT is a row whose value is valid: t = float64(ts), v = float64(value) (bowgetters.go:224-229; the interval column has no nulls)
  * the return type of InputDependent AND IteratorDependent kinds is the INPUT column's type (whole.go:44-46); SetOrDropStrict drops a
    result whose Go type is not the buffer's (whole.go:86): WindowStart - an int64 - over a Float64 column comes back nil
  * FirstValue / LastValue = int64(float64(ts[0])), int64(float64(ts[n - 1])) (whole.go:54-71); IsInclusive is true: every row counts
  * Min / Max (minmax.go): the first valid value seeds - a NaN seed sticks -, then strict comparisons: the earliest of equal extremes
  * Mode (mode.go): the value whose count reaches the maximum FIRST; -0 == +0 as keys, every NaN a key of its own, the row's own bits
  * Factor (factor.go): float64 x * f; int64 int64(float64(x) * f), truncated, INT64_MIN out of range

An ORDER-SENSITIVE result (Sum, ArithmeticMean, IntegralStep / Trapezoid, WeightedAverageStep / Linear) carries three things:
  bits       the reference's own result: the left-to-right loop from 0.0, np.add.accumulate - not np.sum, which adds pairwise
  exact      the exact sum of the same float64 terms (math.fsum), then the one division of Mean / WeightedAverage in float64
  mag, rows  sum |T_i| and the frame's rows: tests/tolerance.py's bound for ONE window of `rows` rows
and `int_exact`: every term is an integer (a multiple of one half for the trapezoid terms, (v0 + v1) / 2 * dt) and sum |T_i| < 2^53
(2^52) - then every partial sum in every order is exact, and an order-free sum must return the reference's bits."""
import math

import numpy as np

import tolerance as tol
from bow_amd import capi
from interp_model import go_f64_to_i64
from oracle import pyoracle as orc

FLOAT64, INT64, BOOLEAN, STRING = capi.FLOAT64, capi.INT64, capi.BOOLEAN, capi.STRING
KINDS = tuple(sorted(orc.AGG, key=orc.AGG.get))
ORDER_SENSITIVE = tol.ORDER_SENSITIVE
_TYPE = {"Count": INT64, "WindowStart": None, "First": None, "Last": None, "Mode": None}     # None: the input column's; else Float64
SNAN = np.array([0x7FF0000000000001], np.uint64).view(np.float64)[0]


def f2b(x):
    return np.array([x], np.float64).view(np.uint64)[0]


def wrap64(x):
    """a Python integer as Go's int64 arithmetic leaves it"""
    return (int(x) + 2 ** 63) % 2 ** 64 - 2 ** 63


class MCol:
    """one column: its n values (no Arrow offset), bool validity, type"""

    def __init__(self, values, valid, typ):
        self.values, self.valid, self.typ = values, valid, typ


class Res:
    """one reducer's output column: type, length (0 for an empty frame, else 1), validity and the 8 bytes of the slot; for an
    order-sensitive kind also exact / mag / rows / count / width / int_exact (see the module's text)"""

    def __init__(self, typ, length=1, valid=False, bits=0):
        self.typ, self.length, self.valid, self.bits = typ, length, bool(valid), np.uint64(int(bits) % 2 ** 64)
        self.exact = None

    def as_float(self):
        return np.array([self.bits], np.uint64).view(np.float64)[0]

    def as_int(self):
        return int(np.array([self.bits], np.uint64).view(np.int64)[0])


def seq_sum(terms):
    """the reference's loop: sum := 0.0; sum += term, left to right"""
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate(([0.0], terms)))[-1]


def exact_sum(terms):
    """the exactly rounded sum of the float64 terms; where a term is not finite, what any order gives: NaN or an infinity"""
    if not np.isfinite(terms).all():
        return float(seq_sum(terms))
    return math.fsum(terms.tolist())


class Model:
    # ---- the rules a kernel can get wrong, one method each (tests/test_whole_model_cpu.py overrides them one at a time)
    def pairs(self, rows):
        """(a, b): point a pairs with point b - every point with the NEXT POINT, wherever its row lies"""
        a = np.arange(max(len(rows) - 1, 0))
        return a, a + 1

    def step_tail(self, v_last, dt_last):
        """the last IntegralStep term: v_last * (float64(LastValue) - t_last) (integral.go:49-52)"""
        with np.errstate(all="ignore"):
            return np.float64(v_last) * np.float64(dt_last)

    def last_value_row(self, n, valid):
        return n - 1

    def seed_sticks(self, seed):
        return np.isnan(seed)

    def extreme_of_equals(self, hits):
        return hits[0]

    def first_row(self, valid):
        hits = np.flatnonzero(valid)
        return int(hits[0]) if hits.size else -1

    def mean_divisor(self, count, n):
        return count

    def own_bits(self, col, row):
        return col.values[row:row + 1].view(np.uint64)[0]

    def strict(self, typ, is_int):
        return (typ == INT64) == is_int

    def mode_row(self, at_max):
        return at_max[0]

    def factor_int(self, x, f):
        with np.errstate(all="ignore"):
            return int(go_f64_to_i64(np.float64(x) * np.float64(f)))

    # ---- whole.go
    def aggregate(self, cols, ts_col, aggs):
        """cols: the frame as MCols (cols[ts_col]: Int64, all valid); aggs: (kind, col[, factors]) -> [Res]"""
        ts = cols[ts_col].values
        n = len(ts)
        out, memo = [], {}
        for a in aggs:
            kind, ci = a[0], a[1]
            factors = list(a[2]) if len(a) > 2 and a[2] else []
            col = cols[ci]
            typ = _TYPE.get(kind, FLOAT64) or col.typ
            if n == 0:
                out.append(Res(typ, 0))
                continue
            if ci not in memo:
                memo[ci] = self.points(ts, col)
            out.append(self.reduce(kind, ts, col, memo[ci], typ, factors))
        return out

    def points(self, ts, col):
        rows = np.flatnonzero(col.valid)
        P = {"rows": rows, "t": ts[rows].astype(np.float64), "v": col.values[rows].astype(np.float64)}
        lr = self.last_value_row(len(ts), col.valid)
        P["first_value"] = int(go_f64_to_i64(np.float64(ts[0])))
        P["last_value"] = int(go_f64_to_i64(np.float64(ts[lr])))
        return P

    def ordered(self, kind, P, n):
        """(terms, divisor or None, nil) of an order-sensitive kind"""
        v, t = P["v"], P["t"]
        if kind in ("Sum", "ArithmeticMean"):
            if kind == "Sum":
                return v, None, False
            return v, (float(self.mean_divisor(len(v), n)) if len(v) else None), len(v) == 0
        a, b = self.pairs(P["rows"])
        with np.errstate(all="ignore"):
            dt = t[b] - t[a]
            if kind in ("IntegralStep", "WeightedAverageStep"):
                if len(v) == 0:
                    return v, None, True
                terms = np.concatenate((v[a] * dt, [self.step_tail(v[-1], np.float64(P["last_value"]) - t[-1])]))
            else:
                if len(a) == 0:
                    return v, None, True
                terms = (v[a] + v[b]) / 2 * dt
        wide = float(wrap64(P["last_value"] - P["first_value"])) if kind.startswith("Weighted") else None
        return terms, wide, False

    def reduce(self, kind, ts, col, P, typ, factors):
        n, rows = len(ts), P["rows"]
        is_int_col = col.typ == INT64
        r = Res(typ)
        value, is_int = None, False              # value: float or int (Go's interface{}); None: nil
        if kind in ORDER_SENSITIVE:
            terms, div, nil = self.ordered(kind, P, n)
            if not nil:
                with np.errstate(all="ignore"):
                    ref, exact = np.float64(seq_sum(terms)), np.float64(exact_sum(terms))
                    mag = math.fsum(np.abs(terms[np.isfinite(terms)]).tolist())
                    if div is not None:
                        ref, exact = ref / np.float64(div), exact / np.float64(div)
                    for f in factors:
                        exact = exact * np.float64(f)
                value = ref
                half = kind in ("IntegralTrapezoid", "WeightedAverageLinear")
                with np.errstate(all="ignore"):
                    whole = bool(np.isfinite(terms).all() and (terms * (2 if half else 1) == np.trunc(terms * (2 if half else 1))).all()
                                 and (P["v"] == np.trunc(P["v"])).all())
                r.exact, r.mag, r.rows, r.count, r.width = float(exact), mag, n, max(len(rows), 1), (abs(div) if kind.startswith("Weighted") else 1.0)
                r.int_exact = whole and mag < (2.0 ** 52 if half else 2.0 ** 53) and bool(np.isfinite(exact))
        elif kind == "WindowStart":
            value, is_int = P["first_value"], True
        elif kind == "NumRows":
            value = np.float64(n)
        elif kind == "Count":
            value, is_int = len(rows), True
        elif kind in ("Min", "Max"):
            if len(rows):
                v = P["v"]
                if self.seed_sticks(v[0]):
                    at = 0
                else:
                    nn = np.flatnonzero(~np.isnan(v))
                    if nn.size == 0:
                        at = 0
                    else:
                        best = v[nn].min() if kind == "Min" else v[nn].max()
                        at = int(self.extreme_of_equals(nn[v[nn] == best]))
                # (float64(v) of the row: for a Float64 column the row's own bits, a signalling NaN seed included)
                value = "bits", (col.values[rows[at]:rows[at] + 1].view(np.uint64)[0] if not is_int_col else f2b(v[at]))
        elif kind in ("First", "Last", "Mode"):
            row = -1
            if kind == "First":
                row = self.first_row(col.valid)
                row = row if row >= 0 and col.valid[row] else -1
            elif kind == "Last":
                row = int(rows[-1]) if len(rows) else -1
            elif len(rows):
                row = int(rows[self.mode_point(col, rows)])
            if row >= 0:
                value, is_int = ("bits", self.own_bits(col, row)), is_int_col
        # transformation.Factor, SetOrDropStrict
        if value is None:
            return r
        if isinstance(value, tuple):
            bits = value[1]
            if not factors:                   # the row's own 8 bytes, untouched (a signalling NaN stays one)
                if self.strict(typ, is_int):
                    r.valid, r.bits = True, np.uint64(bits)
                return r
            value = int(np.array([bits], np.uint64).view(np.int64)[0]) if is_int else np.array([bits], np.uint64).view(np.float64)[0]
        for f in factors:
            if is_int:
                value = self.factor_int(value, f)
            else:
                with np.errstate(all="ignore"):
                    value = np.float64(value) * np.float64(f)
        if not self.strict(typ, is_int):
            return r
        r.valid = True
        r.bits = np.uint64(int(value) % 2 ** 64) if is_int else f2b(value)
        return r

    def mode_point(self, col, rows):
        """which point Mode returns: occurrences per key in row order; the first point whose count equals the largest count"""
        if col.typ == INT64:
            keys, lone = col.values[rows].view(np.uint64), np.zeros(len(rows), bool)
        else:
            v = col.values[rows]
            lone = np.isnan(v)                                     # NaN != NaN: a key of its own each time
            keys = np.where(v == 0, 0.0, v).view(np.uint64)        # -0 == +0
        order = np.argsort(keys, kind="stable")
        ks = keys[order]
        start = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
        occ_sorted = np.arange(len(ks)) - np.repeat(start, np.diff(np.concatenate((start, [len(ks)])))) + 1
        occ = np.empty(len(ks), np.int64)
        occ[order] = occ_sorted
        occ[lone] = 1              # (NaNs of one payload sorted into one run: no other key's count saw them)
        return int(self.mode_row(np.flatnonzero(occ == occ.max())))


M = Model()


def bound(res, kind, factors):
    """tests/tolerance.py's bound on |got - res.exact| for one window of res.rows rows"""
    r = abs(res.exact) if np.isfinite(res.exact) else 0.0
    with np.errstate(all="ignore"):
        return float(tol.window_bound(kind, float(res.rows), res.mag, float(res.count), res.width, list(factors), r))


# ------------------------------------------------------------------ the cases
CASES = 16                       # per seed
SEED_BASE = 31_000
SMALL = (1, 2, 7, 8, 9, 511, 512, 513, 4095, 4096, 4097)
MULTI = (65_535, 65_536, 65_537, 70_001, 131_072, 131_073, 200_000)       # 1 .. 4 workgroups; 65 537: 2 of 33 280 rows, quarters of 8 320
LARGE = 1_000_003                                                        # 16 workgroups
ANY_SIZE = ("no-bitmap", "iid5", "iid30", "iid90", "all-null", "one-point")
# layouts that need two workgroups or more (FOUR: "gap-blocks"), planted from capi.whole_layout
PLANTED = ("two-ends", "one-workgroup", "edge-block", "edge-quarter", "edge-step", "gap-blocks", "tail-nulls", "head-nulls")
LAYOUTS = ANY_SIZE + PLANTED
TS_KINDS = ("dup", "irregular", "negative", "ns")
F_KINDS = ("normal", "mixed", "special", "zeros", "few", "int-exact")
I_KINDS = ("full", "few", "int-exact")
FACTORS = (0.1, -2.5, 1e3, 0.5, 3.0, -1.0, 1e-3)
DECLINES = ("ts-nulls", "ts-float64", "col-boolean", "col-string", "65-reducers", "bad-col", "bad-ts-col")


def edges(n):
    """row indices at which a (workgroup, wavefront quarter, 512-row step) of the device path begins, 0 and n excluded"""
    nblocks, chunk = capi.whole_layout(n)
    blocks, quarters, steps = [], [], []
    for b in range(nblocks):
        lo, hi = b * chunk, min((b + 1) * chunk, n)
        if lo >= n:
            break
        if lo:
            blocks.append(lo)
        s_per = ((hi - lo + 511) // 512 + 3) // 4
        for q in range(1, 4):
            if lo + q * s_per * 512 < hi:
                quarters.append(lo + q * s_per * 512)
        steps += [r for r in range(lo + 512, hi, 512) if (r - lo) % (s_per * 512)]
    return blocks, quarters, steps


def draw_valid(rng, n, layout):
    """bool validity of n rows, or None (no bitmap)"""
    valid = np.zeros(n, bool)
    nblocks, chunk = capi.whole_layout(n)
    if layout == "no-bitmap":
        return None
    if layout.startswith("iid"):
        return rng.random(n) >= int(layout[3:]) / 100.0
    if layout == "all-null":
        return valid
    if layout == "one-point":
        valid[int(rng.integers(0, n))] = True
        return valid
    last = (n - 1) // chunk                           # the last workgroup that has rows
    blocks, quarters, steps = edges(n)
    if layout == "two-ends":
        valid[int(rng.integers(0, chunk))] = True
        valid[int(rng.integers(last * chunk, n))] = True
    elif layout == "one-workgroup":
        b = int(rng.integers(0, last + 1))
        lo, hi = b * chunk, min((b + 1) * chunk, n)
        valid[rng.integers(lo, hi, int(rng.integers(2, 40)))] = True
    elif layout in ("edge-block", "edge-quarter", "edge-step"):
        at = {"edge-block": blocks, "edge-quarter": quarters, "edge-step": steps}[layout]
        r = int(at[int(rng.integers(0, len(at)))])
        valid[[r - 1, r]] = True
        if rng.random() < 0.3:                        # ... and a few points elsewhere
            valid[rng.integers(0, n, 5)] = True
    elif layout == "gap-blocks":
        gap = int(rng.integers(2, last))              # workgroups without a point: 2 .. last - 1
        b0 = int(rng.integers(0, last - gap))
        valid[int(rng.integers(b0 * chunk, (b0 + 1) * chunk))] = True
        b1 = b0 + gap + 1
        valid[int(rng.integers(b1 * chunk, min((b1 + 1) * chunk, n)))] = True
        if rng.random() < 0.5:                        # dense outside the gap
            dense = rng.random(n) >= 0.3
            dense[(b0 + 1) * chunk:b1 * chunk] = False
            valid |= dense
    elif layout in ("tail-nulls", "head-nulls"):
        run = int(rng.integers(chunk + 1, n - 1))
        valid = rng.random(n) >= 0.3
        if layout == "tail-nulls":
            valid[n - run:] = False
            valid[n - run - 1] = True
        else:
            valid[:run] = False
            valid[run] = True
    return valid


def draw_ts(rng, n, kind):
    if kind == "dup":
        return (np.cumsum(rng.integers(0, 3, n)) - int(rng.integers(0, 50))).astype(np.int64)
    if kind == "irregular":
        return (np.cumsum(rng.integers(1, 1000, n)) + int(rng.integers(0, 10 ** 6))).astype(np.int64)
    if kind == "negative":
        t = np.cumsum(rng.integers(0, 40, n)).astype(np.int64)
        return t - int(t[-1]) - int(rng.integers(1, 10 ** 9))
    base = int(rng.choice([1_600_000_000_000_000_000, -3_000_000_000_000_000_000]))          # "ns": |ts| > 2^53, float64(ts) rounds
    return (base + np.cumsum(rng.integers(0, 2_000_000_000, n))).astype(np.int64)


def draw_values(rng, tot, typ, kind, first_valid_at):
    if typ == FLOAT64:
        if kind == "normal":
            return np.round(rng.standard_normal(tot) * 100, 2)
        if kind == "mixed":
            return rng.standard_normal(tot) * 10.0 ** rng.integers(-8, 9, tot)
        if kind == "zeros":
            v = np.abs(np.round(rng.standard_normal(tot) * 3, 0)) * float(rng.choice([1.0, -1.0]))     # zeros of both signs are the minimum (maximum)
            v[rng.random(tot) < 0.5] = 0.0
            v[rng.random(tot) < 0.3] = -0.0
            return v
        if kind == "few":
            v = rng.choice(np.array([1.5, 2.25, 0.0, -0.0, 7.0, np.nan]), tot) * float(rng.choice([1.0, -1.0]))       # Mode ties; zeros the extreme
            if first_valid_at is not None and rng.random() < 0.5:
                v[first_valid_at] = np.nan
            return v
        if kind == "int-exact":
            return rng.integers(-1000, 1000, tot).astype(np.float64)
        v = np.round(rng.standard_normal(tot) * 100, 2)                                        # "special"
        for x, share in ((np.nan, 0.02), (SNAN, 0.01), (0.0, 0.05), (-0.0, 0.05)):
            v[rng.random(tot) < share] = x
        which = int(rng.integers(0, 6))
        if which in (0, 4, 5) and first_valid_at is not None:
            v[first_valid_at] = [np.nan, SNAN][int(rng.integers(0, 2))]                        # a NaN seeds Min / Max
        elif which == 1:
            v[rng.random(tot) < 0.02] = np.inf
        elif which == 2:
            v[rng.random(tot) < 0.02] = np.inf
            v[rng.random(tot) < 0.02] = -np.inf
        return v
    if kind == "full":
        return rng.integers(-2 ** 63, 2 ** 63 - 1, tot, dtype=np.int64, endpoint=True)
    if kind == "few":
        return rng.choice(np.array([2 ** 53 + 1, 2 ** 53, -(2 ** 62) - 3, 5, -5, 2 ** 63 - 1], np.int64), tot)
    return rng.integers(-1000, 1000, tot).astype(np.int64)


def draw_aggs(rng, ncols, count=None):
    if count is None:
        u = rng.random()
        count = 64 if u < 0.04 else int(rng.integers(17, 41)) if u < 0.14 else int(rng.integers(1, 13))
    one_col = count > 16 and rng.random() < 0.7        # more than kMaxAggs reducers of ONE column: the finish launch loops
    col1 = int(rng.integers(0, ncols))
    aggs = []
    for _ in range(count):
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        col = col1 if one_col else int(rng.integers(0, ncols)) if rng.random() < 0.8 else 0
        fac = [float(FACTORS[int(rng.integers(0, len(FACTORS)))]) for _ in range(int(rng.integers(1, capi.MAX_FACTORS + 1)))] if rng.random() < 0.25 else []
        aggs.append((kind, col, fac) if fac else (kind, col))
    if count + 5 <= capi.WHOLE_MAX_AGGS and ncols > 1 and rng.random() < 0.5:
        # the positional reducers of one value column together, unscaled: what a NaN seed, zeros of both signs or a tie does to each
        col = int(rng.integers(1, ncols))
        for kind in ("Min", "Max", "First", "Last", "Mode"):
            aggs.insert(int(rng.integers(0, len(aggs) + 1)), (kind, col))
    return aggs


def cases(seed):
    """the CASES cases of a seed (a function of the seed alone).  A case: label, n, layout per value column, tags; "cols": per column
    of the frame (column 0 the interval column) (buffer, bitmap or None, type, Arrow offset, bool validity of the n rows); aggs;
    stated (null_count given, per column); residency of the inputs ("host" / "pinned" / "device") and of the outputs (out_device);
    ts_col.  Case 0 of a seed may lie outside the domain ("decline") or be the empty frame."""
    rng = np.random.default_rng(SEED_BASE + seed)
    out = []
    for i in range(CASES):
        decline = None
        turn = seed * CASES + i                           # (the listed sizes in turn: every one of them comes up, whatever the draws)
        layouts = [ANY_SIZE[int(rng.integers(0, len(ANY_SIZE)))] for _ in range(int(rng.integers(1, 4)))]
        planted = []
        if rng.random() < 0.4:                            # one column (now and then each) with a layout planted on the kernel's edges
            for k in range(len(layouts)):
                if k == 0 or rng.random() < 0.3:
                    layouts[k] = PLANTED[int(rng.integers(0, len(PLANTED)))]
            planted = [l for l in layouts if l in PLANTED]
            layouts = [layouts[j] for j in rng.permutation(len(layouts))]
        if "gap-blocks" in planted:
            n = LARGE if rng.random() < 0.3 else 200_000
        elif planted:
            n = LARGE if rng.random() < 0.1 else int(MULTI[2 + turn % (len(MULTI) - 2)])                # 65 537 rows and more
        else:
            u = rng.random()
            n = int(rng.integers(1, 3000)) if u < 0.2 else int(SMALL[turn % len(SMALL)]) if u < 0.6 else \
                LARGE if u < 0.63 else int(MULTI[turn % len(MULTI)])
        if i == 0:
            k = seed % (len(DECLINES) + 2)                # each decline in turn, the empty frame, an ordinary case
            if k < len(DECLINES):
                decline = DECLINES[k]
            elif k == len(DECLINES):
                n = 0
            if k <= len(DECLINES):
                layouts = [l if l in ANY_SIZE else "iid30" for l in layouts]
                n = min(n, 4097)
        ts_kind = TS_KINDS[int(rng.integers(0, len(TS_KINDS)))]
        tags = {ts_kind}
        pad = int(rng.integers(0, 71)) if rng.random() < 0.6 else 0
        ts_buf = np.concatenate((rng.integers(-9, 9, pad), draw_ts(rng, n, ts_kind) if n else np.zeros(0, np.int64), rng.integers(-9, 9, 5))).astype(np.int64)
        cols = [(ts_buf, None, INT64, pad, np.ones(n, bool))]
        for layout in layouts:
            typ = INT64 if rng.random() < 0.45 else FLOAT64
            kinds = F_KINDS if typ == FLOAT64 else I_KINDS
            vk = "int-exact" if rng.random() < 0.2 else kinds[int(rng.integers(0, len(kinds)))]
            valid = draw_valid(rng, n, layout) if n else (None if layout == "no-bitmap" else np.zeros(0, bool))
            off = int(rng.integers(0, 71)) if rng.random() < 0.6 else 0
            tot = off + n + 9
            hits = np.flatnonzero(valid) if valid is not None else np.arange(min(n, 1))
            buf = draw_values(rng, tot, typ, vk, off + int(hits[0]) if hits.size else None)
            bm = None
            if valid is not None:
                bits = np.ones((tot + 7) // 8 * 8, bool)         # the bits around the column are SET: a row read outside it would count
                bits[off:off + n] = valid
                bm = np.packbits(bits, bitorder="little")
            cols.append((buf, bm, typ, off, np.ones(n, bool) if valid is None else valid))
            tags |= {layout, ("f64 " if typ == FLOAT64 else "i64 ") + vk}
        aggs = draw_aggs(rng, len(cols))
        ts_col = 0
        if decline == "ts-nulls":
            tv = rng.random(n) >= 0.2
            tv[int(rng.integers(0, n))] = False
            bits = np.ones((pad + n + 7) // 8 * 8 + 8, bool)
            bits[pad:pad + n] = tv
            cols[0] = (ts_buf, np.packbits(bits, bitorder="little"), INT64, pad, tv)
        elif decline == "ts-float64":
            cols[0] = (ts_buf.astype(np.float64), None, FLOAT64, pad, np.ones(n, bool))
        elif decline in ("col-boolean", "col-string"):
            cols.append((rng.integers(0, 255, (n + 7) // 8 + 16).astype(np.uint8), None, BOOLEAN if decline == "col-boolean" else STRING, 0, np.ones(n, bool)))
            aggs.insert(int(rng.integers(0, len(aggs) + 1)), ("Count", len(cols) - 1))
        elif decline == "65-reducers":
            aggs = draw_aggs(rng, len(cols), capi.WHOLE_MAX_AGGS + 1)
        elif decline == "bad-col":
            aggs.insert(int(rng.integers(0, len(aggs) + 1)), ("Sum", [len(cols), -1][int(rng.integers(0, 2))]))
        elif decline == "bad-ts-col":
            ts_col = [len(cols), -1][int(rng.integers(0, 2))]
        stated = [bool(rng.random() < 0.5) for _ in cols]
        u = rng.random()
        case = {"label": "seed %d case %d n=%d %s ts=%s" % (seed, i, n, "+".join(layouts), ts_kind) + (" decline=%s" % decline if decline else ""),
                "seed": seed, "n": n, "layouts": layouts, "tags": tags, "cols": cols, "aggs": aggs, "ts_col": ts_col, "stated": stated,
                "residency": "device" if u < 0.3 else "pinned" if u < 0.45 else "host", "out_device": bool(rng.random() < 0.3), "decline": decline}
        out.append(case)
    return out


def outside(case):
    """None inside the device path's domain, else the error code bowgpu_aggregate_whole declines with - from the inputs alone, in the
    order the call checks them: indices (-6), value column types (-9), [an empty frame is served], the interval column's type (-9),
    its nulls (-13), Float64 (-9), more than 64 reducers (-9)"""
    cols, aggs, ts_col = case["cols"], case["aggs"], case["ts_col"]
    if not 0 <= ts_col < len(cols):
        return -6
    for a in aggs:
        if not 0 <= a[1] < len(cols):
            return -6
        if cols[a[1]][2] not in (INT64, FLOAT64):
            return -9
    if case["n"] == 0:
        return None
    _buf, bm, typ, _off, valid = cols[ts_col]
    if typ not in (INT64, FLOAT64):
        return -9
    if bm is not None and not valid.all():
        return -13
    if typ != INT64 or len(aggs) > capi.WHOLE_MAX_AGGS:
        return -9
    return None


def cut(case, rows):
    """the case's first `rows` rows (what the oracle can afford): same buffers and offsets, shorter columns"""
    n = min(case["n"], rows)
    return dict(case, n=n, cols=[(buf, bm, typ, off, valid[:n]) for buf, bm, typ, off, valid in case["cols"]])


def mcols(case):
    n = case["n"]
    return [MCol(buf[off:off + n], valid, typ) for buf, bm, typ, off, valid in case["cols"]]


def ocols(case):
    n = case["n"]
    return [orc.Column(buf, bm, typ, offset=off, length=n) for buf, bm, typ, off, _valid in case["cols"]]


def ccols(case):
    """the case for the C ABI, host-resident; null_count stated or -1"""
    n = case["n"]
    return [capi.Column(buf, bm, typ, off, n, (int((~valid).sum()) if stated else -1) if bm is not None else 0)
            for (buf, bm, typ, off, valid), stated in zip(case["cols"], case["stated"])]
