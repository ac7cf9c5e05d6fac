"""A vectorised MODEL of Rolling.Interpolate, Bow.FillPrevious / FillNext / FillMean / FillLinear and Interpolate -> Aggregate, and the
seeded cases tests/test_gpu_interp_fuzz.py pushes through the device.

Why a model: the oracle (oracle/bow_oracle.c) restates the reference literally, and the reference's GetPrevFloat64s / GetNextFloat64s
walks start again from every null row and every window - quadratic to cubic in the length of a null run - so a comparison with the
oracle stops at a few hundred rows.  The kernels' machinery (512-row trips and the carry between them, the count scan over super-tiles,
the near walk of 64 validity words and the repeat behind it, the neighbour index and its 4096-bit blocks, the unstaged trips, the
queue of empty-window runs) starts where the oracle stops.  The model costs O(n log n): np.searchsorted for the windows,
np.maximum.accumulate / np.minimum.accumulate for the previous / next valid row.  tests/test_interp_model_cpu.py proves it against the
oracle bit for bit wherever the oracle is affordable and against the reference's own vectors (tests/golden); the GPU tests then let it
stand in for the oracle at the sizes that matter.

What it states, each point from oracle/bow_oracle.c (which cites the reference line by line), for an ASCENDING INT64 INTERVAL COLUMN
WITHOUT NULLS:
  windows      orc_plan_windows / iter_next: s0 from Go's truncating division (above ts[0] when ts[0] is negative), W = (last - s0) /
               interval + 1, FirstIndex of window k = lower_bound(ts, s_k) except window 0 whose slice begins at row 0; rows below s0
               ride in window 0 when it takes a row of its own and are dropped otherwise; an inclusive window also takes the first
               row that sits on its end, and that row opens the next window (`rowIndex - 1`)
  Interpolate  orc_interpolate / apply_interp: a synthetic row in front of a window unless go_f64_to_i64(float64(first timestamp of
               its slice)) equals its start, "first value" -1 for an empty window; Linear in linear.go:34-35's association on the
               nearest valid row before FirstIndex (else the PrevRow point) and the nearest from it on; StepPrevious keeps the integer
  fills        orc_fill / orc_fill_linear, with the `unchanged` flag; C's round (half away from zero) for Int64
  chain        Model.interpolate, then oracle.aggregate on its output (the interpolated frame has no long-null-run problem once the
               oracle only aggregates it)

Out of scope: an interval column with nulls (tests/null_ts_cases.py and test_gpu_null_ts_fuzz.py own it), the sharded forms, Boolean
columns, whole-frame Aggregate."""
import numpy as np

from oracle import pyoracle as orc

FLOAT64, INT64 = orc.FLOAT64, orc.INT64
INT64_MIN = -2 ** 63
TRIP = 512                       # bow_amd/csrc/interpolate.hip kT3Rows, interp_fill.hip kTrip
NEAR_BITS = 2048                 # bitmap_device.h kNbrNearWords * 32: what prev_valid_near / next_valid_near look at
BLOCK_BITS = 4096                # common.h kNbrBlockBits
STAGE_OUTPUTS = 768              # interpolate.hip kT3Stage: a trip with more outputs writes directly
GAP_LIST = 4096                  # interp_fill.hip kGapListCap


# ------------------------------------------------------------------ Go / C numeric semantics
def go_f64_to_i64(x):
    """CVTTSD2SI: truncation, NaN / out of range -> INT64_MIN (bow_oracle.c:20-23)"""
    x = np.asarray(x, np.float64)
    ok = (x >= -9223372036854775808.0) & (x < 9223372036854775808.0)
    out = np.full(x.shape, INT64_MIN, np.int64)
    out[ok] = x[ok].astype(np.int64)
    return out


def c_round(x):
    """C's round(): half away from zero (math.Round).  Not np.round, which goes to even."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(x)
        return np.where(np.abs(x - t) >= 0.5, t + np.copysign(1.0, x), t)


def prev_valid(valid):
    """index of the nearest valid row at or before i, -1 if none"""
    return np.maximum.accumulate(np.where(valid, np.arange(len(valid)), -1))


def next_valid(valid):
    """index of the nearest valid row at or behind i, n if none"""
    n = len(valid)
    return np.minimum.accumulate(np.where(valid, np.arange(n), n)[::-1])[::-1]


def first_window_start(ts0, interval, offset):
    """(s0, normalised offset): rolling.go:114-128 and :87-100 - Go's division truncates"""
    if offset >= interval or offset <= -interval:
        offset = abs(offset) % interval * (1 if offset >= 0 else -1)       # Go's % takes the sign of the dividend
    if offset < 0:
        offset += interval
    q = abs(ts0) // interval * (1 if ts0 >= 0 else -1)
    first = q * interval + offset
    if first > ts0:
        first -= interval
    return first, offset


def plan(ts, interval, offset):
    """(s0, W) of orc_plan_windows"""
    if len(ts) == 0:
        return 0, 0
    s0, _ = first_window_start(int(ts[0]), interval, offset)
    last = int(ts[-1])
    return s0, (0 if s0 > last else (last - s0) // interval + 1)


class MCol:
    """one column of the model: the n values of the column itself (no Arrow offset), bool validity, type"""

    def __init__(self, values, valid, typ):
        self.values, self.valid, self.typ = values, valid, typ

    def column(self):
        """as an oracle Column (what tests/test_gpu_callers.cmp_out and orc.aggregate take)"""
        return orc.Column(self.values, np.packbits(self.valid, bitorder="little"), self.typ, 0, len(self.values))


class Windows:
    """the iteration of one frame: per window its start, FirstIndex, slice [begin, end) and whether a synthetic row precedes it"""
    pass


class Model:
    """The hooks below are what tests/test_interp_model_cpu.py overrides to make deliberately wrong models."""

    # ---- hooks
    def prev_from(self, first_index):              # linear.go:20 / stepprevious.go:17: the search starts at FirstIndex - 1
        return first_index - 1

    def next_from(self, first_index):              # linear.go:28: ... and at FirstIndex
        return first_index

    def window0_first(self, lb0):                  # rolling.go:188: window 0 begins at row 0 whatever lies below s0
        return 0

    def empty_gets_a_row(self, start):             # interpolation.go:119-127: an empty window's "first value" is -1 - its start, once
        return start != -1

    def inclusive_extra(self, on_end):             # rolling.go:201-209: the row on the window's end belongs to it too
        return on_end

    def round_half(self, x):                       # bowfill.go:93, :150: math.Round
        return c_round(x)

    def step_int(self, v):                         # stepprevious.go:22: GetValue keeps the int64
        return v

    def prev_row_first(self):                      # linear.go:21-26: PrevRow only when the frame has no previous row
        return False

    def note(self, **figures):                     # what a step was made of, for whoever wants to count it (the coverage conditions)
        pass

    # ---- windows
    def windows(self, ts, interval, offset, inclusive):
        n = len(ts)
        w = Windows()
        w.s0, w.W = plan(ts, interval, offset)
        k = np.arange(w.W, dtype=np.int64)
        w.start = w.s0 + k * interval
        lb = np.searchsorted(ts, w.start, side="left")
        end = np.searchsorted(ts, w.start + interval, side="left")
        if inclusive and w.W:
            on_end = (end < n) & (ts[np.minimum(end, n - 1)] == w.start + interval)
            end = end + self.inclusive_extra(on_end).astype(np.int64)
        w.first_index = lb.copy()
        if w.W:
            w.first_index[0] = self.window0_first(int(lb[0]))
        # a slice holds a row of the window's own (window 0: one at or above s0) or nothing at all
        w.begin = w.first_index
        w.end = np.where(end > lb, end, w.begin)
        w.length = w.end - w.begin
        has = w.length > 0
        fv = np.zeros(w.W, np.int64)
        fv[has] = go_f64_to_i64(ts[w.begin[has]].astype(np.float64))          # interpolation.go:121 reads the timestamp as float64
        w.synthetic = np.where(has, fv != w.start, self.empty_gets_a_row(w.start))
        return w

    # ---- synthetic values of one column, for the windows `sel` (indices)
    def synthetic(self, w, sel, ts, col, ip):
        """(values, valid) of column `col`'s synthetic rows"""
        kind, m = ip["kind"], len(sel)
        is_int = col.typ == INT64
        zero = np.zeros(m, np.int64 if is_int else np.float64)
        nil = np.zeros(m, bool)
        if kind == "WindowStart":
            return w.start[sel].astype(zero.dtype), ~nil
        if kind == "None":
            return zero, nil
        if kind == "Const":
            c = np.full(m, ip.get("const", 0.0), np.float64)
            return (go_f64_to_i64(c) if is_int else c), ~nil
        n = len(ts)
        fi = w.first_index[sel]
        pv = np.concatenate((prev_valid(col.valid), [-1]))          # [-1] -> -1: no row to search from
        pf = self.prev_from(fi)
        p = pv[np.where((pf >= 0) & (pf < n), pf, -1)]
        prev = ip.get("prev")
        if kind == "StepPrevious":
            out, ok = zero.copy(), p >= 0
            out[ok] = self.step_int(col.values[p[ok]]) if is_int else col.values[p[ok]]
            if prev is not None and prev[3]:                         # stepprevious.go:13-15: the PrevRow VALUE (its timestamp is not looked at)
                use = ~ok | self.prev_row_first()
                out[use] = prev[4] if is_int else prev[2]
                ok = ok | use
                self.note(prev_row_used=int((use & (p < 0)).sum()))
            return out, ok
        # Linear
        nv = np.concatenate((next_valid(col.valid), [n]))
        nf = self.next_from(fi)
        q = nv[np.where((nf >= 0) & (nf < n), nf, n)]
        t0 = ts[np.maximum(p, 0)].astype(np.float64)
        v0 = col.values[np.maximum(p, 0)].astype(np.float64)
        have0 = p >= 0
        if prev is not None and prev[1] and prev[3]:                 # linear.go:14-18: both halves of the PrevRow point
            use = ~have0 | self.prev_row_first()
            t0, v0 = np.where(use, np.float64(prev[0]), t0), np.where(use, np.float64(prev[2]), v0)
            have0 = have0 | use
            self.note(prev_row_used=int((use & (p < 0) & (q < n)).sum()))
        ok = have0 & (q < n)
        t2 = ts[np.minimum(q, n - 1)].astype(np.float64)
        v2 = col.values[np.minimum(q, n - 1)].astype(np.float64)
        with np.errstate(all="ignore"):
            coef = (w.start[sel].astype(np.float64) - t0) / (t2 - t0)      # linear.go:34
            r = ((v2 - v0) * coef) + v0                                    # linear.go:35: no fused multiply-add
        out = go_f64_to_i64(r) if is_int else r                            # Buffer.SetOrDrop converts (bowconvert.go:28-29)
        self.note(linear=dict(ok=ok, back=np.where(p >= 0, fi - 1 - p, 0), ahead=np.where(q < n, q - fi, 0), t0=t0, t2=t2, r=r, is_int=is_int))
        return np.where(ok, out, zero), ok

    def interpolate(self, ts, cols, interval, interps, offset=0, inclusive=False):
        """ts: int64[n] ascending; cols: MCol per value column (column 1 .. of the Bow); interps: one per column of the Bow, column 0
        the interval column.  Returns the interpolated Bow as [MCol]."""
        n = len(ts)
        frame = [MCol(ts, np.ones(n, bool), INT64)] + list(cols)
        w = self.windows(ts, interval, offset, inclusive)
        syn = w.synthetic.astype(np.int64)
        per = syn + w.length
        pos = np.cumsum(per) - per                                   # output row of the window's first output
        total = int(per.sum())
        sel = np.flatnonzero(w.synthetic)
        rows = int(w.length.sum())
        wr = np.repeat(np.arange(w.W), w.length)                     # window of each copied row
        j = np.arange(rows) - np.repeat(np.cumsum(w.length) - w.length, w.length)
        src, dst = w.begin[wr] + j, pos[wr] + syn[wr] + j
        out = []
        for c, ip in zip(frame, interps):
            v = np.zeros(total, c.values.dtype)
            ok = np.zeros(total, bool)
            v[dst], ok[dst] = c.values[src], c.valid[src]
            sv, sok = self.synthetic(w, sel, ts, c, ip)
            v[pos[sel]], ok[pos[sel]] = sv, sok
            out.append(MCol(v, ok, c.typ))
        return out

    # ---- fills
    def fill(self, col, method):
        """(MCol, unchanged): bowfill.go:105-253"""
        n = len(col.values)
        v, ok = col.values.copy(), col.valid.copy()
        if ok.all():
            return MCol(v, ok, col.typ), True
        nul = np.flatnonzero(~ok)
        p, q = prev_valid(ok)[nul], next_valid(ok)[nul]
        if method == "Previous":
            hit = p >= 0
            v[nul[hit]] = col.values[p[hit]]
        elif method == "Next":
            hit = q < n
            v[nul[hit]] = col.values[q[hit]]
        else:
            hit = (p >= 0) & (q < n)
            with np.errstate(all="ignore"):
                mean = (col.values[p[hit]].astype(np.float64) + col.values[q[hit]].astype(np.float64)) / 2
            v[nul[hit]] = go_f64_to_i64(self.round_half(mean)) if col.typ == INT64 else mean
            self.note(mean=mean, is_int=col.typ == INT64)
        ok[nul[hit]] = True
        return MCol(v, ok, col.typ), False

    @staticmethod
    def is_sorted(ref):
        """bowassertion.go:15-81: not empty, and ascending or descending (ties allowed) over its valid rows"""
        x = ref.values[ref.valid]
        if len(x) == 0:
            return False
        d = np.diff(x.astype(np.float64)) if ref.typ == FLOAT64 else np.diff(x)
        return bool(not ((d > 0).any() and (d < 0).any()))

    def fill_linear(self, ref, col):
        """(MCol, unchanged) or (-8,): bowfill.go:14-103"""
        n = len(col.values)
        v, ok = col.values.copy(), col.valid.copy()
        if not ref.valid.any():
            return MCol(v, ok, col.typ), True                        # :35-37
        if not self.is_sorted(ref):
            return (-8,)                                             # :39-42
        if ok.all():
            return MCol(v, ok, col.typ), True                        # :53-55
        nul = np.flatnonzero(~ok)
        p, q = prev_valid(ok)[nul], next_valid(ok)[nul]
        pc, qc = np.maximum(p, 0), np.minimum(q, n - 1)
        both = (p >= 0) & (q < n)
        hit = both & ref.valid[nul] & ref.valid[pc] & ref.valid[qc]                     # :74: all three ref values
        self.note(skipped_for_a_null_ref=int((both & ~hit).sum()))
        nul, pc, qc = nul[hit], pc[hit], qc[hit]
        rr, pr, nr = (ref.values[i].astype(np.float64) for i in (nul, pc, qc))
        pf, nf = col.values[pc].astype(np.float64), col.values[qc].astype(np.float64)
        with np.errstate(all="ignore"):
            tmp = rr - pr                                            # :87-90, one operation per statement (next_ref == prev_ref divides by zero)
            tmp = tmp / (nr - pr)
            tmp = tmp * (nf - pf)
            tmp = tmp + pf
        self.note(ref_ties=int((nr == pr).sum()))
        v[nul] = go_f64_to_i64(self.round_half(tmp)) if col.typ == INT64 else tmp
        ok[nul] = True
        return MCol(v, ok, col.typ), False

    # ---- Interpolate -> Aggregate
    def interpolate_aggregate(self, ts, cols, interval, interps, aggs, offset=0, inclusive=False):
        """(list of oracle Columns, new_interval_col): the model's Interpolate, the oracle's Aggregate on it"""
        mid = [c.column() for c in self.interpolate(ts, cols, interval, interps, offset=offset, inclusive=inclusive)]
        return orc.aggregate(mid, 0, interval, aggs, offset=offset, inclusive=inclusive)


M = Model()


# ------------------------------------------------------------------ the documented domain of the device path
def trip_figures(ts, s0, interval):
    """per 512-row trip of an ascending column at or above s0: (span of its rows from the start of its first row's window, windows
    between the row in front of the trip and its last row)"""
    n = len(ts)
    first = np.arange(0, n, TRIP)
    last = np.minimum(first + TRIP, n) - 1
    win = [(int(t) - s0) // interval for t in ts[first]]
    span = np.array([int(ts[b]) - (s0 + k * interval) for b, k in zip(last, win)], dtype=object)
    before = [0] + [(int(t) - s0) // interval for t in ts[first[1:] - 1]]
    crossed = np.array([(int(ts[b]) - s0) // interval - a for b, a in zip(last, before)], dtype=object)
    return span, crossed


def outside_inclusive_interpolate(ts, interval, offset):
    """None, or why inclusive Interpolate declines this frame (BOWGPU_ERR_UNSUPPORTED, -9).  From the inputs alone:
      * rows below s0, a window that starts at the reference's -1 sentinel, an interval of 2^31 and more, timestamps beyond 2^53:
        bow_amd/csrc/interpolate_api.cpp interp_prepare (interp_fast32 / interp_wide32, interpolate.hip:991-1001, and drop != 0)
      * a 512-row trip that spans 2^31 - 1 or more from the start of its first row's window, or that crosses 2^22 - 1 windows and more
        in one step, or whose outputs do not fit the 16-bit position table: interpolate_api.cpp interp_fill_impl (interpolate.hip:515, :522, :577, :606)
    "Fewer than two rows per window on average" is no condition of today's code - interp_wave3_kernel<true> lists up to 512 runs per
    trip (interpolate.hip:922), as many as a trip has rows - so it is not one here: such a frame has to be served."""
    s0, W = plan(ts, interval, offset)
    first, last = int(ts[0]), int(ts[-1])
    if W == 0 or first < s0:
        return "rows below s0"
    if s0 <= -1 and (-1 - s0) % interval == 0 and (-1 - s0) // interval < W:
        return "a window starts at -1"
    if interval >= 2 ** 31:
        return "interval of 2^31 and more"
    if first <= -2 ** 53 or last >= 2 ** 53:
        return "timestamps beyond 2^53"
    span, crossed = trip_figures(ts, s0, interval)
    if (span >= 2 ** 31 - 1).any():
        return "a trip spans 2^31"
    step = np.diff((ts - s0) // interval) if len(ts) > 1 else np.zeros(0, np.int64)
    if (crossed >= 0xFFFF - TRIP - 1).any() or (step >= 0x3FFFFF).any():
        return "a trip with 65 535 outputs or a gap of millions of empty windows"
    return None


def rows_below_s0_ride(ts, interval, offset):
    """rows below the first window start that window 0 takes along: the interpolated interval column then begins s0, ts[0] < s0, ...
    and Aggregate declines it (BOWGPU_ERR_TS_UNSORTED, -14: agg_pass.cpp fail_ts_unsorted; include/bowgpu.h:465-468, "including their
    declines")"""
    s0, W = plan(ts, interval, offset)
    if W == 0 or int(ts[0]) >= s0:
        return False
    a = int(np.searchsorted(ts, s0, side="left"))
    return a < len(ts) and int(ts[a]) < s0 + interval


def outside(case):
    """None, or (code, reason): the one predicate a device decline is checked against"""
    if case["kind"] == "fill":
        return None
    ts, interval, offset = case["ts"], case["interval"], case["offset"]
    if case["inclusive"]:
        why = outside_inclusive_interpolate(ts, interval, offset)
        if why:
            return -9, why
    if case["kind"] == "chain" and rows_below_s0_ride(ts, interval, offset):
        return -14, "the interpolated interval column is not ascending"
    return None


# ------------------------------------------------------------------ figures of a case (what the coverage conditions are stated in)
def longest_null_run(valid):
    if valid.all():
        return 0
    edges = np.flatnonzero(np.diff(np.concatenate(([1], valid.astype(np.int8), [1]))))
    return int((edges[1::2] - edges[::2]).max())


def fill_needs_the_index(valid):
    """a null run so long that some 512-row trip inside it cannot see its end within the near walk (64 words of 32 bits, less than a
    word lost to alignment): fill_api.cpp fill_finish repeats the kernel with the neighbour index built"""
    return longest_null_run(valid) >= NEAR_BITS + TRIP + 64


def run_crosses_a_block_edge(valid, pad):
    """a null run that lies across a multiple of 4096 in the bit numbering of the bitmap itself (Arrow offset `pad`)"""
    bits = np.arange(len(valid)) + pad
    edge = np.flatnonzero((bits % BLOCK_BITS == 0) & (np.arange(len(valid)) > 0))
    return bool((~valid[edge] & ~valid[edge - 1]).any())


def in_the_fused_shape(case):
    """include/bowgpu.h:460-464: exclusive windows of 4 .. 128 rows on average and none longer than 128, a frame at or above 0 that spans
    less than 2^32 - and (rolling_fused.hip gave_up) no neighbour point further away than the near walk"""
    ts, interval = case["ts"], case["interval"]
    if case["inclusive"] or int(ts[0]) < 0 or int(ts[-1]) - int(ts[0]) >= 2 ** 32 - interval:
        return False
    w = M.windows(ts, interval, case["offset"], False)
    if not 4 <= case["n"] / max(w.W, 1) <= 128 or int(w.length.max()) > 128:
        return False
    return all(longest_null_run(c[4]) < NEAR_BITS - 64 or ip["kind"] == "None" for c, ip in zip(case["raw"], case["interps"][1:]))


# ------------------------------------------------------------------ the cases
SIZES = [1, 2, 511, 512, 513, 1023, 1025, 2047, 2049, 4095, 4097, 8193, 20_000, 70_001]
CASES = {"interp": 24, "fill": 16, "chain": 24}      # per seed
WILD = 3                                             # the one case of a seed whose inclusive / chain frame may lie outside the domain
VALIDITY = ("iid", "runs", "long-run", "edge-runs", "ends-only", "all-null", "two-ends", "own")
ORACLE_BUDGET = 3e7                                  # windows x (longest null run)^2 up to which a case of <= 700 rows is drawn
MAX_WINDOWS = 300_000
SEED_BASE = {"interp": 21_000, "fill": 22_000, "chain": 23_000}
FUSED_SHAPED_MIN = 3                                 # chain cases of a seed inside the fused kernel's documented shape, at least (asserted on the CPU)
FUSED_FLOOR = 1                                      # ... of which rolling_fused_kernel has to serve at least this many (a third: a tile it cannot describe sends a call back)


def draw_size(rng):
    if rng.random() < 0.15:
        return int(rng.integers(1, 3000))
    return max(1, int(SIZES[int(rng.integers(0, len(SIZES)))]) + int(rng.integers(-1, 2)))


def value_validity(rng, n, pad, mode=None):
    """(bool[n] or None for "the column's own bits", mode): the five patterns of null_ts_cases.interval_validity, all null, valid only at
    the two ends; leading nulls (no previous row) in a third of the draws"""
    from null_ts_cases import interval_validity
    if mode is None:
        mode = VALIDITY[int(rng.choice(len(VALIDITY), p=[0.2, 0.12, 0.2, 0.15, 0.05, 0.06, 0.1, 0.12]))]
    if mode == "own":
        return None, mode
    if mode == "all-null":
        return np.zeros(n, bool), mode
    if mode == "two-ends":
        v = np.zeros(n, bool)
        v[0] = v[-1] = True
        return v, mode
    v, mode = interval_validity(rng, n, pad, mode=mode)
    if rng.random() < 0.35:
        v[:min(n, int(rng.integers(1, 100)) if rng.random() < 0.7 else int(rng.integers(2040, 4200)))] = False
    if rng.random() < 0.2:
        v[max(0, n - int(rng.integers(1, 100))):] = False
    return v, mode


def value_col(rng, n, pad, mode=None):
    """(v, bm, typ, off, valid bool[n], mode): rand_col's column with one of the patterns above in its own rows, junk bits around"""
    from test_gpu_fuzz import rand_col
    v, bm, typ, off = rand_col(rng, n, pad)
    if typ == INT64 and rng.random() < 0.3:               # integers float64 cannot hold: StepPrevious must not pass through float64
        v = rng.integers(-2 ** 62, 2 ** 62, len(v)).astype(np.int64)
    valid, mode = value_validity(rng, n, pad, mode)
    if valid is not None:
        bits = rng.random(len(v)) < 0.5 if bm is None else np.unpackbits(bm, bitorder="little")[:len(v)].astype(bool)
        bits[pad:pad + n] = valid
        bm = np.packbits(bits, bitorder="little")
    valid = np.ones(n, bool) if bm is None else np.unpackbits(bm, bitorder="little")[pad:pad + n].astype(bool)
    return v, bm, typ, off, valid, mode


def draw_ts(rng, n, wild, tame):
    """(ts, interval, offset, tags).  tame: a frame inside the domain of inclusive Interpolate and with nothing below s0 - non-negative,
    0 <= offset < interval, s0 <= ts[0], small scale."""
    from test_gpu_fuzz import rand_ts
    tags = []
    ts = rand_ts(rng, n)
    interval = int([1, 2, 5, 10, 64, 100, 1000, 12345][int(rng.integers(0, 8))])
    shape = rng.random()
    if n >= 2 and shape < 0.15:
        # thousands of empty windows in one step - beyond the queue of 4096 runs in half of the draws
        gap = int(rng.integers(1000, 4000)) if rng.random() < 0.5 else int(rng.integers(4097, 9000))
        ts = ts.copy()
        ts[int(rng.integers(1, n)):] += gap * interval
        tags.append("gap")
    elif n >= 2 and shape < 0.25:
        # few rows per window: trips with more outputs than the stage holds
        ts = np.cumsum(rng.integers(1, 8, n)).astype(np.int64) * int(rng.integers(2, 5)) + int(rng.integers(-2000, 2000))
        interval = int(rng.integers(1, 4))
        tags.append("sparse")
    elif n >= 2 and shape < 0.32 and not tame:
        # one trip that spans more than 2^31: an interval of millions, a step of billions
        interval = int(rng.integers(10 ** 6, 10 ** 9))
        ts = ts.copy()
        ts[int(rng.integers(1, n)):] += int(rng.integers(2 ** 31, 2 ** 33))
        tags.append("trip spans 2^31")
    ns = rng.random() < 0.2 and not tame
    if ns:     # nanosecond scale, as test_gpu_fuzz.aggregate_cases does it: far more than 2^32 (2^53 with the shift) from zero
        scale = int(10 ** rng.integers(5, 10)) + int(rng.integers(0, 3))
        ts = ts * scale + int(rng.integers(-2, 3)) * 1_500_000_000_000_000_000 // 2
        interval *= scale
        tags.append("ns")
    if tame:
        ts = ts - min(int(ts[0]), 0) + int(rng.integers(0, 50))
    while (int(ts[-1]) - int(ts[0])) // interval > MAX_WINDOWS:
        interval *= 10
    offset = int(rng.integers(0, interval)) if tame else int(rng.integers(-2 * interval, 2 * interval + 1))
    for _ in range(12):      # (a tame frame stays one inclusive Interpolate serves: no trip with 65 535 outputs)
        if not (tame and outside_inclusive_interpolate(ts, interval, offset)):
            break
        interval *= 10
    if not tame and not ns and n >= 3 and rng.random() < 0.12:
        # the -1 sentinel: a window starts at -1 and holds no row ("no first value" == its start: no synthetic row)
        ts = ts - int(ts[n // 2])
        offset = interval - 1
        hole = (ts >= -1) & (ts < interval - 1)
        ts = np.where(hole, -2, ts)
        tags.append("sentinel")
    s0, W = plan(ts, interval, offset)
    if W > 2 and rng.random() < 0.3:
        # duplicates sitting on a window start
        k = int(rng.integers(1, W))
        a = int(np.searchsorted(ts, s0 + k * interval))
        if 0 < a < n:
            ts = ts.copy()
            ts[a:min(n, a + int(rng.integers(1, 40)))] = s0 + k * interval
            tags.append("duplicates on a start")
    return ts.astype(np.int64), interval, offset, tags


def prev_row(rng, ts0):
    """Options.PrevRow with valid and with null halves: (t, t_valid, v, v_valid, v_i64)"""
    return (float(ts0 - int(rng.integers(1, 50))), bool(rng.random() < 0.8), 42.5, bool(rng.random() < 0.8), 42)


def oracle_cost(case):
    """windows x (longest null run)^2: what the oracle's restarting walks cost on this case"""
    W = plan(case["ts"], case["interval"], case["offset"])[1] if "interval" in case else 1
    return W * max([longest_null_run(c[4]) for c in case["raw"]] + [1]) ** 2


def frame_case(rng, seed, i, kind):
    wild = i == WILD
    inclusive = bool(rng.random() < (0.35 if kind == "interp" else 0.2)) or (wild and kind == "interp")
    n = draw_size(rng)
    fused = kind == "chain" and not wild and i % 2 == 0
    tame = (inclusive or kind == "chain") and not wild
    if fused:
        # the fused kernel's domain (include/bowgpu.h:460-464): exclusive windows of 4 .. 128 rows, a frame at or above 0
        inclusive = False
        n = max(n, 600)
        ts = (np.cumsum(rng.integers(0, int(rng.integers(2, 30)), n)) + int(rng.integers(0, 3000))).astype(np.int64)
        if rng.random() < 0.3:
            ts[n // 2:] += int(rng.integers(1000, 200_000))
        interval = max(1, int(max(int(ts[-1] - ts[0]), 1) / (n / float(rng.integers(5, 90)))))
        offset, tags = int(rng.integers(-2 * interval, 2 * interval + 1)), ["fused shape"]
    else:
        ts, interval, offset, tags = draw_ts(rng, n, wild, tame)
    pad = int(rng.integers(1, 70)) if rng.random() < 0.5 else 0
    ncols = int(rng.integers(1, 4)) if not fused else 1 + int(rng.random() < 0.4)
    raw = [value_col(rng, n, pad) for _ in range(ncols)]
    case = {"kind": kind, "n": n, "ts": ts, "interval": interval, "offset": offset, "inclusive": inclusive, "pad": pad, "raw": raw}
    while n <= 700 and oracle_cost(case) > ORACLE_BUDGET:      # (a small case stays affordable for the oracle: fewer windows)
        case["interval"] = interval = interval * 10
    junk = rng.integers(-2 ** 62, 2 ** 62, pad + n + 3).astype(np.int64)
    junk[pad:pad + n] = ts
    case["ts_buf"] = junk
    ip = [{"kind": "WindowStart", "col": 0}]
    for j in range(ncols):
        ip.append({"kind": ["Linear", "StepPrevious", "None"][int(rng.integers(0, 3))], "col": 1 + j})
        if rng.random() < 0.35:
            ip[-1]["prev"] = prev_row(rng, int(ts[0]))
    case["interps"] = ip
    case["device"] = bool(rng.random() < 0.4)
    case["stated"] = [bool(rng.random() < 0.5) for _ in raw]       # null_count stated, or -1
    case["tags"] = tags
    if kind == "chain":
        from test_gpu_aggregate import ALL_AGGS
        kinds = list(rng.choice(ALL_AGGS[1:], size=int(rng.integers(1, 7))))
        aggs = [("WindowStart", 0)] + [(str(k), int(rng.integers(0 if k in ("Count", "NumRows") else 1, ncols + 1))) for k in kinds]
        if rng.random() < 0.3:
            a = int(rng.integers(1, len(aggs)))
            aggs[a] = aggs[a] + ([float(rng.choice([2.0, -1.0, 0.5, 1e3]))],)
        case["aggs"] = aggs
    case["label"] = "%s seed=%d case=%d n=%d I=%d off=%d pad=%d incl=%d dev=%d %s %s %s" % (
        kind, seed, i, n, interval, offset, pad, inclusive, case["device"], [p["kind"] for p in ip[1:]], [c[5] for c in raw], tags)
    return case


def fill_case(rng, seed, i):
    n = draw_size(rng)
    pad = int(rng.integers(1, 70)) if rng.random() < 0.5 else 0
    col = value_col(rng, n, pad, mode="long-run" if i == 0 and n >= 4200 else None)
    # the reference column of FillLinear: sorted either way, ties (next_ref == prev_ref divides by zero), nulls, either type
    step = rng.integers(0, 3 if rng.random() < 0.5 else 20, n)
    ref = np.cumsum(step).astype(np.int64) + int(rng.integers(-5000, 5000))
    if rng.random() < 0.4:
        ref = ref[::-1].copy()
    rtyp = INT64 if rng.random() < 0.5 else FLOAT64
    rbuf = np.concatenate([rng.integers(-9, 9, pad), ref, rng.integers(-9, 9, 3)]).astype(np.int64)
    rbuf = rbuf if rtyp == INT64 else rbuf.astype(np.float64) * 0.5
    rbits = rng.random(pad + n + 3) < 0.5
    rvalid = rng.random(n) >= [0.0, 0.05, 0.3, 1.0][int(rng.choice(4, p=[0.35, 0.35, 0.25, 0.05]))]
    rbits[pad:pad + n] = rvalid
    rbm = None if rvalid.all() and rng.random() < 0.5 else np.packbits(rbits, bitorder="little")
    case = {"kind": "fill", "n": n, "pad": pad, "raw": [col], "ref": (rbuf, rbm, rtyp, pad, rvalid), "device": bool(rng.random() < 0.4),
            "stated": [bool(rng.random() < 0.5)], "tags": []}
    case["label"] = "fill seed=%d case=%d n=%d pad=%d dev=%d %s type=%d ref=%d" % (seed, i, n, pad, case["device"], col[5], col[2], rtyp)
    return case


def cases(seed, kind):
    """the seeded cases of one kind ("interp", "fill", "chain") as plain dicts; a function of the seed alone"""
    rng = np.random.default_rng(SEED_BASE[kind] + seed)
    return [fill_case(rng, seed, i) if kind == "fill" else frame_case(rng, seed, i, kind) for i in range(CASES[kind])]


# ------------------------------------------------------------------ a case as columns
def mcols(case):
    return [MCol(v[off:off + case["n"]], valid, typ) for v, bm, typ, off, valid, _mode in case["raw"]]


def ref_mcol(case):
    v, bm, typ, off, valid = case["ref"]
    return MCol(v[off:off + case["n"]], valid, typ)


def ocols(case):
    """the case for the oracle: [interval column,] value columns[, the reference column]"""
    n = case["n"]
    out = [orc.Column(case["ts_buf"], None, orc.INT64, offset=case["pad"], length=n)] if "ts_buf" in case else []
    out += [orc.Column(v, bm, typ, offset=off, length=n) for v, bm, typ, off, _valid, _mode in case["raw"]]
    if "ref" in case:
        v, bm, typ, off, _valid = case["ref"]
        out.append(orc.Column(v, bm, typ, offset=off, length=n))
    return out


def ccols(case):
    """the case for the C ABI (host- or device-resident); null_count stated or -1"""
    from bow_amd import capi
    n = case["n"]
    out = [capi.Column(case["ts_buf"], None, capi.INT64, case["pad"], n, 0)] if "ts_buf" in case else []
    for (v, bm, typ, off, valid, _mode), stated in zip(case["raw"], case["stated"]):
        out.append(capi.Column(v, bm, typ, off, n, int((~valid).sum()) if stated and bm is not None else -1 if bm is not None else 0))
    if "ref" in case:
        v, bm, typ, off, valid = case["ref"]
        out.append(capi.Column(v, bm, typ, off, n, -1 if bm is not None else 0))
    return [c.to_device() for c in out] if case["device"] else out
