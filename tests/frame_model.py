"""The frame operations of include/bowgpu.h (Bow.SortByCol ... Bow.OuterJoin) by their definitions, in numpy and plain Python, and a
generator of test plans over them.  Nothing here touches the library: the model is a second, independent statement of the header's
contract (no helper of the test_gpu_* files is used), and a plan is data - frames, arguments and the model's expectation for every
step - which tests/test_gpu_frame_fuzz.py executes through capi and tests/test_frame_model_cpu.py checks without a GPU.

A frame is a list of MCol(typ, bits: uint64[n], valid: bool[n]).  An INPUT column may hold anything under its null slots; every OUTPUT
has the shape Buffer.SetOrDropStrict leaves: 0 under null slots.  A decline is the value (code,)."""
from collections import namedtuple

import numpy as np

FLOAT64, INT64 = 1, 2                      # include/bowgpu.h BOWGPU_FLOAT64 / BOWGPU_INT64
HOST, DEVICE, PINNED = 0, 1, 2             # BOWGPU_HOST / BOWGPU_DEVICE / BOWGPU_HOST_PINNED
INNER, OUTER = 0, 1                        # BOWGPU_JOIN_INNER / BOWGPU_JOIN_OUTER
ERR_BAD_COL, ERR_TYPE, ERR_UNSUPPORTED, ERR_ARG, ERR_SORT_NULLS = -6, -7, -9, -10, -16

MCol = namedtuple("MCol", "typ bits valid")
DTYPE = {INT64: np.int64, FLOAT64: np.float64}
NAN_BITS = np.uint64(0x7FF8000000000BAD)   # a quiet NaN with a payload, the hostile value under null slots


def mcol(values, valid=None):
    values = np.ascontiguousarray(values)
    typ = INT64 if values.dtype == np.int64 else FLOAT64
    assert values.dtype in (np.int64, np.float64)
    return MCol(typ, values.view(np.uint64).copy(), np.ones(len(values), bool) if valid is None else np.asarray(valid, bool).copy())


def from_list(data, typ):
    """a Python list with None for nil; typ: "int64" / "float64" or the type code"""
    typ = {"int64": INT64, "float64": FLOAT64}.get(typ, typ)
    valid = np.array([x is not None for x in data], bool)
    return mcol(np.array([0 if x is None else x for x in data], DTYPE[typ]), valid)


def vals(c):
    return c.bits.view(DTYPE[c.typ])


def to_list(c):
    return [x if ok else None for x, ok in zip(vals(c).tolist(), c.valid.tolist())]


def rows_of(frame):
    return len(frame[0].bits) if frame else 0


def slice_frame(frame, first, count):
    """rows [first, first + count) of the INPUT columns, payloads under null slots included: what a contiguous answer stands for"""
    return [MCol(c.typ, c.bits[first:first + count], c.valid[first:first + count]) for c in frame]


def concat_frames(frames):
    return [MCol(cs[0].typ, np.concatenate([c.bits for c in cs]), np.concatenate([c.valid for c in cs])) for cs in zip(*frames)]


def declined(r):
    return isinstance(r, tuple) and len(r) == 1


class R(dict):
    """the model's answer to one call: counts and flags by name, `cols` (None: the outputs are not written), `idx` (index outputs),
    `mask` (a row bitmap as bools), `gen_nan` (Diff: per output column, the slots whose NaN the subtraction generated)"""
    __getattr__ = dict.get


class Model:
    # ---- the pieces a kernel could get subtly wrong: each one a method, so that a test can put a wrong one in its place
    def settle(self, bits, valid):
        """SetOrDropStrict: null slots hold 0"""
        return MCol(None, np.where(valid, bits, np.uint64(0)), valid)

    def pack(self, valid):
        """validity bytes, LSB first, the padding bits of the last byte clear"""
        return np.packbits(valid, bitorder="little") if len(valid) else np.zeros(0, np.uint8)

    def order(self, c):
        """the stable ascending permutation under Buffer.Less (-0.0 equals +0.0)"""
        v = vals(c)
        return np.argsort(v + 0.0 if c.typ == FLOAT64 else v, kind="stable")

    def equal(self, v, x):
        """Go's == of a column's values against one value: exact for Int64, IEEE for Float64 (a NaN equals nothing)"""
        return v == x

    def right_rows(self, rows):
        """the right rows of one key, in the order the pair list visits them"""
        return rows

    def right_only_key(self, bits, valid):
        return bits, valid

    def nil_search_start(self, row_start):
        return 0

    def select_cols(self, ncols, col_idx):
        """selectCols: none named means all; a repeated index counts once"""
        if any(i < 0 or i >= ncols for i in col_idx):
            return (ERR_BAD_COL,)
        return sorted(set(col_idx)) if len(col_idx) else list(range(ncols))

    def distinct_survivor(self, perm, heads):
        """which row of each group of equal values gives the stored bits (perm: the stable order, heads: where its groups begin): the
        last in row order (Go's map assignment rewrites the key)"""
        return perm[np.append(heads[1:], len(perm)) - 1]

    # ---- helpers
    def out(self, typ, bits, valid):
        s = self.settle(bits, valid)
        return MCol(typ, s.bits, s.valid)

    def gather(self, c, idx):
        """c at rows idx, -1: no row (a null)"""
        idx = np.asarray(idx, np.int64)
        if len(c.bits) == 0:
            return self.out(c.typ, np.zeros(len(idx), np.uint64), np.zeros(len(idx), bool))
        safe = np.where(idx >= 0, idx, 0)
        return self.out(c.typ, np.where(idx >= 0, c.bits[safe], np.uint64(0)), (idx >= 0) & c.valid[safe])

    @staticmethod
    def has_nan(c):
        return c.typ == FLOAT64 and bool(np.isnan(vals(c)[c.valid]).any())

    @staticmethod
    def is_sorted(c):
        v = vals(c)
        return not bool((v[1:] < v[:-1]).any())

    # ---- Bow.SortByCol
    def sort_decline(self, key):
        if (~key.valid).any():
            return (ERR_SORT_NULLS,)
        if self.has_nan(key):
            return (ERR_UNSUPPORTED,)
        return None

    def argsort(self, key):
        d = self.sort_decline(key)
        if d:
            return d
        if len(key.bits) < 2 or self.is_sorted(key):
            return R(sorted=1)
        return R(sorted=0, idx=[self.order(key).astype(np.int64)])

    def take(self, c, idx):
        idx = np.asarray(idx, np.int64)
        if ((idx < 0) | (idx >= len(c.bits))).any():
            return (ERR_ARG,)
        return R(cols=[self.gather(c, idx)])

    def sort_by_col(self, frame, key_col):
        if not 0 <= key_col < len(frame):
            return (ERR_BAD_COL,)
        r = self.argsort(frame[key_col])
        if declined(r):
            return r
        if r.sorted:
            return R(unchanged=1)
        return R(unchanged=0, cols=[self.gather(c, r.idx[0]) for c in frame])

    def sort_by_col_sharded(self, ranks, key_col):
        """the one-device model on the concatenation, cut back into the input rank lengths; merged_ranks: the destination ranks whose
        rows do not come in source-rank order (their pulled runs overlap and have to be merged)"""
        whole = concat_frames(ranks)
        r = self.sort_by_col(whole, key_col)
        if declined(r) or r.unchanged:
            return r
        lens = [rows_of(f) for f in ranks]
        ends = np.cumsum(lens)
        src = np.searchsorted(ends, self.order(whole[key_col]), side="right")
        out, merged = [], 0
        for n, e in zip(lens, ends):
            out.append(slice_frame(r.cols, e - n, n))
            s = src[e - n:e]
            merged += bool((s[1:] < s[:-1]).any())
        return R(unchanged=0, ranks=out, merged_ranks=merged)

    # ---- Bow.Filter
    def pred_rows(self, c, values, match_null):
        v = vals(c)
        hit = np.zeros(len(v), bool)
        for x in np.asarray(values, v.dtype):
            hit |= self.equal(v, x)
        return np.where(c.valid, hit, bool(match_null))

    def keep_of(self, frame, preds, and_mask):
        keep = np.ones(rows_of(frame), bool)
        for p in preds:
            if not 0 <= p[0] < len(frame):
                return (ERR_BAD_COL,)
            keep &= self.pred_rows(frame[p[0]], p[1], p[2] if len(p) > 2 else False)
        return keep if and_mask is None else keep & and_mask

    @staticmethod
    def mask_answer(keep):
        rows = np.flatnonzero(keep)
        return R(mask=keep, selected=len(rows), first=int(rows[0]) if len(rows) else -1, last=int(rows[-1]) if len(rows) else -1)

    def filter_mask(self, frame, preds, and_mask=None):
        keep = self.keep_of(frame, preds, and_mask)
        return keep if declined(keep) else self.mask_answer(keep)

    def compact(self, frame, keep, capacity=None):
        rows = np.flatnonzero(keep[:rows_of(frame)])
        if len(rows) == 0 or rows[-1] - rows[0] + 1 == len(rows):
            return R(contiguous=1, first=int(rows[0]) if len(rows) else 0, count=len(rows))
        if capacity is not None and capacity < len(rows):
            return (ERR_ARG,)
        return R(contiguous=0, first=int(rows[0]), count=len(rows), cols=[self.gather(c, rows) for c in frame])

    def filter(self, frame, preds, and_mask=None, capacity=None):
        keep = self.keep_of(frame, preds, and_mask)
        return keep if declined(keep) else self.compact(frame, keep, capacity)

    # ---- Bow.DropNils / Bow.Diff / Bow.Distinct
    def valid_keep(self, frame, col_idx, and_mask):
        sel = self.select_cols(len(frame), list(col_idx))
        if declined(sel):
            return sel
        keep = np.ones(rows_of(frame), bool)
        for i in sel:
            keep &= frame[i].valid
        return keep if and_mask is None else keep & and_mask

    def valid_mask(self, frame, col_idx=(), and_mask=None):
        keep = self.valid_keep(frame, col_idx, and_mask)
        return keep if declined(keep) else self.mask_answer(keep)

    def drop_nils(self, frame, col_idx=(), capacity=None):
        keep = self.valid_keep(frame, col_idx, None)
        return keep if declined(keep) else self.compact(frame, keep, capacity)

    def diff(self, frame, col_idx=()):
        sel = self.select_cols(len(frame), list(col_idx))
        if declined(sel):
            return sel
        cols, gen = [], []
        for i in sel:
            c = frame[i]
            n = len(c.bits)
            valid, bits, g = np.zeros(n, bool), np.zeros(n, np.uint64), np.zeros(n, bool)
            if n > 1:
                valid[1:] = c.valid[1:] & c.valid[:-1]
                if c.typ == INT64:
                    bits[1:] = c.bits[1:] - c.bits[:-1]                 # two's complement: wraps as Go's int64 does
                else:
                    v = vals(c)
                    with np.errstate(invalid="ignore", over="ignore"):
                        d = v[1:] - v[:-1]                              # one IEEE subtraction
                    bits[1:] = d.view(np.uint64)
                    g[1:] = valid[1:] & np.isnan(d) & ~np.isnan(v[1:]) & ~np.isnan(v[:-1])     # inf - inf: a NaN of the device's bits
            cols.append(self.out(c.typ, bits, valid))
            gen.append(g)
        return R(cols=cols, gen_nan=gen)

    def distinct(self, c, capacity=None):
        if self.has_nan(c):
            return (ERR_UNSUPPORTED,)
        rows = np.flatnonzero(c.valid)
        if len(rows) == 0:
            return R(n_distinct=0)
        live = MCol(c.typ, c.bits[rows], np.ones(len(rows), bool))
        perm = self.order(live)
        v = vals(live)[perm]
        heads = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
        if capacity is not None and capacity < len(heads):
            return (ERR_ARG,)
        keep = self.distinct_survivor(perm, heads)
        return R(n_distinct=len(heads), cols=[self.out(c.typ, live.bits[keep], np.ones(len(heads), bool))])

    # ---- AppendBows / Bow.FindNext
    def append(self, frames, capacity=None):
        for cs in zip(*frames):
            if any(c.typ != cs[0].typ for c in cs):
                return (ERR_TYPE,)
        if len(frames) == 1:
            return R(unchanged=1)
        total = sum(rows_of(f) for f in frames)
        if capacity is not None and capacity < total:
            return (ERR_ARG,)
        return R(unchanged=0, cols=[self.out(c.typ, c.bits, c.valid) for c in concat_frames(frames)])

    def find_next(self, c, value, row_start=0):
        n = len(c.bits)
        if value is None:
            hit = np.flatnonzero(~c.valid[self.nil_search_start(row_start):]) + self.nil_search_start(row_start)
        elif row_start >= n:
            return R(row=-1)
        else:
            hit = np.flatnonzero(c.valid[row_start:] & self.equal(vals(c)[row_start:], DTYPE[c.typ](value))) + row_start
        return R(row=int(hit[0]) if len(hit) else -1)

    # ---- Bow.InnerJoin / Bow.OuterJoin
    def join_rows(self, lk, rk, kind):
        if lk is None and rk is None:
            return R(rows=0, pairs=0, idx=[np.zeros(0, np.int64), np.zeros(0, np.int64)])
        if lk.typ != rk.typ:
            return (ERR_TYPE,)
        if self.has_nan(lk) or self.has_nan(rk):
            return (ERR_UNSUPPORTED,)
        where = {}
        for r, (x, ok) in enumerate(zip(vals(rk).tolist(), rk.valid.tolist())):
            where.setdefault(x if ok else None, []).append(r)       # (a float key: -0.0 and 0.0 are one key; None is nil)
        li, ri, pairs, hit = [], [], 0, np.zeros(len(rk.bits), bool)
        for l, (x, ok) in enumerate(zip(vals(lk).tolist(), lk.valid.tolist())):
            rows = where.get(x if ok else None)
            if rows:
                rows = self.right_rows(rows)
                pairs += len(rows)
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
        return R(rows=len(li), pairs=pairs, idx=[np.array(li, np.int64), np.array(ri, np.int64)])

    def join(self, left, lk, right, rk, kind, capacity=None):
        nl, nr = rows_of(left), rows_of(right)
        if lk == -1 and rk == -1:
            no = np.full
            li = np.concatenate([np.arange(nl), no(nr, -1)]).astype(np.int64) if kind == OUTER else np.zeros(0, np.int64)
            ri = np.concatenate([no(nl, -1), np.arange(nr)]).astype(np.int64) if kind == OUTER else np.zeros(0, np.int64)
            r = R(rows=len(li), pairs=0, idx=[li, ri])
        else:
            if not (0 <= lk < len(left) and 0 <= rk < len(right)):
                return (ERR_BAD_COL,)
            r = self.join_rows(left[lk], right[rk], kind)
            if declined(r):
                return r
            li, ri = r.idx
        if capacity is not None and capacity < r.rows:
            return (ERR_ARG,)
        cols = []
        for i, c in enumerate(left):
            g = self.gather(c, li)
            if i == lk:                      # a right-only row takes the RIGHT key's value and validity
                k = self.gather(right[rk], ri)
                kb, kv = self.right_only_key(k.bits, k.valid)
                g = self.out(c.typ, np.where(li >= 0, g.bits, kb), np.where(li >= 0, g.valid, kv))
            cols.append(g)
        cols += [self.gather(c, ri) for i, c in enumerate(right) if lk < 0 or i != rk]
        return R(rows=r.rows, pairs=r.pairs, cols=cols)


# ------------------------------------------------------------------ one step of a plan, run through a model
def run_step(model, step):
    """the model's answer to step = {"op", "frames": [[MCol]], "args": {...}}"""
    op, fr, a = step["op"], step["frames"], step["args"]
    f = fr[0] if fr else []
    if op == "argsort":
        return model.argsort(f[a["col"]])
    if op == "take":
        return model.take(f[a["col"]], a["idx"])
    if op == "sort_by_col":
        return model.sort_by_col(f, a["key"])
    if op == "sort_by_col_sharded":
        return model.sort_by_col_sharded(cut(f, a["cuts"]), a["key"])
    if op == "filter_mask":
        return model.filter_mask(f, a["preds"], a.get("and_mask"))
    if op == "compact":
        return model.compact(f, a["mask"], a.get("cap"))
    if op == "filter":
        return model.filter(f, a["preds"], a.get("and_mask"), a.get("cap"))
    if op == "valid_mask":
        return model.valid_mask(f, a["col_idx"], a.get("and_mask"))
    if op == "drop_nils":
        return model.drop_nils(f, a["col_idx"], a.get("cap"))
    if op == "diff":
        return model.diff(f, a["col_idx"])
    if op == "distinct":
        return model.distinct(f[a["col"]], a.get("cap"))
    if op == "append":
        return model.append(fr, a.get("cap"))
    if op == "find_next":
        return model.find_next(f[a["col"]], a["value"], a["row_start"])
    if op == "join_rows":
        return model.join_rows(fr[0][a["lk"]], fr[1][a["rk"]], a["kind"])
    if op == "join":
        return model.join(fr[0], a["lk"], fr[1], a["rk"], a["kind"], a.get("cap"))
    raise ValueError(op)


def cut(frame, lens):
    out, at = [], 0
    for n in lens:
        out.append(slice_frame(frame, at, n))
        at += n
    return out


def signature(model, r):
    """everything a comparison looks at, as a list of hashable items: two answers differ exactly when their signatures do"""
    if declined(r):
        return [("declined", r[0])]
    sig = [(k, int(v)) for k, v in sorted(r.items()) if isinstance(v, (int, np.integer, bool))]
    for c in (r.cols or []) + [c for f in (r.ranks or []) for c in f]:
        sig.append((c.typ, len(c.bits), int((~c.valid).sum()), c.bits.tobytes(), model.pack(c.valid).tobytes()))
    for i in r.idx or []:
        sig.append(i.tobytes())
    if r.mask is not None:
        sig.append(model.pack(r.mask).tobytes())
    for g in r.gen_nan or []:
        sig.append(g.tobytes())
    return sig


# ------------------------------------------------------------------ the generator of frames
ROW_COUNTS = [0, 1, 2, 63, 64, 65, 1023, 1025, 2047, 2049, 4095, 4096, 4097, 3 * 4096 + 17]
BIG_ROWS = (1 << 16) + 1
OFFSETS = [0, 1, 7, 8, 63, 64, 65]
DENSITIES = [0.0, 0.05, 0.3, 0.9, 1.0]
RESIDENCIES = [HOST, DEVICE, PINNED]
MOVE_COLS = 4                  # bow_amd/csrc/common.h kMoveCols: columns per launch group
NCOLS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9]
I64 = np.iinfo(np.int64)
INT_SHAPES = ["unique", "ties16", "extremes", "top byte", "low byte", "byte 3", "reversed", "few", "sorted ties"]
FLOAT_SHAPES = ["specials", "zeros", "ties", "few", "sorted ties"]
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 0.0, -0.0, 1.0, -1.0])


def pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def draw_rows(rng):
    return int(rng.integers(0, 3000)) if rng.random() < 0.3 else pick(rng, ROW_COUNTS)


def int_values(rng, n, shape):
    if shape == "unique":
        return rng.permutation(n).astype(np.int64)
    if shape == "ties16":
        return rng.integers(0, 16, n).astype(np.int64)
    if shape == "extremes":
        v = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
        if n >= 4:
            v[rng.integers(0, n, 2)] = I64.min
            v[rng.integers(0, n, 2)] = I64.max
            v[rng.integers(0, n, 2)] = [0, -1]
        return v
    if shape == "top byte":
        return (rng.integers(-128, 128, n).astype(np.int64) << 56) | 0x1234
    if shape == "low byte":
        return rng.integers(0, 256, n).astype(np.int64) + (0x1122334455 << 8)
    if shape == "byte 3":
        return (rng.integers(0, 256, n).astype(np.int64) << 24) | 0x5500AABBCC
    if shape == "reversed":
        return np.arange(n, 0, -1, dtype=np.int64)
    if shape == "few":
        return np.array([-7, 0, I64.max], np.int64)[rng.integers(0, 3, n)]
    return np.sort(rng.integers(0, max(n // 3, 1), n)).astype(np.int64)          # already in order, with ties


def float_values(rng, n, shape):
    if shape == "specials":
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
        if n >= 4:
            at = rng.integers(0, n, min(n, 200))
            v[at] = SPECIALS[rng.integers(0, len(SPECIALS), len(at))]
        return v
    if shape == "zeros":
        return np.where(rng.random(n) < 0.5, 0.0, -0.0)
    if shape == "ties":
        return rng.integers(-3, 4, n).astype(np.float64) / 2
    if shape == "few":
        return np.array([-0.0, 0.0, np.inf, -2.5])[rng.integers(0, 4, n)]
    v = np.sort(rng.integers(-2, max(n // 3, 1), n)).astype(np.float64)          # already in order, with ties and both zeros
    return np.where((v == 0) & (rng.random(n) < 0.5), -0.0, v)


def gen_col(rng, n, typ=None, shape=None, density=None, nan_ok=True, clean=False):
    """(MCol, phys): phys says how the column lies in memory - Arrow offset, bitmap present or absent, null_count stated or -1,
    residency.  clean: no nulls and no NaN (a column a sort accepts).  The payloads under null slots are hostile."""
    typ = typ or pick(rng, [INT64, FLOAT64])
    shape = shape or pick(rng, INT_SHAPES if typ == INT64 else FLOAT_SHAPES)
    v = int_values(rng, n, shape) if typ == INT64 else float_values(rng, n, shape)
    density = 0.0 if clean else pick(rng, DENSITIES) if density is None else density
    valid = rng.random(n) >= density
    if typ == FLOAT64 and nan_ok and not clean and n and rng.random() < 0.25:
        v[rng.integers(0, n, 1 + n // 100)] = np.nan          # valid NaNs in a value column move as raw payloads
    bits = v.view(np.uint64).copy()
    dead = np.flatnonzero(~valid)
    if len(dead):
        live = np.flatnonzero(valid)
        how = int(rng.integers(0, 3))
        if how == 0 or len(live) == 0:
            bits[dead] = NAN_BITS
        elif how == 1:
            bits[dead] = bits[live[rng.integers(0, len(live), len(dead))]]        # values that are valid elsewhere in the column
        # (how == 2: the generated values stay - for the ordered shapes the very values of the neighbours)
    phys = {"offset": pick(rng, OFFSETS), "bitmap": bool(len(dead)) or rng.random() < 0.5, "known": rng.random() < 0.5,
            "res": pick(rng, RESIDENCIES)}
    return MCol(typ, bits, valid), phys


def gen_frame(rng, n, ncols=None, special=None, **kw):
    """ncols columns of n rows; special: {index: gen_col keywords} for the columns an operation has plans for"""
    ncols = ncols or pick(rng, NCOLS)
    cols, phys = [], []
    for i in range(ncols):
        c, p = gen_col(rng, n, **dict(kw, **((special or {}).get(i, {}))))
        cols.append(c)
        phys.append(p)
    return cols, phys


def poison(rng, c, values):
    """put `values` (the predicate set, the searched value) under some null slots of c"""
    dead = np.flatnonzero(~c.valid)
    if len(dead) and len(values):
        at = dead[rng.random(len(dead)) < 0.5]
        c.bits[at] = np.asarray(values, DTYPE[c.typ]).view(np.uint64)[rng.integers(0, len(values), len(at))]


def a_column(rng, ncols):
    """a column index that favours the last launch group of a wide frame"""
    return ncols - 1 if rng.random() < 0.4 else int(rng.integers(0, ncols))


def clean_cols(frame):
    return [i for i, c in enumerate(frame) if c.valid.all() and not Model.has_nan(c)]


def sample_values(rng, c, k, misses=True):
    """k values for a predicate set or a search: values of the column (valid or under a null), misses, a NaN"""
    v = vals(c)
    out = [v[int(rng.integers(0, len(v)))] for _ in range(k) if len(v)]
    if misses:
        out += [DTYPE[c.typ](x) for x in ([123456789, -5][:int(rng.integers(0, 3))])]
        if c.typ == FLOAT64 and (rng.random() < 0.3 or Model.has_nan(c)):
            out.append(np.nan)
    return np.array(out, DTYPE[c.typ])


# ------------------------------------------------------------------ arguments of one operation on a given frame
M = Model()


def args_filter(rng, frame, with_mask=True, hostile=True):
    n, preds, and_mask = rows_of(frame), [], None
    flavour = rng.random()
    if with_mask and flavour < 0.25 and n:                    # the caller's bitmap alone, one run of rows: a contiguous answer
        a, b = sorted(rng.integers(0, n + 1, 2).tolist())
        and_mask = np.zeros(n, bool)
        and_mask[a:b] = True
        return {"preds": preds, "and_mask": and_mask}
    nans = [i for i, c in enumerate(frame) if Model.has_nan(c)]
    if nans and rng.random() < 0.5:                           # a NaN in the set, NaNs among the column's valid rows: no match
        i = pick(rng, nans)
        return {"preds": [(i, np.append(sample_values(rng, frame[i], 1, misses=False), np.nan), False)], "and_mask": None}
    for _ in range(int(rng.integers(1, 4))):
        i = a_column(rng, len(frame))
        few = len(np.unique(frame[i].bits[:4096])) < 20
        values = sample_values(rng, frame[i], int(rng.integers(0, 3 if few else 6)))
        if hostile:
            poison(rng, frame[i], values)
        preds.append((i, values, bool(rng.random() < 0.4)))
    if with_mask and flavour > 0.8:
        and_mask = rng.random(n) < 0.7
    return {"preds": preds, "and_mask": and_mask}


def args_col_idx(rng, frame):
    """selectCols arguments: none, some, some repeated"""
    nc, how = len(frame), rng.random()
    if how < 0.2:
        return []
    idx = [a_column(rng, nc) for _ in range(int(rng.integers(1, min(nc, 3) + 1)))]
    if how > 0.55:
        idx += [idx[0]] if how < 0.8 or len(set(idx)) == 1 else idx
    return idx


def gen_right(rng, left, lk, right_rows=None):
    """a right frame for a join against left[lk]: the key drawn from the left key's values plus misses, nulls where the left has some"""
    lkey = left[lk]
    for attempt in range(2):
        nr = draw_rows(rng) if right_rows is None else right_rows
        nr = min(nr, 4200)
        ncols = pick(rng, NCOLS)
        rk = a_column(rng, ncols)
        cols, phys = gen_frame(rng, nr, ncols, special={rk: {"typ": lkey.typ, "density": 0.0}})
        lv = vals(lkey)[lkey.valid]
        lv = lv[~np.isnan(lv)] if lkey.typ == FLOAT64 else lv
        key = np.empty(nr, DTYPE[lkey.typ])
        from_left = (rng.random(nr) < 0.7) & (len(lv) > 0)
        key[:] = (np.arange(nr) * 7 + 1000003).astype(DTYPE[lkey.typ])          # misses
        if len(lv):
            key[from_left] = lv[rng.integers(0, len(lv), int(from_left.sum()))]
        if attempt == 1:                  # too many pairs: every right key once, one null at the most
            key = np.unique(key + 0 if lkey.typ == INT64 else key + 0.0)
            nr = len(key)
            cols, phys = gen_frame(rng, nr, ncols, special={rk: {"typ": lkey.typ, "density": 0.0}})
        if rng.random() < 0.4:
            key = np.sort(key)            # the time-series case: the right key already in order
        valid = np.ones(nr, bool)
        if not lkey.valid.all() or rng.random() < 0.5:
            k = 1 if attempt == 1 else max(1, nr // 20)
            valid[rng.integers(0, max(nr, 1), min(k, nr))] = False
        bits = key.view(np.uint64).copy()
        bits[~valid] = NAN_BITS if rng.random() < 0.5 or not len(lv) else lv[:1].view(np.uint64)[0]
        cols[rk] = MCol(lkey.typ, bits, valid)
        phys[rk]["bitmap"] = phys[rk]["bitmap"] or not valid.all()
        nulls = int((~lkey.valid).sum()) * int((~valid).sum())
        counts = dict(zip(*np.unique(key[valid], return_counts=True)))
        pairs = nulls + sum(counts.get(x, 0) for x in lv.tolist()) if len(counts) < 200000 else 0
        if pairs <= 30000:
            break
    return cols, phys, rk


def fresh(cols, phys):
    return {"cols": cols, "phys": phys}


def plan_op(rng, op, n, decline=None):
    """one single-operation case on fresh frames -> step (frames, args, physical placement, out residency)"""
    out_res = pick(rng, RESIDENCIES)
    step = {"op": op, "args": {}, "out_res": out_res, "tags": set()}
    a = step["args"]
    if op in ("argsort", "sort_by_col", "sort_by_col_sharded"):
        ncols = 1 if op == "argsort" else pick(rng, NCOLS)
        k = a_column(rng, ncols)
        if decline in ("nan key", "null key"):
            n = max(n, 2)
        spec = {"clean": True}
        if decline == "nan key":
            spec = {"clean": True, "typ": FLOAT64}
        if decline == "null key":
            spec = {"density": pick(rng, [0.05, 0.3]), "nan_ok": False}
        cols, phys = gen_frame(rng, n, ncols, special={k: spec})
        if decline == "nan key":
            cols[k].bits[rng.integers(0, n)] = NAN_BITS
        if decline == "null key":
            cols[k].valid[rng.integers(0, n)] = False
            phys[k]["bitmap"] = True
        step["inputs"] = [fresh(cols, phys)]
        a["col" if op == "argsort" else "key"] = k
        if op == "sort_by_col_sharded":
            a["cuts"] = rank_cuts(rng, n)
    elif op == "take":
        cols, phys = gen_frame(rng, n, 1)
        m = draw_rows(rng) if n else 0
        idx = rng.integers(0, max(n, 1), m).astype(np.int64)
        if decline == "take index":
            idx = np.append(idx, [n if rng.random() < 0.5 else -1]).astype(np.int64)
            rng.shuffle(idx)
        step["inputs"] = [fresh(cols, phys)]
        a.update(col=0, idx=idx, idx_res=pick(rng, [HOST, DEVICE]))
    elif op in ("filter_mask", "filter", "compact"):
        cols, phys = gen_frame(rng, n)
        step["inputs"] = [fresh(cols, phys)]
        a.update(args_filter(rng, cols))
        a["mask_res"] = pick(rng, RESIDENCIES)
        if op == "compact":
            keep = M.keep_of(cols, a["preds"], a["and_mask"])
            a.clear()
            a.update(mask=keep, mask_res=pick(rng, RESIDENCIES))
    elif op in ("valid_mask", "drop_nils", "diff"):
        infs = {0: {"typ": FLOAT64, "shape": "few"}} if op == "diff" and rng.random() < 0.35 else None      # inf - inf
        cols, phys = gen_frame(rng, n, nan_ok=op != "diff", special=infs)
        step["inputs"] = [fresh(cols, phys)]
        a["col_idx"] = args_col_idx(rng, cols)
        if op == "valid_mask":
            a["and_mask"] = rng.random(n) < 0.8 if rng.random() < 0.3 else None
            a["mask_res"] = pick(rng, RESIDENCIES)
            a["want_mask"] = rng.random() < 0.85
    elif op == "distinct":
        shape = {"typ": FLOAT64, "shape": pick(rng, ["zeros", "few", "sorted ties", "ties"])} if rng.random() < 0.4 else {}
        cols, phys = gen_frame(rng, n, 1, nan_ok=False, special={0: shape})
        if decline == "nan key":
            cols, phys = gen_frame(rng, max(n, 2), 1, nan_ok=False, special={0: {"typ": FLOAT64, "density": 0.05}})
            at = int(rng.integers(0, max(n, 2)))
            cols[0].bits[at] = NAN_BITS
            cols[0].valid[at] = True
        step["inputs"] = [fresh(cols, phys)]
        a["col"] = 0
    elif op == "append":
        ncols = pick(rng, NCOLS)
        npieces = pick(rng, [1, 2, 2, 3, 5, 9])
        first, _ = gen_frame(rng, 0, ncols)
        pieces = []
        for p in range(npieces):
            m = 0 if rng.random() < 0.25 else draw_rows(rng) if p < 3 else int(rng.integers(0, 200))
            pieces.append(gen_frame(rng, m, ncols, special={i: {"typ": c.typ} for i, c in enumerate(first)}))
        if decline == "append type":
            if npieces == 1:
                pieces.append(gen_frame(rng, 5, ncols, special={i: {"typ": c.typ} for i, c in enumerate(first)}))
            i = a_column(rng, ncols)
            m = rows_of(pieces[-1][0])
            pieces[-1][0][i], pieces[-1][1][i] = gen_col(rng, m, typ=INT64 + FLOAT64 - first[i].typ)
        step["inputs"] = [fresh(c, p) for c, p in pieces]
    elif op == "find_next":
        how = rng.random()
        cols, phys = gen_frame(rng, n, 1, special={0: {"density": pick(rng, [0.05, 0.3, 0.9])}} if how < 0.35 else None)
        c = cols[0]
        if how < 0.35:
            value = None
        elif how < 0.45 and c.typ == FLOAT64:
            value = float("nan")
        else:
            value = sample_values(rng, c, 1, misses=False)
            value = value[0].item() if len(value) and rng.random() < 0.85 else 424242
            if value != value:
                value = 0.0
            poison(rng, c, [value])
        # row_start in the middle of a validity word of the (sliced) column, at its ends, past the end
        row_start = pick(rng, [0, 0, n // 2, max(n - 1, 0), int(rng.integers(0, n + 1)), min(n, 37), n + 3])
        if value is None:                 # nil is searched from row 0 whatever row_start says: a row_start behind the first null
            row_start = pick(rng, [n // 2, max(n - 1, 0), int(rng.integers(0, max(n, 1)))])
        step["inputs"] = [fresh(cols, phys)]
        a.update(col=0, value=value, row_start=row_start)
    elif op in ("join_rows", "join"):
        nl = min(n, 4200)
        ncols = 1 if op == "join_rows" else pick(rng, NCOLS)
        lk = a_column(rng, ncols)
        spec = {"nan_ok": False, "density": pick(rng, [0.0, 0.05, 0.3])}
        if rng.random() < 0.5:
            spec["shape"] = "unique" if rng.random() < 0.5 else "sorted ties"
        left, lphys = gen_frame(rng, nl, ncols, special={lk: spec})
        if left[lk].typ == FLOAT64 and spec.get("shape") == "unique":
            left[lk], lphys[lk] = gen_col(rng, nl, typ=INT64, **spec)
        right, rphys, rk = gen_right(rng, left, lk)
        if op == "join_rows":
            right, rphys, rk = [right[rk]], [rphys[rk]], 0
        kind = pick(rng, [INNER, OUTER])
        if decline == "nan key" and (left[lk].typ != FLOAT64 or not nl or not rows_of(right)):
            left, lphys = gen_frame(rng, max(nl, 3), ncols, special={lk: {"typ": FLOAT64, "clean": True}})
            right, rphys, rk = gen_right(rng, left, lk, right_rows=max(min(rows_of(right), 300), 2))
            if op == "join_rows":
                right, rphys, rk = [right[rk]], [rphys[rk]], 0
        if decline == "nan key":
            side = right[rk] if rng.random() < 0.5 else left[lk]
            at = int(rng.integers(0, len(side.bits)))
            side.bits[at] = NAN_BITS
            side.valid[at] = True
        if op == "join" and decline is None and rng.random() < 0.08:
            lk = rk = -1                  # no common column
        step["inputs"] = [fresh(left, lphys), fresh(right, rphys)]
        a.update(lk=lk, rk=rk, kind=kind)
    else:
        raise ValueError(op)
    step["frames"] = [f["cols"] for f in step["inputs"]]
    finish(rng, step, decline)
    return step


CAP_OPS = ("compact", "filter", "drop_nils", "distinct", "append", "join")


def finish(rng, step, decline=None):
    """the expectation; a capacity one too small where that is the planned decline; the tags the coverage conditions count"""
    step["expect"] = r = run_step(M, step)
    if decline == "capacity" and not declined(r) and step["op"] in CAP_OPS:
        need = r.rows if step["op"] == "join" else r.n_distinct if step["op"] == "distinct" else \
            rows_of(r.cols) if step["op"] == "append" and r.cols else r.count
        if r.cols and need:
            step["args"]["cap"] = need - 1
            step["expect"] = r = run_step(M, step)
            assert r == (ERR_ARG,)
    step["decline"] = decline if declined(r) else None
    tag(step)


def tag(step):
    r, a, op, t = step["expect"], step["args"], step["op"], step["tags"]
    frames = step["frames"]
    t.add("op:" + op)
    if declined(r):
        t.add("declined")
        return
    if r.contiguous:
        t.add("contiguous")
    if r.unchanged:
        t.add("unchanged")
    if op in ("join", "join_rows") and a["lk"] >= 0:
        if (~frames[0][a["lk"]].valid).any() and (~frames[1][a["rk"]].valid).any():
            t.add("join null keys both sides kind %d" % a["kind"])
    if op == "distinct" and not declined(r):
        c = frames[0][a["col"]]
        z = c.bits[c.valid & (vals(c) == 0)] if c.typ == FLOAT64 else []
        if len(set(np.asarray(z).tolist())) == 2:
            t.add("distinct both zeros")
    if op == "diff" and any(g.any() for g in r.gen_nan):
        t.add("diff generates NaN")
    if op == "sort_by_col_sharded" and r.merged_ranks:
        t.add("sharded merge")
    third = 2 * MOVE_COLS
    named = [a.get("key", -1), a.get("lk", -1)] + [p[0] for p in a.get("preds", [])] + list(a.get("col_idx", []))
    named.append(a.get("rk", -1))
    if any(i >= third for i in named):
        t.add("third launch group")
    for f in step.get("inputs", []):
        for p in f["phys"] or []:
            t.add("offset:%d" % p["offset"])
    ins = [f for f in step.get("inputs", []) if f["phys"]]
    if ins:
        t.add("res:%d%d%d" % (ins[0]["phys"][0]["res"], ins[-1]["phys"][-1]["res"], step["out_res"]))


def rank_cuts(rng, n):
    """1 to 6 ranks of random lengths, empty ranks included"""
    world = int(rng.integers(1, 7))
    at = np.sort(rng.integers(0, n + 1, world - 1)) if rng.random() < 0.8 else np.sort(rng.integers(0, 2, world - 1) * n)
    return np.diff(np.concatenate([[0], at, [n]])).astype(int).tolist()


# ------------------------------------------------------------------ chains
CHAIN_OPS = ["filter", "drop_nils", "sort_by_col", "sort_by_col_sharded", "diff", "distinct", "append", "join"]


def chain_step(rng, op, frame, out_res, force=None):
    """one chain step on the chain's current frame (model columns; the executor holds the physical ones) -> step or None"""
    step = {"op": op, "args": {}, "out_res": out_res, "tags": set(), "inputs": [{"cols": frame, "phys": None}]}
    a, n, nc = step["args"], rows_of(frame), len(frame)
    if op == "filter":
        a.update(args_filter(rng, frame, hostile=False))      # (the frame already lies in memory: its null slots stay as they are)
    elif op == "drop_nils":
        a["col_idx"] = args_col_idx(rng, frame)
    elif op in ("sort_by_col", "sort_by_col_sharded"):
        ok = clean_cols(frame)
        if not ok:
            if rng.random() > 0.1 or n < 2:
                return None
            ok = list(range(nc))          # a planned decline: a null or a NaN in the key ends the chain
        a["key"] = nc - 1 if nc - 1 in ok and rng.random() < 0.4 else pick(rng, ok)
        if op == "sort_by_col_sharded":
            a["cuts"] = rank_cuts(rng, n)
    elif op == "diff":
        gen = M.diff(frame).gen_nan
        ok = [i for i, c in enumerate(frame) if not gen[i].any() and not (c.typ == FLOAT64 and np.isnan(vals(c)[c.valid]).any())]
        if not ok:
            return None
        k = int(rng.integers(1, len(ok) + 1))
        a["col_idx"] = [] if len(ok) == nc and rng.random() < 0.3 else sorted(rng.permutation(ok)[:k].tolist())
    elif op == "distinct":
        ok = [i for i, c in enumerate(frame) if not M.has_nan(c)]
        if not ok:
            return None
        a["col"] = pick(rng, ok)
    elif op == "append":
        pieces = [frame]
        for _ in range(pick(rng, [0, 1, 1, 2, 3])):
            m = 0 if rng.random() < 0.3 else draw_rows(rng)
            cols, phys = gen_frame(rng, min(m, 4200), nc, special={i: {"typ": c.typ} for i, c in enumerate(frame)})
            step["inputs"].insert(int(rng.integers(0, len(step["inputs"]) + 1)), fresh(cols, phys))
    elif op == "join":
        ok = [i for i, c in enumerate(frame) if not M.has_nan(c)]
        if not ok:
            return None
        lk = nc - 1 if nc - 1 in ok and rng.random() < 0.4 else pick(rng, ok)
        right, rphys, rk = gen_right(rng, frame, lk)
        step["inputs"].append(fresh(right, rphys))
        a.update(lk=lk, rk=rk, kind=pick(rng, [INNER, OUTER]))
    a.update(force or {})
    step["self"] = [i for i, f in enumerate(step["inputs"]) if f["phys"] is None][0]       # where the chain's own frame stands
    step["frames"] = [f["cols"] for f in step["inputs"]]
    finish(rng, step)
    if not declined(step["expect"]) and step["expect"].rows and step["expect"].rows > 40000:
        return None
    return step


def advance(step):
    """the frame(s) the next step reads: ("outs", frame) the outputs through out_as_column; ("slice", frame, first, count) rows of
    this step's input columns; ("same", frame) the input itself; ("ranks", frames) the rank outputs of a sharded sort; None: the end"""
    r, f = step["expect"], step["frames"][step.get("self", 0)]
    if declined(r):
        return None
    op = step["op"]
    if op == "find_next":
        return ("same", f)
    if op == "distinct":
        return ("outs", r.cols) if r.n_distinct else None
    if r.contiguous:
        return ("slice", slice_frame(f, r.first, r.count), r.first, r.count)
    if r.unchanged:
        return ("same", f)
    if op == "sort_by_col_sharded":
        return ("ranks", r.ranks)
    return ("outs", r.cols)


def plan_chain(rng, length, out_res, ops=None, start=None):
    cols, phys = start or gen_frame(rng, min(draw_rows(rng), 4200))
    state, steps, planned = ("fresh", cols), [], 0
    inputs0 = fresh(cols, phys)
    complete = True
    while planned < length:
        frame = state[1]
        if state[0] == "ranks":               # the shards of a sharded sort are put together again by AppendBows
            step = {"op": "append", "args": {}, "out_res": out_res, "tags": set(),
                    "inputs": [{"cols": f, "phys": None} for f in frame]}
            step["frames"] = frame
            finish(rng, step)
            step["self"] = 0
        else:
            op, force = ops[planned] if ops else (pick(rng, CHAIN_OPS), None)
            step = None
            for _ in range(8):
                step = chain_step(rng, op, frame, out_res, force)
                if step is not None:
                    break
                op, force = pick(rng, ["filter", "drop_nils", "append"]), None
            planned += 1
        if not steps:
            step["inputs"][step["self"]] = inputs0
        if state[0] in ("slice", "same") and steps:
            step["tags"].add("fed by " + ("contiguous" if state[0] == "slice" else "unchanged"))
        steps.append(step)
        nxt = advance(step)
        if nxt is not None and step["op"] == "distinct" and nxt[0] == "outs":
            c = nxt[1][0]
            find = {"op": "find_next", "out_res": out_res, "tags": set(), "inputs": [{"cols": nxt[1], "phys": None}],
                    "args": {"col": 0, "value": None if rng.random() < 0.2 else vals(c)[int(rng.integers(0, len(c.bits)))].item(),
                             "row_start": int(rng.integers(0, len(c.bits) + 1))}}
            if find["args"]["value"] is None:
                find["args"]["row_start"] = 0
            find["frames"] = [nxt[1]]
            finish(rng, find)
            steps.append(find)
        step["next"] = nxt if nxt is None else (nxt[0],) + tuple(nxt[2:])
        if nxt is None:
            complete = planned >= length
            break
        state = nxt
    return {"steps": steps, "out_res": out_res, "length": length, "complete": complete, "final": state}


ENTRY_POINTS = ["argsort", "take", "sort_by_col", "sort_by_col_sharded", "filter_mask", "compact", "filter", "valid_mask", "drop_nils",
                "diff", "distinct", "append", "find_next", "join_rows", "join"]
DECLINES = {"nan key": ["argsort", "sort_by_col", "sort_by_col_sharded", "distinct", "join", "join_rows"],
            "null key": ["argsort", "sort_by_col", "sort_by_col_sharded"], "append type": ["append"], "take index": ["take"],
            "capacity": list(CAP_OPS)}
EXTRA_OPS = 7                   # single-operation cases per seed beyond one of every entry point
CHAINS = 3                      # chains per seed: two with DEVICE outputs between the steps, one with HOST


def plans(seed):
    """the cases of one seed: ("op", step) for every entry point and a few more, then ("chain", chain)"""
    rng = np.random.default_rng(0xF4A3E + seed)
    ops = list(rng.permutation(ENTRY_POINTS)) + [pick(rng, ENTRY_POINTS) for _ in range(EXTRA_OPS)]
    big = int(rng.integers(0, len(ops))) if seed % 8 == 3 else -1
    for i, op in enumerate(ops):
        decline = None
        if rng.random() < (1 / 4 if op in ("append", "take") else 1 / 6):
            kinds = [k for k, where in DECLINES.items() if op in where]
            decline = pick(rng, kinds) if kinds else None
        n = BIG_ROWS if i == big and op in ("argsort", "filter", "drop_nils", "diff", "distinct", "find_next") else draw_rows(rng)
        yield "op", plan_op(rng, str(op), n, decline)
    for i in range(CHAINS):
        yield "chain", plan_chain(rng, int(rng.integers(3, 7)), DEVICE if i < 2 else HOST)


def rolling_plan(seed):
    """a chain that ends sorted by its Int64 column 0 with DEVICE outputs - drop_nils, filter, sort - for the rolling call behind it"""
    rng = np.random.default_rng(0x70111 + seed)
    n = pick(rng, [2049, 4097, 3000])
    ts, tp = gen_col(rng, n, typ=INT64, shape="ties16" if seed % 2 else "unique", density=0.05)
    v1, p1 = gen_col(rng, n, typ=FLOAT64, shape="ties", density=0.3, nan_ok=False)
    v2, p2 = gen_col(rng, n, typ=INT64, shape="few", density=0.05)
    v2 = MCol(INT64, (vals(v2) % 1000).view(np.uint64), v2.valid)
    chain = None
    while chain is None or not chain["complete"] or chain["steps"][-1]["expect"].unchanged:
        chain = plan_chain(rng, 3, DEVICE, ops=[("drop_nils", {"col_idx": [0]}), ("filter", None), ("sort_by_col", {"key": 0})], start=([ts, v1, v2], [tp, p1, p2]))
    return chain
