"""Vectorised numpy models of the per-row half of Bow.Equal (bow.go:227-275), of the Prev / Next valid-row getters
(bowgetters.go:65-151) and of IsColEmpty (bowassertion.go:84-86), and the seeded case plan the GPU fuzz draws from.

The models work over LOGICAL columns: (values, valid) pairs - values an int64 / float64 / bool array, valid a bool array or None (no
bitmap).  A PCol is a column as it lies in memory: buffers with junk in front of and behind the rows, an Arrow offset per column, the
validity as an unpacked bool array.  PCol.logical() slices it.  tests/test_equal_model_cpu.py proves the models against row loops
written from the quoted Go lines and shows that the plan's cases tell deliberately wrong variants (the `flaw` arguments) apart."""
import numpy as np

EQUAL_GO, EQUAL_BITS = 0, 1
T = 4096   # rows per tile (bow_amd/csrc/common.h kFilterTileRows)
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 12289]   # word, batch, wave and tile edges
OFFSETS = [0, 1, 7, 8, 31, 32, 33, 63]
NCOLS = [1, 4, 5, 9]            # one group, a full group, groups + 1
RESIDENCIES = ["host", "device", "pinned"]
EQUAL_FLAWS = ["null_slots", "nan_equal_go", "negzero_equal_bits", "lowest_col_overall", "right_offset"]
VALID_ROW_FLAWS = ["start_word", "past_length"]
FAMILIES = ["identical", "value_diff", "valid_diff", "under_null", "ones_vs_none", "two_groups", "same_row_two_cols", "int_bits",
            "nan_same", "nan_payload", "negzero", "identical_nulls"]
VR_FAMILIES = ["at_start", "same_word", "next_word", "other_tile", "none", "interleave", "row0", "last_row"]


# ------------------------------------------------------------------ columns as they lie in memory
class PCol:
    """typ: 'int64' | 'float64' | 'bool' | 'utf8' (bitmap only).  values: the physical array (bool: one bool per bit), bits: the
    physical validity (one bool per bit) or None; rows are [offset, offset + length) of both.  known: null_count is stated"""

    def __init__(self, typ, values, bits, offset, length, known=True):
        self.typ, self.values, self.bits, self.offset, self.length, self.known = typ, values, bits, offset, length, known

    def logical(self, offset=None):
        o = self.offset if offset is None else offset
        vals = None if self.values is None else self.values[o:o + self.length]
        return vals, None if self.bits is None else self.bits[o:o + self.length]

    def null_count(self):
        if self.bits is None:
            return 0
        return int(self.length - self.logical()[1].sum()) if self.known else -1


def _round64(k):
    return (k + 63) // 64 * 64


def pcol(rng, typ, values, valid, offset, known=True, stray_ones=False):
    """the logical column (values, valid) laid out at `offset`: random payloads and random bits in front of and behind the rows
    (stray_ones: every bit outside the rows set)"""
    n = len(valid) if values is None else len(values)
    total = _round64(offset + n + 64)   # (a slice taken at another column's offset still lies inside)
    tail = total - offset - n

    def junk_bits(k):
        return np.ones(k, bool) if stray_ones else rng.integers(0, 2, k).astype(bool)

    if typ == "bool":
        phys = np.concatenate([junk_bits(offset), values, junk_bits(tail)])
    elif typ == "utf8":
        phys = None
    else:
        dt = np.int64 if typ == "int64" else np.float64
        phys = np.concatenate([rng.integers(-1 << 62, 1 << 62, offset).view(dt), values, rng.integers(-1 << 62, 1 << 62, tail).view(dt)])
    bits = None if valid is None else np.concatenate([junk_bits(offset), valid, junk_bits(tail)])
    return PCol(typ, phys, bits, offset, n, known)


# ------------------------------------------------------------------ the models
def _type_of(values):
    return {"i": "int64", "f": "float64", "b": "bool"}[values.dtype.kind]


def _valid(valid, n):
    return np.ones(n, bool) if valid is None else valid


def equal(left, right, mode, flaw=None):
    """left / right: lists of (values, valid).  -> (equal, first_row, first_col) as bowgpu_equal reports them"""
    assert len(left) == len(right)
    if not left:
        return True, -1, -1
    for c, ((lv, _), (rv, _)) in enumerate(zip(left, right)):
        if _type_of(lv) != _type_of(rv):
            return False, -1, c
    n = len(left[0][0])
    if n != len(right[0][0]):
        return False, -1, -1
    if n == 0:
        return True, -1, -1
    differs = np.zeros((len(left), n), bool)
    for c, ((lv, lb), (rv, rb)) in enumerate(zip(left, right)):
        lb, rb = _valid(lb, n), _valid(rb, n)
        if lv.dtype.kind == "f" and mode == EQUAL_GO:
            neq = ~(lv == rv)                       # IEEE ==: a NaN differs from everything, -0.0 equals +0.0
            if flaw == "nan_equal_go":
                neq &= ~(np.isnan(lv) & np.isnan(rv) & (lv.view(np.uint64) == rv.view(np.uint64)))
        elif lv.dtype.kind == "f" and flaw == "negzero_equal_bits":   # (the 64 bits, but the zeros alike)
            neq = (lv.view(np.uint64) != rv.view(np.uint64)) & ~((lv == 0) & (rv == 0))
        elif lv.dtype.kind == "b":
            neq = lv != rv
        else:
            neq = lv.view(np.uint64) != rv.view(np.uint64)
        differs[c] = (lb ^ rb) | (lb & rb & neq)
        if flaw == "null_slots":
            differs[c] |= ~lb & ~rb & neq
    rows = differs.any(axis=0)
    if not rows.any():
        return True, -1, -1
    row = int(np.argmax(rows))
    col = int(np.argmax(differs.any(axis=1))) if flaw == "lowest_col_overall" else int(np.argmax(differs[:, row]))
    return False, row, col


def valid_row(cols, row_start, direction):
    """cols: list of (values, valid).  The nearest row <= row_start (direction -1) or >= row_start (+1) where every column is valid"""
    assert direction in (-1, 1) and cols
    n = len(cols[0][1]) if cols[0][0] is None else len(cols[0][0])
    if row_start < 0 or row_start >= n:
        return -1
    every = np.ones(n, bool)
    for _, valid in cols:
        every &= _valid(valid, n)
    rows = np.flatnonzero(every[row_start:]) + row_start if direction > 0 else np.flatnonzero(every[:row_start + 1])
    if len(rows) == 0:
        return -1
    return int(rows[0] if direction > 0 else rows[-1])


def is_col_empty(col):
    """NullN() == Len()"""
    values, valid = col
    n = len(valid) if values is None else len(values)
    return n == 0 or (valid is not None and not valid.any())


# ------------------------------------------------------------------ the models over columns in memory (and their wrong variants)
def equal_p(left, right, mode, flaw=None):
    """left / right: lists of PCol"""
    for c, (l, r) in enumerate(zip(left, right)):
        if l.typ != r.typ:
            return False, -1, c
    if left and left[0].length != right[0].length:
        return False, -1, -1
    lo = [l.logical() for l in left]
    ro = [r.logical(l.offset if flaw == "right_offset" else None) for l, r in zip(left, right)]
    return equal(lo, ro, mode, flaw)


def valid_row_p(cols, row_start, direction, flaw=None):
    n = cols[0].length
    if row_start < 0 or row_start >= n:
        return -1
    if flaw == "start_word":       # the whole 64-row word of row_start is searched
        row_start = row_start - row_start % 64 if direction > 0 else min(n - 1, row_start | 63)
    if flaw == "past_length":      # rows up to the end of the last 64-row word are searched
        n = _round64(n)
    lo = [(None, np.ones(n, bool) if c.bits is None else c.bits[c.offset:c.offset + n]) for c in cols]
    return valid_row(lo, row_start, direction)


# ------------------------------------------------------------------ the seeded plan
NAN_A = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]
NAN_B = np.array([0xFFF8000000000003], np.uint64).view(np.float64)[0]


def _edge_rows(n):
    rows = {0, n - 1}
    for t in range(T, n + 2, T):
        rows |= {t - 1, t, t + 1}
    return sorted(r for r in rows if 0 <= r < n)


def _values(rng, typ, n):
    if typ == "int64":
        return rng.integers(-1 << 62, 1 << 62, n)
    if typ == "float64":
        return rng.standard_normal(n)
    return rng.integers(0, 2, n).astype(bool)


def _other(typ, v):
    """a value of the type that differs from v under both modes"""
    if typ == "bool":
        return not v
    return v + 1 if typ == "int64" else v + 1.5


def equal_case(seed):
    """-> dict: left / right (lists of PCol), residency (one name per side and column), family, and what was planted"""
    rng = np.random.default_rng(7000 + seed)
    family = FAMILIES[seed % len(FAMILIES)]
    n = LENGTHS[(seed * 7 + seed // 15) % len(LENGTHS)]
    ncols = NCOLS[(seed // 3) % len(NCOLS)]
    if family == "two_groups":
        ncols = max(ncols, 5)
    if family == "same_row_two_cols":
        ncols = max(ncols, 4)
    types = [["int64", "float64", "bool"][(seed + c) % 3] for c in range(ncols)]
    p_null = 0.6 if family == "identical_nulls" else 0.3
    lo_l, lo_r = [], []
    for c, typ in enumerate(types):
        vals = _values(rng, typ, n)
        valid = rng.random(n) >= p_null
        if family == "ones_vs_none" or (c % 4 == 3 and family != "under_null"):
            valid = np.ones(n, bool)
        rvals = vals.copy()
        if typ != "bool":   # other payloads under the nulls of the right side
            rvals[~valid] = _values(rng, typ, n)[~valid]
        else:
            rvals[~valid] ^= True
        lo_l.append([vals, valid.copy()])
        lo_r.append([rvals, valid.copy()])
    rows = _edge_rows(n)
    pick = lambda: int(rows[rng.integers(len(rows))]) if rng.random() < 0.7 else int(rng.integers(n))
    planted = []

    def col_of(typ, start=0):
        for c in range(start, ncols):
            if types[c] == typ:
                return c
        return None

    def plant_value(c, r):
        lo_l[c][1][r] = lo_r[c][1][r] = True
        lo_r[c][0][r] = _other(types[c], lo_l[c][0][r])
        planted.append((r, c))

    def plant_float(c, r, lv, rv):
        lo_l[c][1][r] = lo_r[c][1][r] = True
        lo_l[c][0][r], lo_r[c][0][r] = lv, rv
        planted.append((r, c))

    if family == "value_diff":
        plant_value(int(rng.integers(ncols)), pick())
    elif family == "valid_diff":
        c, r = int(rng.integers(ncols)), pick()
        lo_r[c][1][r] = not lo_l[c][1][r]
        planted.append((r, c))
    elif family == "two_groups":       # the lower row lies in the higher column, in a later launch group
        r_hi = pick()
        if r_hi == 0:
            r_hi = n - 1
        plant_value(0, r_hi)
        if r_hi > 0:
            plant_value(ncols - 1, int(rng.integers(r_hi)))
    elif family == "same_row_two_cols":
        r = pick()
        plant_value(1, r)
        plant_value(3, r)
    elif family == "int_bits":
        c, r = col_of("int64"), pick()
        if c is not None:
            lo_l[c][1][r] = lo_r[c][1][r] = True
            k = (seed // len(FAMILIES)) % 3
            v = [(1 << 53) + 2, 0, 5][k]
            lo_l[c][0][r] = v
            lo_r[c][0][r] = [(1 << 53) + 3, -(1 << 63), 4][k]   # above 2^53; bit 63 alone; bit 0 alone
            planted.append((r, c))
    elif family in ("nan_same", "nan_payload", "negzero"):
        c, r = col_of("float64"), pick()
        if c is not None:
            plant_float(c, r, *{"nan_same": (NAN_A, NAN_A), "nan_payload": (NAN_A, NAN_B), "negzero": (-0.0, 0.0)}[family])
    left, right, res = [], [], []
    for c, typ in enumerate(types):
        no_bitmap_l = lo_l[c][1].all() and (family == "ones_vs_none" or rng.random() < 0.5)
        no_bitmap_r = lo_r[c][1].all() and family != "ones_vs_none" and rng.random() < 0.5
        ol, orr = OFFSETS[int(rng.integers(len(OFFSETS)))], OFFSETS[int(rng.integers(len(OFFSETS)))]
        left.append(pcol(rng, typ, lo_l[c][0], None if no_bitmap_l else lo_l[c][1], ol, known=bool(rng.integers(2)), stray_ones=bool(rng.integers(2))))
        right.append(pcol(rng, typ, lo_r[c][0], None if no_bitmap_r else lo_r[c][1], orr, known=bool(rng.integers(2)), stray_ones=bool(rng.integers(2))))
        res.append((RESIDENCIES[int(rng.integers(3))], RESIDENCIES[int(rng.integers(3))]))
    return {"seed": seed, "family": family, "n": n, "left": left, "right": right, "residency": res, "planted": planted}


def valid_row_case(seed):
    """-> dict: cols (PCol: any type, bitmaps are all that is read), row_start, direction, residency, family"""
    rng = np.random.default_rng(9000 + seed)
    family = VR_FAMILIES[seed % len(VR_FAMILIES)]
    direction = 1 if (seed // len(VR_FAMILIES)) % 2 == 0 else -1
    n = LENGTHS[(seed * 4 + seed // 15 + 3) % len(LENGTHS)]
    ncols = [1, 2, 8, 3][(seed // 2) % 4]
    start = int(rng.integers(n))
    if family == "other_tile" and n > T:
        start = int(rng.integers(n - T)) if direction > 0 else int(rng.integers(T, n))
    if family == "row0":
        direction, start = -1, int(rng.integers(n))
    if family == "last_row":
        direction, start = 1, int(rng.integers(n))
    # rows where every column is valid: the answer, and one on the wrong side of row_start inside its word
    ahead = np.arange(start, n) if direction > 0 else np.arange(start, -1, -1)
    word = ahead[(ahead // 64) == start // 64]
    target = {"at_start": start, "same_word": int(word[-1]), "next_word": int(ahead[min(len(ahead) - 1, len(word))]),
              "other_tile": int(ahead[min(len(ahead) - 1, T + 5)]), "none": None, "interleave": int(ahead[len(ahead) // 2]),
              "row0": 0, "last_row": n - 1}[family]
    every = np.zeros(n, bool)
    if target is not None:
        every[target] = True
        beyond = ahead[np.flatnonzero(ahead == target)[0] + 1:]      # more common rows further away
        every[beyond[rng.random(len(beyond)) < 0.2]] = True
    behind = np.arange(0, start) if direction > 0 else np.arange(start + 1, n)
    every[behind[rng.random(len(behind)) < 0.5]] = True
    if len(behind):
        every[behind[-1] if direction > 0 else behind[0]] = True      # right next to row_start, on the wrong side
    cols, res = [], []
    for c in range(ncols):
        valid = every.copy()
        if ncols > 1:   # rows that are valid in this column and not in its neighbour: they interleave, no common row is added
            some = (rng.random(n) < 0.4) & ~every & ((np.arange(n) + c) % 2 == 0)
            valid |= some
        typ = ["float64", "utf8", "bool", "int64"][(seed + c) % 4]
        no_bitmap = typ != "utf8" and valid.all() and rng.random() < 0.5
        cols.append(pcol(rng, typ, None if typ == "utf8" else _values(rng, typ, n), None if no_bitmap else valid,
                         OFFSETS[int(rng.integers(len(OFFSETS)))], known=bool(rng.integers(2)), stray_ones=True))
        res.append(RESIDENCIES[int(rng.integers(3))])
    return {"seed": seed, "family": family, "n": n, "cols": cols, "row_start": start, "direction": direction, "residency": res}
