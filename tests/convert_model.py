"""A numpy model of Bow.Convert among Int64, Float64 and Boolean (reference bowsetters.go:52-56, bowtypes.go:64-81, bowconvert.go) and
what the tests of bowgpu_convert share: the special values, the columns a case is made of, the expected output of a column and its
exact comparison, and the seeded fuzz cases.

The oracle has no Convert, so this model stands in.  Every rule is written out - nothing rests on what numpy's astype gives outside a
type's range - and tests/test_convert_model_cpu.py proves it without a GPU: against Python's own arithmetic, by coverage of the seeded
cases, and by deliberately wrong variants (VARIANTS) that the seeded cases must tell from the model.

The rules, per valid row (a null row stays null and its slot holds 0 / a clear bit; a valid row stays valid):
  Int64 -> Float64    Go's float64(v): round to nearest, ties to even       Int64 -> Boolean     v != 0
  Float64 -> Int64    Go's int64(v) on amd64: truncation toward zero where -2^63 <= v < 2^63, else 0x8000000000000000
  Float64 -> Boolean  v != 0.0 (NaN is true, -0.0 is false)                 Boolean -> Int64 / Float64   1 / 0, 1.0 / 0.0
  same type           the same bits (NaN payloads included)"""
import math
import struct

import numpy as np

from bow_amd import capi

F, I, B = capi.FLOAT64, capi.INT64, capi.BOOLEAN
TYPES = (I, F, B)
PAIRS = [(a, b) for a in TYPES for b in TYPES]
NAMES = {I: "int64", F: "float64", B: "bool"}
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
OFFSETS = (0, 1, 7, 8, 13, 69)
VARIANTS = ("saturate", "rtz", "nan_false", "negzero_true", "leak", "padding")


def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


QNAN, NEG_NAN, SNAN = 0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000ABCDEF   # quiet, negative, signalling with a payload
FLOAT_SPECIALS_BITS = [struct.unpack("<Q", struct.pack("<d", x))[0] for x in (
    0.0, -0.0, 0.5, -0.5, 0.9999999999999999, -0.9999999999999999, -1.9, 5e-324, 2.0 ** 52 + 0.5, 2.0 ** 53,
    math.nextafter(2.0 ** 63, 0.0), 2.0 ** 63, -2.0 ** 63, math.nextafter(-2.0 ** 63, -math.inf), 1e19, math.inf, -math.inf)] + [QNAN, NEG_NAN, SNAN]
INT_SPECIALS = [0, 1, -1, 2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 3), 2 ** 54 + 2, 2 ** 54 + 6, INT64_MAX, INT64_MIN]


def float_specials():
    return np.array(FLOAT_SPECIALS_BITS, np.uint64).view(np.float64)


def int_specials():
    return np.array(INT_SPECIALS, np.int64)


def specials(typ):
    return {I: int_specials(), F: float_specials(), B: np.array([False, True])}[typ]


# ---------------------------------------------------------------- the value rules
def int_to_float(v, variant=None):
    """float64(v), nearest-even: the high and the low half are exact as doubles and so is hi * 2^32; the one addition rounds"""
    v = np.asarray(v, np.int64)
    if variant == "rtz":   # (wrong on purpose) the magnitude cut to 53 bits
        neg = v < 0
        u = v.view(np.uint64)
        mag = np.where(neg, ~u + np.uint64(1), u)                # (2^63 for INT64_MIN)
        shift = np.zeros(v.shape, np.uint64)
        for k in range(11):
            shift += (mag >= np.uint64(2 ** (53 + k))).astype(np.uint64)
        cut = (mag >> shift) << shift                            # at most 53 significant bits: exact as a double
        r = (cut >> np.uint64(32)).astype(np.float64) * 4294967296.0 + (cut & np.uint64(0xFFFFFFFF)).astype(np.float64)
        return np.where(neg, -r, r)
    hi = (v >> np.int64(32)).astype(np.float64)                  # |hi| <= 2^31: exact
    lo = (v & np.int64(0xFFFFFFFF)).astype(np.float64)           # < 2^32: exact
    return hi * 4294967296.0 + lo


def float_to_int(v, variant=None):
    """int64(v) as gc/amd64 gives it (CVTTSD2SQ)"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (v >= -9223372036854775808.0) & (v < 9223372036854775808.0)   # a NaN is outside
    t = np.trunc(np.where(inside, v, 0.0))                       # an integer below 2^63 in magnitude, or -2^63: the cast is exact
    out = t.astype(np.int64)
    if variant == "saturate":   # (wrong on purpose)
        with np.errstate(invalid="ignore"):
            return np.where(inside, out, np.where(v != v, 0, np.where(v > 0, INT64_MAX, INT64_MIN))).astype(np.int64)
    return np.where(inside, out, np.int64(INT64_MIN))


def float_to_bool(v, variant=None):
    v = np.asarray(v, np.float64)
    bits = v.view(np.uint64)
    out = (bits & np.uint64(0x7FFFFFFFFFFFFFFF)) != 0            # != 0.0: everything but the two zeros, NaN included
    if variant == "nan_false":
        out = out & ~(v != v)
    if variant == "negzero_true":
        out = out | (bits == np.uint64(0x8000000000000000))
    return out


def convert_slots(slots, from_t, to_t, variant=None):
    """every slot of a column converted, as if valid: int64 / float64 / bool array in, int64 / float64 / bool array out"""
    if from_t == to_t:
        return slots.copy()
    if from_t == I:
        return int_to_float(slots, variant) if to_t == F else slots != 0
    if from_t == F:
        return float_to_int(slots, variant) if to_t == I else float_to_bool(slots, variant)
    return slots.astype(np.int64) if to_t == I else np.where(slots, 1.0, 0.0)


class Expected:
    """the output column of one conversion: values (uint64 slots, or packed bytes for a Boolean target), validity bytes, null count"""

    def __init__(self, slots, valid, from_t, to_t, variant=None):
        n = len(slots)
        valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        conv = convert_slots(slots, from_t, to_t, variant)
        if variant != "leak":
            conv = np.where(valid, conv, np.zeros(1, conv.dtype))   # SetOrDropStrict of nil: the slot NewBuffer zeroed
        self.type, self.length, self.null_count = to_t, n, int(n - valid.sum())
        self.valid = valid
        self.validity = self._pack(valid, variant)
        self.values = self._pack(conv, variant) if to_t == B else np.ascontiguousarray(conv).view(np.uint64)

    @staticmethod
    def _pack(bits, variant):
        out = np.packbits(bits, bitorder="little") if len(bits) else np.zeros(0, np.uint8)
        if variant == "padding" and len(bits) % 8:
            out[-1] |= np.uint8((0xFF << (len(bits) % 8)) & 0xFF)
        return out

    def same_as(self, other):
        return np.array_equal(self.values, other.values) and np.array_equal(self.validity, other.validity)


# ---------------------------------------------------------------- columns
GARBAGE = {I: np.int64(0x0123456789ABCDEF), F: np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0], B: True}


def null_fill(typ, kind):
    """what a null slot of an input holds: 'nan' (NaN for Float64, -1 for Int64, a set bit), 'one' (1 / 1.0 / a set bit), 'zero'"""
    if kind == "zero":
        return {I: np.int64(0), F: 0.0, B: False}[typ]
    if kind == "one":
        return {I: np.int64(1), F: 1.0, B: True}[typ]
    return {I: np.int64(-1), F: _f(NEG_NAN), B: True}[typ]


def pack_bits(bits, offset, fill=True, tail=5):
    """bools -> Arrow LSB-first bytes with `offset` leading and `tail` trailing bits of `fill`"""
    b = np.concatenate([np.full(offset, fill, bool), np.asarray(bits, bool), np.full(tail, fill, bool)])
    return np.packbits(b, bitorder="little")


def make_column(typ, slots, valid, offset=0, null_count=-1):
    """the host Column of the logical rows `slots` (null slots as they are) at Arrow offset `offset`; the rows and bits around the
    column's own hold garbage / are set, so that a kernel reading them shows up.  valid None: no validity buffer"""
    n = len(slots)
    if typ == B:
        values = pack_bits(slots, offset)
    else:
        values = np.concatenate([np.full(offset, GARBAGE[typ]), np.asarray(slots), np.full(3, GARBAGE[typ])]).astype(np.int64 if typ == I else np.float64)
    bm = None if valid is None else pack_bits(valid, offset)
    if valid is not None and null_count >= 0:
        null_count = int(n - np.asarray(valid).sum())
    return capi.Column(values, bm, typ, offset, n, 0 if bm is None else null_count)


def place(col, residency):
    """the column in pageable, registered or device memory (a registered column: unpin() it when done)"""
    if residency == capi.DEVICE:
        return col.to_device()
    if residency == capi.HOST_PINNED:
        vals = capi.page_aligned(len(col.values), col.values.dtype)
        vals[:] = col.values
        bm = None
        if col.validity is not None:
            bm = capi.page_aligned(len(col.validity), np.uint8)
            bm[:] = col.validity
        return capi.Column(vals, bm, col.type, col.offset, col.length, col.null_count).pin()
    return col


def compare(name, got, want):
    """got: capi.OutColumn, want: Expected - type, length, null count and every byte of both buffers (zeroed null slots and clear
    padding bits are part of `want`)"""
    assert got.type == want.type, (name, "type", got.type, want.type)
    assert got.length == want.length, (name, "length", got.length, want.length)
    assert got.null_count == want.null_count, (name, "null_count", got.null_count, want.null_count)
    gv, gb = got.host_arrays()
    gv = np.asarray(gv).view(np.uint8 if want.type == B else np.uint64)
    bad = np.flatnonzero(gv != want.values)
    assert bad.size == 0, (name, "values", bad[:8], gv[bad[:4]], want.values[bad[:4]])
    bad = np.flatnonzero(np.asarray(gb) != want.validity)
    assert bad.size == 0, (name, "validity", bad[:8], np.asarray(gb)[bad[:4]], want.validity[bad[:4]])


# ---------------------------------------------------------------- seeded cases
def random_slots(rng, typ, n):
    if typ == B:
        return rng.random(n) < 0.5
    if typ == I:
        kind = rng.integers(0, 3)
        if kind == 0:
            return rng.integers(-3, 4, n).astype(np.int64)
        if kind == 1:
            return rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
        return (rng.integers(-2 ** 10, 2 ** 10, n) + (np.int64(1) << rng.integers(50, 63, n))).astype(np.int64)   # around the 53-bit edge
    kind = rng.integers(0, 3)
    if kind == 0:
        return np.round(rng.standard_normal(n) * 3.0, 1)
    if kind == 1:
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64, endpoint=False).view(np.float64)   # every bit pattern
    return rng.standard_normal(n) * np.exp2(rng.integers(40, 70, n).astype(np.float64))             # around 2^63


class CaseColumn:
    """one column of a case: logical slots, validity (None: no buffer), how it is handed over, and the pair"""

    def __init__(self, from_t, to_t, slots, valid, offset, null_count, residency, null_rows_special=()):
        self.from_t, self.to_t, self.slots, self.valid = from_t, to_t, slots, valid
        self.offset, self.null_count, self.residency = offset, null_count, residency
        self.null_rows_special = null_rows_special   # rows where a special value sits in a null slot (coverage)

    def column(self):
        return make_column(self.from_t, self.slots, self.valid, self.offset, self.null_count)

    def expected(self, variant=None):
        return Expected(self.slots, self.valid, self.from_t, self.to_t, variant)


def salt(rng, typ, slots, valid):
    """every special value of the type into a row kept valid and - where the column has nulls - into a null slot"""
    sp = specials(typ)
    n = len(slots)
    null_rows = []
    if n < 2 * len(sp):
        if n:
            rows = rng.choice(n, min(n, len(sp)), replace=False)
            slots[rows] = rng.permutation(sp)[:len(rows)]
        return null_rows
    rows = rng.choice(n, 2 * len(sp), replace=False)
    slots[rows[:len(sp)]] = sp
    slots[rows[len(sp):]] = sp
    if valid is not None:
        valid[rows[:len(sp)]] = True
        valid[rows[len(sp):]] = False
        null_rows = list(rows[len(sp):])
    return null_rows


def fuzz_case(seed):
    """the columns of one bowgpu_convert call (list[CaseColumn]) and the residency of its outputs"""
    rng = np.random.default_rng(1_000_003 * seed + 17)
    ncols = int(rng.choice([1, 2, 3, 4, 5, 9]))
    cols = []
    for k in range(ncols):
        from_t, to_t = PAIRS[(seed * 5 + k * 2 + int(rng.integers(0, 2))) % 9]
        n = int(rng.choice([0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, int(rng.integers(2, 3000)), int(rng.integers(3000, 70002))]))
        offset = int(rng.choice(OFFSETS)) if rng.random() < 0.8 else int(rng.integers(0, 300))
        slots = random_slots(rng, from_t, n)
        nulls = rng.choice(["none", "all", "some", "some", "some"])
        valid = None
        if nulls == "all":
            valid = np.zeros(n, bool)
        elif nulls == "some":
            valid = rng.random(n) >= (0.3 if rng.random() < 0.7 else rng.choice([0.01, 0.9]))
        null_rows = [] if nulls == "all" else salt(rng, from_t, slots, valid)
        if valid is not None:
            fill = rng.choice(["nan", "one", "keep"])
            if fill != "keep":
                keep = np.zeros(n, bool)
                keep[null_rows] = True
                slots[~valid & ~keep] = null_fill(from_t, fill)
        cols.append(CaseColumn(from_t, to_t, slots, valid, offset, int(rng.choice([-1, 1])), int(rng.choice([capi.HOST, capi.HOST_PINNED, capi.DEVICE])),
                               null_rows))
    return cols, int(rng.choice([capi.HOST, capi.DEVICE, capi.HOST_PINNED]))
