"""A numpy / dict model of the join on several common columns (reference getCommonCols bowjoin.go:128-155, getCommonRows :161-186, the
per-column fills :383-400), exact and independent of the library.  A row's key is the tuple of (None for nil, else the value) over the
key columns; Python's == and hash on such tuples are Go's == per column (-0.0 and +0.0 are one float key, nil == nil, a value under a
null is never looked at).  A dict from key tuple to ascending right rows gives the pair list in O(L + R + pairs).

A column is anything with .values (int64 / float64 array), .valid (bool array or None), .typ and .bits() - test_gpu_filter.Col is one.
tests/test_join_keys_cpu.py proves the model against a literal nested-loop restatement of the reference and against both fixtures."""
import numpy as np

from bow_amd import capi

INNER, OUTER = capi.JOIN_INNER, capi.JOIN_OUTER


class ModelCol:
    """the least a column of the model is (test_gpu_filter.Col adds the Arrow offset and the ctypes view)"""

    def __init__(self, values, valid=None):
        self.values, self.valid = np.ascontiguousarray(values), valid
        self.typ = capi.INT64 if self.values.dtype == np.int64 else capi.FLOAT64

    def bits(self):
        return self.values.view(np.uint64)


def case_frame(cols, make=ModelCol):
    """a fixture frame (column-based lists, None for nil) as model columns; 0 under a null"""
    out = []
    for c in cols:
        data = c["data"]
        valid = np.array([x is not None for x in data], bool)
        vals = np.array([0 if x is None else x for x in data], np.int64 if c["type"] == "int64" else np.float64)
        out.append(make(vals, None if valid.all() else valid))
    return out


def valid_of(col):
    return np.ones(len(col.values), bool) if col.valid is None else np.asarray(col.valid, bool)


def key_tuples(keys):
    """the rows of the key columns as hashable tuples; no key column: every row the empty tuple (never used - no keys is no pair list)"""
    n = len(keys[0].values) if keys else 0
    per_col = [[x if ok else None for x, ok in zip(k.values.tolist(), valid_of(k).tolist())] for k in keys]
    return list(zip(*per_col)) if per_col else [()] * n


def pair_rows(lkeys, rkeys, kind):
    """(l_idx, r_idx, pairs): getCommonRows ordered by l then r, then the fill order of the kind.  lkeys / rkeys: lists of key columns"""
    where = {}
    rt = key_tuples(rkeys)
    for r, t in enumerate(rt):
        where.setdefault(t, []).append(r)
    li, ri, pairs, hit = [], [], 0, np.zeros(len(rt), bool)
    for l, t in enumerate(key_tuples(lkeys)):
        rows = where.get(t, ())
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
    """no pair list (no common column): InnerJoin has no rows, OuterJoin all left rows then all right rows"""
    if kind == INNER:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    return np.concatenate([np.arange(nl), np.full(nr, -1)]).astype(np.int64), np.concatenate([np.full(nl, -1), np.arange(nr)]).astype(np.int64), 0


def join_rows(left, lks, right, rks, kind):
    """the rows of the join of two frames on the key pairs (lks[k], rks[k])"""
    if not lks:
        return identity_rows(len(left[0].values) if left else 0, len(right[0].values) if right else 0, kind)
    return pair_rows([left[k] for k in lks], [right[k] for k in rks], kind)


def take(col, idx):
    """(bits, valid) of col at idx, -1: null; null slots hold 0"""
    ok = idx >= 0
    if len(col.values) == 0:
        return np.zeros(len(idx), np.uint64), np.zeros(len(idx), bool)
    safe = np.where(ok, idx, 0)
    valid = ok & valid_of(col)[safe]
    return np.where(valid, col.bits()[safe], np.uint64(0)), valid


def expected_columns(left, lks, right, rks, li, ri):
    """[(type, bits, valid)]: every left column, then every right column that is no right key.  EACH key column holds the left row's
    value and, on a right-only row, the value and validity of ITS OWN right key column"""
    want = []
    for i, c in enumerate(left):
        bits, valid = take(c, li)
        if i in lks:
            b2, v2 = take(right[rks[list(lks).index(i)]], ri)
            bits, valid = np.where(li >= 0, bits, b2), np.where(li >= 0, valid, v2)
        want.append((c.typ, bits, valid))
    for i, c in enumerate(right):
        if i not in rks:
            want.append((c.typ,) + take(c, ri))
    return want


def to_lists(want):
    """expected_columns as the fixture writes frames: one list per column, None for nil"""
    out = []
    for typ, bits, valid in want:
        vals = bits.view(np.int64 if typ == capi.INT64 else np.float64).tolist()
        out.append([v if ok else None for v, ok in zip(vals, valid.tolist())])
    return out
