"""The numpy models of tests/equal_model.py, proven without a GPU: against plain Python row loops written from the reference's lines
(Bow.Equal bow.go:227-275 over GetRow's boxed values; the getters bowgetters.go:65-151, statement by statement), a census of the seeded
plan the GPU fuzz draws from, and deliberately wrong model variants that the plan's cases must tell apart from the right one."""
import struct

import numpy as np
import pytest

import equal_model as M

NAN_A, NAN_B = float(M.NAN_A), float(M.NAN_B)
SEEDS = range(64)   # BOW_FUZZ_SEEDS' default in tests/test_gpu_equal.py


# ------------------------------------------------------------------ brute force: the reference's loops
def box(col, r):
    """GetValue (bowgetters.go:46-63): nil for a null row, else the boxed value"""
    values, valid = col
    if valid is not None and not valid[r]:
        return None
    v = values[r]
    return bool(v) if values.dtype.kind == "b" else int(v) if values.dtype.kind == "i" else float(v)


def deep_equal(a, b, mode):
    """reflect.DeepEqual on two boxed values of the same column type (Python's float == is IEEE, as Go's); EQUAL_BITS: the 64 bits"""
    if a is None or b is None:
        return a is None and b is None
    if mode == M.EQUAL_BITS and isinstance(a, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    return a == b


def brute_equal(left, right, mode):
    for c, (l, r) in enumerate(zip(left, right)):
        if l[0].dtype.kind != r[0].dtype.kind:      # Schema().Equal
            return False, -1, c
    if not left:
        return True, -1, -1
    if len(left[0][0]) != len(right[0][0]):          # ok1 != ok2: one channel runs dry first
        return False, -1, -1
    for r in range(len(left[0][0])):                 # GetRowsChan, row by row
        for c in range(len(left)):
            if not deep_equal(box(left[c], r), box(right[c], r), mode):
                return False, r, c
    return True, -1, -1


class GoBow:
    """just enough of the reference's bow for the getters' loops"""

    def __init__(self, cols):
        self.cols = cols

    def NumRows(self):
        return len(self.cols[0][0])

    def GetValue(self, c, r):
        return box(self.cols[c], r)

    def GetPrevValue(self, colIndex, rowIndex):      # bowgetters.go:67-77
        while rowIndex >= 0 and rowIndex < self.NumRows():
            value = self.GetValue(colIndex, rowIndex)
            if value is not None:
                return value, rowIndex
            rowIndex -= 1
        return None, -1

    def GetNextValue(self, colIndex, rowIndex):      # bowgetters.go:81-91
        while rowIndex >= 0 and rowIndex < self.NumRows():
            value = self.GetValue(colIndex, rowIndex)
            if value is not None:
                return value, rowIndex
            rowIndex += 1
        return None, -1

    def GetPrevValues(self, colIndex1, colIndex2, rowIndex):   # bowgetters.go:95-107
        while rowIndex >= 0 and rowIndex < self.NumRows():
            v1, rowIndex = self.GetPrevValue(colIndex1, rowIndex)
            v2, rowIndex2 = self.GetPrevValue(colIndex2, rowIndex)
            if rowIndex == rowIndex2:
                return v1, v2, rowIndex
            rowIndex -= 1
        return None, None, -1

    def GetNextValues(self, colIndex1, colIndex2, rowIndex):   # bowgetters.go:111-123
        while rowIndex >= 0 and rowIndex < self.NumRows():
            v1, rowIndex = self.GetNextValue(colIndex1, rowIndex)
            v2, rowIndex2 = self.GetNextValue(colIndex2, rowIndex)
            if rowIndex == rowIndex2:
                return v1, v2, rowIndex
            rowIndex += 1
        return None, None, -1

    def GetPrevRowIndex(self, colIndex, rowIndex):   # bowgetters.go:127-137
        while rowIndex >= 0 and rowIndex < self.NumRows():
            if self.cols[colIndex][1] is None or self.cols[colIndex][1][rowIndex]:
                return rowIndex
            rowIndex -= 1
        return -1

    def GetNextRowIndex(self, colIndex, rowIndex):   # bowgetters.go:141-151
        while rowIndex >= 0 and rowIndex < self.NumRows():
            if self.cols[colIndex][1] is None or self.cols[colIndex][1][rowIndex]:
                return rowIndex
            rowIndex += 1
        return -1


def random_frame(rng, n, ncols):
    cols = []
    for c in range(ncols):
        kind = rng.integers(3)
        if kind == 0:
            vals = rng.integers(-1, 2, n)
        elif kind == 1:
            vals = rng.choice(np.array([0.0, -0.0, 1.0, NAN_A, NAN_B, np.inf]), n)
        else:
            vals = rng.integers(0, 2, n).astype(bool)
        p = [0.0, 0.1, 0.5, 0.95][rng.integers(4)]
        cols.append((vals, None if rng.random() < 0.2 else rng.random(n) >= p))
    return cols


def mutate(rng, frame):
    out = []
    for vals, valid in frame:
        vals, valid = vals.copy(), None if valid is None else valid.copy()
        n = len(vals)
        for _ in range(int(rng.integers(0, 3)) if n else 0):
            r = int(rng.integers(n))
            what = rng.integers(3)
            if what == 0 and valid is not None:
                valid[r] = not valid[r]
            elif what == 1:
                vals[r] = {"i": 7, "f": [NAN_A, NAN_B, -0.0, 0.0, 2.5][rng.integers(5)], "b": not vals[r]}[vals.dtype.kind]
            elif valid is None:
                valid = np.ones(n, bool)   # a bitmap of all ones against none
        out.append((vals, valid))
    return out


@pytest.mark.parametrize("block", range(6))
def test_equal_model_against_the_row_loop(block):
    rng = np.random.default_rng(100 + block)
    seen = set()
    for _ in range(60):
        n = int(rng.integers(0, 301))
        left = random_frame(rng, n, int(rng.integers(1, 6)))
        right = mutate(rng, left) if rng.random() < 0.8 else left
        if rng.random() < 0.05 and n:
            right = [(v[:-1], None if b is None else b[:-1]) for v, b in right]
        if rng.random() < 0.05:
            right = [(right[0][0].astype(np.float64) if right[0][0].dtype.kind != "f" else np.zeros(len(right[0][0]), np.int64), right[0][1])] + right[1:]
        for mode in (M.EQUAL_GO, M.EQUAL_BITS):
            want = brute_equal(left, right, mode)
            assert M.equal(left, right, mode) == want
            seen.add(want[0])
    assert seen == {True, False}
    assert M.equal([], [], M.EQUAL_GO) == (True, -1, -1)


def test_equal_of_a_frame_with_itself():
    """Equal(b, b) is false for a frame with a valid NaN, as in the reference; a NaN under a null does not count"""
    vals = np.array([1.0, NAN_A, 2.0])
    for valid, go in ((None, False), (np.array([1, 1, 1], bool), False), (np.array([1, 0, 1], bool), True)):
        b = [(vals, valid)]
        assert brute_equal(b, b, M.EQUAL_GO)[0] == go and M.equal(b, b, M.EQUAL_GO)[0] == go
        assert brute_equal(b, b, M.EQUAL_BITS)[0] and M.equal(b, b, M.EQUAL_BITS)[0]


@pytest.mark.parametrize("block", range(6))
def test_getter_models_against_the_go_loops(block):
    rng = np.random.default_rng(200 + block)
    for _ in range(50):
        n = int(rng.integers(1, 301))
        cols = random_frame(rng, n, 3)
        b = GoBow(cols)
        for start in list(rng.integers(-2, n + 2, 12)) + [0, n - 1, -1, n]:
            start = int(start)
            for c in range(3):
                assert M.valid_row([cols[c]], start, -1) == b.GetPrevRowIndex(c, start) == b.GetPrevValue(c, start)[1]
                assert M.valid_row([cols[c]], start, +1) == b.GetNextRowIndex(c, start) == b.GetNextValue(c, start)[1]
            for c1, c2 in ((0, 1), (1, 2), (2, 0), (1, 1)):
                v1, v2, row = b.GetPrevValues(c1, c2, start)
                assert M.valid_row([cols[c1], cols[c2]], start, -1) == row
                assert (v1, v2) == ((None, None) if row < 0 else (b.GetValue(c1, row), b.GetValue(c2, row))) or row >= 0 and (v1 != v1 or v2 != v2)
                assert M.valid_row([cols[c1], cols[c2]], start, +1) == b.GetNextValues(c1, c2, start)[2]
        for c in range(3):
            valid = cols[c][1]
            assert M.is_col_empty(cols[c]) == (n - (n if valid is None else int(valid.sum())) == n)   # NullN() == Len()
    assert M.is_col_empty((np.zeros(0), None)) and M.is_col_empty((np.zeros(0), np.zeros(0, bool)))


# ------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def plan():
    return [M.equal_case(s) for s in SEEDS], [M.valid_row_case(s) for s in SEEDS]


def test_census_of_the_plan(plan):
    eq_cases, vr_cases = plan
    verdicts = [M.equal_p(c["left"], c["right"], mode)[0] for c in eq_cases for mode in (M.EQUAL_GO, M.EQUAL_BITS)]
    assert sum(verdicts) * 3 >= len(verdicts) and (len(verdicts) - sum(verdicts)) * 3 >= len(verdicts)
    assert {c["family"] for c in eq_cases} == set(M.FAMILIES)
    assert {c["family"] for c in vr_cases} == set(M.VR_FAMILIES)
    for cases, cols_of in ((eq_cases, lambda c: c["left"] + c["right"]), (vr_cases, lambda c: c["cols"])):
        assert {c["n"] for c in cases} == set(M.LENGTHS)
        assert {p.offset for c in cases for p in cols_of(c)} == set(M.OFFSETS)
    assert {len(c["left"]) for c in eq_cases} == set(M.NCOLS)
    assert {len(c["cols"]) for c in vr_cases} >= {1, 2, 8}
    assert {r for c in eq_cases for pair in c["residency"] for r in pair} == set(M.RESIDENCIES)
    assert any(l != r for c in eq_cases for l, r in c["residency"])            # mixed between the sides
    assert {r for c in vr_cases for r in c["residency"]} == set(M.RESIDENCIES)
    assert {p.typ for c in eq_cases for p in c["left"]} == {"int64", "float64", "bool"}
    assert {p.typ for c in vr_cases for p in c["cols"]} == {"int64", "float64", "bool", "utf8"}
    assert {c["direction"] for c in vr_cases} == {-1, 1}
    answers = [M.valid_row_p(c["cols"], c["row_start"], c["direction"]) for c in vr_cases]
    assert -1 in answers and any(a == c["row_start"] for a, c in zip(answers, vr_cases))
    assert any(a >= 0 and a // M.T != c["row_start"] // M.T for a, c in zip(answers, vr_cases))   # the answer in another tile
    # the lower row in the higher column, in a later launch group
    assert any(c["family"] == "two_groups" and len(c["planted"]) == 2 and c["planted"][1][0] < c["planted"][0][0] and c["planted"][1][1] >= 4
               for c in eq_cases)


@pytest.mark.parametrize("flaw", M.EQUAL_FLAWS)
def test_plan_tells_a_wrong_equal_model_apart(plan, flaw):
    told = [c["seed"] for c in plan[0] for mode in (M.EQUAL_GO, M.EQUAL_BITS)
            if M.equal_p(c["left"], c["right"], mode, flaw) != M.equal_p(c["left"], c["right"], mode)]
    assert told, flaw


@pytest.mark.parametrize("flaw", M.VALID_ROW_FLAWS)
def test_plan_tells_a_wrong_valid_row_model_apart(plan, flaw):
    told = [c["seed"] for c in plan[1]
            if M.valid_row_p(c["cols"], c["row_start"], c["direction"], flaw) != M.valid_row_p(c["cols"], c["row_start"], c["direction"])]
    assert told, flaw
    assert {plan[1][s % len(SEEDS)]["direction"] for s in told} == {-1, 1} or flaw == "past_length"
