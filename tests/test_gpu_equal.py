"""bowgpu_equal / bowgpu_valid_row / bowgpu_is_col_empty on the device against the numpy models of tests/equal_model.py (proven
without a GPU by tests/test_equal_model_cpu.py).  Every comparison is exact: equal, first_row, first_col; the row; the flag."""
import os
import subprocess

import numpy as np
import pytest

import equal_model as M
from bow_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = M.T
TYPES = {"int64": capi.INT64, "float64": capi.FLOAT64, "bool": capi.BOOLEAN, "utf8": capi.STRING}
RES = {"host": capi.HOST, "device": capi.DEVICE, "pinned": capi.HOST_PINNED}
MODES = (capi.EQUAL_GO, capi.EQUAL_BITS)


# ------------------------------------------------------------------ columns in memory -> the C ABI
def pack(bits):
    return np.packbits(bits, bitorder="little")


def column(p, residency="host"):
    """a PCol as a capi.Column of the residency: every buffer is live and at least as large as offset + length says"""
    validity = None if p.bits is None else pack(p.bits)
    if p.typ == "bool":
        values = pack(p.values)
    elif p.typ == "utf8":
        values = np.zeros(8, np.uint8)   # (never read: only the bitmap of a String-typed column is)
    else:
        values = p.values
    c = capi.Column(values, validity, TYPES[p.typ], p.offset, p.length, p.null_count())
    if residency == "device":
        return c.to_device()
    if residency == "pinned":
        pc = capi.Column(capi.page_aligned(len(c.values), c.values.dtype), None if validity is None else capi.page_aligned(len(validity), np.uint8),
                         c.type, c.offset, c.length, c.null_count)
        pc.values[:] = c.values
        if validity is not None:
            pc.validity[:] = validity
        return pc.pin()
    return c


def release(cols):
    for c in cols:
        if c.residency == capi.HOST_PINNED:
            c.unpin()


def check_equal(left, right, res=None, modes=MODES):
    """left / right: lists of PCol; res: one (left, right) pair of residency names per column, or one name for all.  -> the model's answers"""
    if res is None or isinstance(res, str):
        res = [(res or "host", res or "host")] * len(left)
    lc = [column(p, r[0]) for p, r in zip(left, res)]
    rc = [column(p, r[1]) for p, r in zip(right, res)]
    try:
        wants = []
        for mode in modes:
            want = M.equal_p(left, right, mode)
            got = capi.equal(lc, rc, mode)
            assert got == want, (mode, got, want)
            wants.append(want)
        return wants
    finally:
        release(lc + rc)


def check_valid_row(cols, start, direction, res=None):
    if res is None or isinstance(res, str):
        res = [res or "host"] * len(cols)
    cc = [column(p, r) for p, r in zip(cols, res)]
    try:
        want = M.valid_row_p(cols, start, direction)
        got = capi.valid_row(cc, start, direction)
        assert got == want, (start, direction, got, want)
        return want
    finally:
        release(cc)


def frame(rng, n, ncols, p_null=0.3, first_type=0):
    """logical columns, mixed Int64 / Float64 / Boolean: [values, valid] lists"""
    out = []
    for c in range(ncols):
        typ = ["int64", "float64", "bool"][(first_type + c) % 3]
        out.append([typ, M._values(rng, typ, n), rng.random(n) >= p_null])
    return out


def lay(rng, cols, offsets=None, bitmaps=True, **kw):
    """the logical columns as PCols; offsets: one per column (default: drawn from OFFSETS)"""
    out = []
    for c, (typ, vals, valid) in enumerate(cols):
        off = M.OFFSETS[int(rng.integers(len(M.OFFSETS)))] if offsets is None else offsets[c]
        out.append(M.pcol(rng, typ, vals.copy(), valid.copy() if bitmaps else None, off, **kw))
    return out


def copy_of(cols):
    return [[typ, vals.copy(), valid.copy()] for typ, vals, valid in cols]


def res_cycle(k, ncols):
    names = M.RESIDENCIES
    return [(names[(k + c) % 3], names[(k + 2 * c + 1) % 3]) for c in range(ncols)]


# ------------------------------------------------------------------ Equal
@pytest.mark.parametrize("n", M.LENGTHS)
def test_identical_frames(n):
    rng = np.random.default_rng(n)
    cols = frame(rng, n, 3, first_type=n)
    wants = check_equal(lay(rng, cols), lay(rng, cols, known=False), res_cycle(n, 3))
    assert wants == [(True, -1, -1)] * 2


@pytest.mark.parametrize("what", ["value", "validity"])
@pytest.mark.parametrize("n", M.LENGTHS)
def test_one_difference_at_the_edges(n, what):
    """row 0, row n - 1 and each tile edge +- 1"""
    rng = np.random.default_rng(n + 1)
    cols = frame(rng, n, 3, first_type=n + 1)
    left = lay(rng, cols)
    for k, row in enumerate(M._edge_rows(n)):
        c = k % 3
        other = copy_of(cols)
        if what == "value":
            for side in (cols, other):
                side[c][2][row] = True
            left = lay(rng, cols)
            other[c][1][row] = M._other(cols[c][0], cols[c][1][row])
        else:
            other[c][2][row] = not cols[c][2][row]
        wants = check_equal(left, lay(rng, other), "device" if k % 2 else "host")
        assert wants == [(False, row, c)] * 2


def test_difference_only_under_a_null_and_garbage_outside_the_rows():
    rng = np.random.default_rng(5)
    n = T + 65
    cols = frame(rng, n, 3, p_null=0.5)
    other = copy_of(cols)
    for typ, vals, valid in other:
        vals[~valid] = M._values(rng, typ, n)[~valid] if typ != "bool" else ~vals[~valid]
    for k in range(3):   # other payloads under the nulls, other bits and payloads outside [offset, offset + n)
        wants = check_equal(lay(rng, cols, stray_ones=bool(k % 2)), lay(rng, other, stray_ones=not k % 2), res_cycle(k, 3))
        assert wants == [(True, -1, -1)] * 2


@pytest.mark.parametrize("res", M.RESIDENCIES)
def test_bitmap_of_all_ones_against_no_bitmap(res):
    rng = np.random.default_rng(6)
    n = 2 * T + 1
    cols = frame(rng, n, 3, p_null=0.0)
    for known in (True, False):
        assert check_equal(lay(rng, cols, bitmaps=False), lay(rng, cols, known=known), res) == [(True, -1, -1)] * 2
        assert check_equal(lay(rng, cols, known=known), lay(rng, cols, bitmaps=False), res) == [(True, -1, -1)] * 2


@pytest.mark.parametrize("ncols", [5, 9])
def test_lower_row_in_a_higher_column_of_a_later_launch_group(ncols):
    rng = np.random.default_rng(ncols)
    n = 3 * T + 1
    cols = frame(rng, n, ncols, p_null=0.0)
    other = copy_of(cols)
    hi, lo = 2 * T + 5, T - 1
    other[0][1][hi] = M._other(cols[0][0], cols[0][1][hi])
    other[ncols - 1][1][lo] = M._other(cols[ncols - 1][0], cols[ncols - 1][1][lo])
    for res in ("host", "device"):
        assert check_equal(lay(rng, cols), lay(rng, other), res) == [(False, lo, ncols - 1)] * 2
    # ... and two columns differing at the same row, one in each group: the lower column
    other = copy_of(cols)
    for c in (ncols - 1, 2):
        other[c][1][lo] = M._other(cols[c][0], cols[c][1][lo])
    assert check_equal(lay(rng, cols), lay(rng, other), "device") == [(False, lo, 2)] * 2


def test_two_columns_differ_at_the_same_row():
    rng = np.random.default_rng(8)
    n = T + 1
    cols = frame(rng, n, 4, p_null=0.0)
    for row in (0, 63, 64, T - 1, T):
        other = copy_of(cols)
        other[3][1][row] = M._other(cols[3][0], cols[3][1][row])
        other[1][2][row] = False                       # a null against a value, in the lower column
        if row + 1 < n:
            other[0][1][row + 1] = M._other(cols[0][0], cols[0][1][row + 1])   # a still lower column, one row later
        assert check_equal(lay(rng, cols), lay(rng, other), "device") == [(False, row, 1)] * 2


def test_int64_values_that_differ_in_one_bit():
    n = 300
    base = np.arange(n, dtype=np.int64) * 3
    valid = np.ones(n, bool)
    rng = np.random.default_rng(9)
    for row, (a, b) in ((7, (4, 5)), (64, (0, -(1 << 63))), (299, ((1 << 53) + 2, (1 << 53) + 3)), (128, ((1 << 62) + 1, 1 << 62))):
        l, r = base.copy(), base.copy()
        l[row], r[row] = a, b
        wants = check_equal(lay(rng, [["int64", l, valid]]), lay(rng, [["int64", r, valid]]), "device")
        assert wants == [(False, row, 0)] * 2


def test_nan_and_signed_zeros():
    rng = np.random.default_rng(10)
    n = T + 7
    vals = rng.standard_normal(n)
    valid = rng.random(n) >= 0.3
    for row in (0, 100, T, n - 1):
        valid[row] = True
        for (a, b), (go, bits) in ((((M.NAN_A, M.NAN_A)), (False, True)), ((M.NAN_A, M.NAN_B), (False, False)), ((-0.0, 0.0), (True, False)),
                                   ((0.0, -0.0), (True, False)), ((np.inf, np.inf), (True, True))):
            l, r = vals.copy(), vals.copy()
            l[row], r[row] = a, b
            wants = check_equal(lay(rng, [["float64", l, valid]]), lay(rng, [["float64", r, valid]]), res_cycle(row, 1))
            assert wants == [(True, -1, -1) if go else (False, row, 0), (True, -1, -1) if bits else (False, row, 0)]
        # a NaN under a null on both sides differs from nothing
        l = vals.copy()
        l[row] = M.NAN_A
        nulled = valid.copy()
        nulled[row] = False
        assert check_equal(lay(rng, [["float64", l, nulled]]), lay(rng, [["float64", l, nulled]])) == [(True, -1, -1)] * 2


def test_a_frame_with_a_valid_nan_against_itself_on_the_same_device_buffers():
    rng = np.random.default_rng(11)
    n = 2 * T + 3
    cols = frame(rng, n, 3, first_type=1)    # float64, bool, int64
    row = T + 70
    cols[0][1][row], cols[0][2][row] = M.NAN_A, True
    placed = [column(p, "device") for p in lay(rng, cols)]
    assert capi.equal(placed, placed, capi.EQUAL_GO) == (False, row, 0)
    assert capi.equal(placed, placed, capi.EQUAL_BITS) == (True, -1, -1)
    cols[0][2][row] = False
    placed = [column(p, "device") for p in lay(rng, cols)]
    assert capi.equal(placed, placed, capi.EQUAL_GO) == (True, -1, -1)


@pytest.mark.parametrize("ncols", M.NCOLS)
def test_column_counts_and_mixed_residencies(ncols):
    rng = np.random.default_rng(20 + ncols)
    n = T + 257
    cols = frame(rng, n, ncols, first_type=ncols)
    for k in range(3):
        assert check_equal(lay(rng, cols), lay(rng, cols), res_cycle(k, ncols)) == [(True, -1, -1)] * 2
        other = copy_of(cols)
        c, row = (ncols - 1, n - 1) if k % 2 else (ncols // 2, 64)
        other[c][2][row] = not cols[c][2][row]
        assert check_equal(lay(rng, cols), lay(rng, other), res_cycle(k, ncols)) == [(False, row, c)] * 2


@pytest.mark.parametrize("left_offset", M.OFFSETS)
def test_arrow_offsets_chosen_independently(left_offset):
    rng = np.random.default_rng(30 + left_offset)
    n = 1025
    cols = frame(rng, n, 3, first_type=left_offset)
    other = copy_of(cols)
    other[2][2][n - 1] = not cols[2][2][n - 1]
    for k, right_offset in enumerate(M.OFFSETS):
        lo = [left_offset, M.OFFSETS[(k + 3) % 8], right_offset]
        ro = [right_offset, left_offset, M.OFFSETS[(k + 5) % 8]]
        res = "device" if k % 2 else "host"
        assert check_equal(lay(rng, cols, lo, stray_ones=bool(k & 2)), lay(rng, cols, ro), res) == [(True, -1, -1)] * 2
        assert check_equal(lay(rng, cols, lo), lay(rng, other, ro, stray_ones=bool(k & 2)), res) == [(False, n - 1, 2)] * 2


# ------------------------------------------------------------------ the valid-row search
def bitmap_col(rng, typ, valid, offset=None, **kw):
    n = len(valid)
    off = M.OFFSETS[int(rng.integers(len(M.OFFSETS)))] if offset is None else offset
    return M.pcol(rng, typ, None if typ == "utf8" else M._values(rng, typ, n), valid, off, stray_ones=True, **kw)


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 4097, 12289])
def test_valid_row_where_the_answer_lies(n, direction):
    """at row_start; in its 64-row word on both sides; in the next word; in another tile; at row 0 and at row n - 1; nowhere"""
    rng = np.random.default_rng(n)
    starts = sorted({0, n - 1, n // 2, min(n - 1, 70), min(n - 1, T + 100), min(n - 1, 2 * T)})
    for k, start in enumerate(starts):
        ahead = np.arange(start, n) if direction > 0 else np.arange(start, -1, -1)
        targets = {start, int(ahead[min(len(ahead) - 1, 3)]), int(ahead[min(len(ahead) - 1, 64)]), int(ahead[min(len(ahead) - 1, 130)]),
                   int(ahead[min(len(ahead) - 1, T + 3)]), int(ahead[-1])}
        for target in sorted(targets) + [None]:
            valid = np.zeros(n, bool)
            if target is not None:
                valid[target] = True
                valid[ahead[-1]] = True        # a farther one
            wrong = start - direction          # right next to row_start, on the wrong side
            if 0 <= wrong < n:
                valid[wrong] = True
            typ = ["float64", "utf8", "bool", "int64"][k % 4]
            want = check_valid_row([bitmap_col(rng, typ, valid, known=bool(k % 2))], start, direction, M.RESIDENCIES[k % 3])
            assert want == (-1 if target is None else target)


@pytest.mark.parametrize("ncols", [2, 8])
def test_valid_row_of_interleaved_columns_with_one_common_row(ncols):
    rng = np.random.default_rng(ncols)
    n = 3 * T + 11
    for common in (0, 63, 64, T - 1, T, 2 * T + 70, n - 1):
        cols = []
        for c in range(ncols):
            valid = (np.arange(n) + c) % 2 == 0        # column c and column c + 1 never meet ...
            valid[common] = True                        # ... but here
            cols.append(bitmap_col(rng, ["int64", "bool", "utf8", "float64"][c % 4], valid, known=bool(c % 2)))
        res = [M.RESIDENCIES[(c + common) % 3] for c in range(ncols)]
        for start in (0, common, n - 1, max(0, common - 1), min(n - 1, common + 1)):
            assert check_valid_row(cols, start, -1, res) == (common if start >= common else -1)
            assert check_valid_row(cols, start, +1, res) == (common if start <= common else -1)


def test_valid_row_offsets_that_differ_and_columns_that_drop_out():
    rng = np.random.default_rng(40)
    n = T + 300
    valid = rng.random(n) < 0.02
    for k, offs in enumerate(((0, 1, 63), (7, 8, 31), (33, 32, 0), (63, 63, 1))):
        a = bitmap_col(rng, "bool", valid | (rng.random(n) < 0.3), offs[0])
        b = bitmap_col(rng, "utf8", valid | (rng.random(n) < 0.3), offs[1], known=False)
        c = M.pcol(rng, "int64", M._values(rng, "int64", n), None, offs[2])                    # no bitmap: drops out
        d = M.pcol(rng, "float64", M._values(rng, "float64", n), np.ones(n, bool), offs[2])   # all ones
        for start in (0, 64, 1000, T, n - 1):
            for direction in (-1, 1):
                check_valid_row([a, b, c, d], start, direction, [M.RESIDENCIES[(k + j) % 3] for j in range(4)])
                assert check_valid_row([c], start, direction, "device") == start
                assert check_valid_row([c, d], start, direction, "device") == start


# ------------------------------------------------------------------ IsColEmpty
@pytest.mark.parametrize("res", M.RESIDENCIES)
@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_is_col_empty(n, res):
    rng = np.random.default_rng(n)
    shapes = [(np.zeros(n, bool), True)]
    for row in {0, n - 1}:
        valid = np.zeros(n, bool)
        valid[row] = True
        shapes.append((valid, False))
    for k, (valid, want) in enumerate(shapes):
        for known in (True, False):
            for typ in ("float64", "bool", "utf8"):
                c = column(bitmap_col(rng, typ, valid, known=known), res)
                try:
                    assert capi.is_col_empty(c) == want == M.is_col_empty((None, valid))
                finally:
                    release([c])


# ------------------------------------------------------------------ the mirror, the fuzz
def test_cpp_mirror():
    exe = os.path.join(ROOT, "tests", "cpp", "test_equal")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failures" in p.stdout


@pytest.mark.parametrize("block", range(4))
def test_fuzz_over_the_seeded_plan(block):
    seeds = int(os.environ.get("BOW_FUZZ_SEEDS", "64"))
    for seed in range(block, seeds, 4):
        case = M.equal_case(seed)
        check_equal(case["left"], case["right"], case["residency"])
        vr = M.valid_row_case(seed)
        check_valid_row(vr["cols"], vr["row_start"], vr["direction"], vr["residency"])
        for p, res in zip(vr["cols"][:2], vr["residency"]):
            c = column(p, res)
            try:
                assert capi.is_col_empty(c) == M.is_col_empty((None, np.ones(p.length, bool) if p.bits is None else p.logical()[1])), seed
            finally:
                release([c])
