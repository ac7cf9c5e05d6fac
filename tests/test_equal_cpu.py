"""bowgpu_equal / bowgpu_valid_row / bowgpu_is_col_empty without a GPU: the symbols, everything the header says is answered without a
device, every decline with its code, and no CPU fallback for a call that has rows to look at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bowgpu_equal", "bowgpu_valid_row", "bowgpu_is_col_empty"]
ARG, UNSUPPORTED, NO_DEVICE = -10, -9, -11


def col(data, typ):
    return capi.Column.from_list(data, typ)


def claimed(n, typ=capi.INT64, validity=False):
    """a host column that CLAIMS n rows over a tiny buffer: only what is decided before any data is read may be asked of it"""
    return capi.Column(np.zeros(8, np.int64), np.zeros(8, np.uint8) if validity else None, typ, 0, n, -1)


def code_of(fn, *args):
    with pytest.raises(capi.BowGpuError) as e:
        fn(*args)
    return e.value.code, e.value.message


def test_header_and_binding_hold_the_symbols():
    header = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    assert int(re.search(r"#define BOWGPU_ABI_VERSION (\d+)", header).group(1)) == 14 == capi.ABI_VERSION == capi.lib().bowgpu_abi_version()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert re.search(r"BOWGPU_EQUAL_GO = 0", code) and re.search(r"BOWGPU_EQUAL_BITS = 1", code)
    assert (capi.EQUAL_GO, capi.EQUAL_BITS) == (0, 1)
    assert int(re.search(r"#define BOWGPU_VALID_ROW_MAX_COLS (\d+)", code).group(1)) == capi.VALID_ROW_MAX_COLS == 8
    assert C.sizeof(capi.EqualInfo) == 16
    assert "(still 14): bowgpu_equal" in header


@pytest.mark.parametrize("mode", [capi.EQUAL_GO, capi.EQUAL_BITS])
def test_equal_answered_without_a_device(mode):
    assert capi.equal([], [], mode) == (True, -1, -1)                                                     # zero columns
    assert capi.equal([col([], "int64"), col([], "bool")], [col([], "int64"), col([], "bool")], mode) == (True, -1, -1)   # zero rows
    # the types of column 1 and 2 differ: the lowest such column, before the lengths are looked at
    left = [col([1, 2], "int64"), col([1.0, 2.0], "float64"), col([True, False], "bool")]
    right = [col([1], "int64"), col([1], "int64"), col([1.0], "float64")]
    assert capi.equal(left, right, mode) == (False, -1, 1)
    assert capi.equal([col([1, 2], "int64")], [col([1], "int64")], mode) == (False, -1, -1)              # lengths differ
    assert capi.equal([col([], "float64")], [col([0.5], "float64")], mode) == (False, -1, -1)
    assert capi.equal([claimed(1000)], [claimed(999)], mode) == (False, -1, -1)                           # (no row is read)


def test_equal_declines():
    i2, f2, s2 = col([1, 2], "int64"), col([1.0, 2.0], "float64"), capi.Column(np.zeros(8, np.uint8), None, capi.STRING, 0, 2, 0)
    assert code_of(capi.equal, [i2, s2], [i2, s2])[0] == UNSUPPORTED                                      # String on both sides
    assert code_of(capi.equal, [s2], [i2])[0] == UNSUPPORTED and code_of(capi.equal, [i2], [s2])[0] == UNSUPPORTED
    for mode in (-1, 2, 7):
        assert code_of(capi.equal, [i2], [i2], mode)[0] == ARG
    assert code_of(capi.equal, [i2, col([1.0], "float64")], [i2, f2])[0] == ARG                           # unequal lengths within a frame
    assert code_of(capi.equal, [i2, f2], [i2, col([1.0, 2.0, 3.0], "float64")])[0] == ARG
    code, msg = code_of(capi.equal, [claimed(1 << 31)], [claimed(1 << 31)])
    assert code == UNSUPPORTED and "2^31" in msg
    info = capi.EqualInfo()
    arr = capi._cols([i2])
    assert capi.lib().bowgpu_equal(arr, arr, -1, 0, C.byref(info)) == ARG
    assert capi.lib().bowgpu_equal(arr, arr, 1, 0, None) == ARG


def test_valid_row_answered_without_a_device():
    n = 10
    with_nulls = col([1, None, 3, None, 5, 6, None, 8, 9, None], "int64")
    for direction in (-1, 1):
        for start in (-5, -1, n, n + 3):                                                                  # the loops' guard; a negative start is no error
            assert capi.valid_row([with_nulls], start, direction) == -1
        # no nulls to look at: no bitmap, or null_count stated as 0 (the bitmap is then not read) - whatever the type
        plain = [capi.Column(np.zeros(n, np.int64), None, capi.INT64, 0, n, 0),
                 capi.Column(np.zeros(n, np.float64), np.zeros(2, np.uint8), capi.FLOAT64, 0, n, 0),
                 capi.Column(np.zeros(8, np.uint8), None, capi.STRING, 0, n, 0), capi.Column(np.zeros(8, np.uint8), None, capi.BOOLEAN, 3, n, 0)]
        for start in (0, 4, n - 1):
            assert capi.valid_row(plain, start, direction) == start
            assert capi.valid_row(plain[:1], start, direction) == start
        assert capi.valid_row([claimed((1 << 31) - 1)], 12345, direction) == 12345


def test_valid_row_declines():
    c = col([1, None, 3], "int64")
    assert code_of(capi.valid_row, [], 0, 1)[0] == ARG
    code, msg = code_of(capi.valid_row, [c] * (capi.VALID_ROW_MAX_COLS + 1), 0, 1)
    assert code == ARG and "BOWGPU_VALID_ROW_MAX_COLS = 8" in msg
    for direction in (0, 2, -2):
        assert code_of(capi.valid_row, [c], 0, direction)[0] == ARG
    assert code_of(capi.valid_row, [c, col([1, 2], "int64")], 0, 1)[0] == ARG                             # unequal lengths
    code, msg = code_of(capi.valid_row, [claimed(1 << 31, validity=True)], 0, 1)
    assert code == UNSUPPORTED and "2^31" in msg


def test_is_col_empty_answered_without_a_device():
    assert capi.is_col_empty(col([], "int64")) and capi.is_col_empty(col([], "utf8"))                     # 0 == 0
    assert capi.is_col_empty(col([None, None, None], "float64"))                                          # null_count stated: 3 == 3
    assert not capi.is_col_empty(col([None, 2.0, None], "float64"))
    assert not capi.is_col_empty(col([True], "bool"))
    assert not capi.is_col_empty(capi.Column(np.zeros(4, np.int64), None, capi.INT64, 0, 4, 0))           # no bitmap
    assert not capi.is_col_empty(capi.Column(np.zeros(8, np.int64), np.zeros(8, np.uint8), capi.INT64, 0, 1 << 40, 0))   # null_count stated as 0
    assert capi.is_col_empty(capi.Column(np.zeros(8, np.uint8), np.zeros(8, np.uint8), capi.STRING, 0, 1 << 40, 1 << 40))


def test_no_cpu_fallback_without_gpu():
    try:
        n = capi.device_count()
    except capi.BowGpuError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is present")
    a, b = col([1, None, 3], "int64"), col([1, None, 4], "int64")
    assert code_of(capi.equal, [a], [b])[0] == NO_DEVICE
    assert code_of(capi.equal, [a], [a], capi.EQUAL_BITS)[0] == NO_DEVICE
    assert code_of(capi.valid_row, [a], 1, -1)[0] == NO_DEVICE
    unknown = capi.Column(np.zeros(3, np.int64), np.array([5], np.uint8), capi.INT64, 0, 3, -1)
    assert code_of(capi.is_col_empty, unknown)[0] == NO_DEVICE
