"""Bow.SortByCol on the GPU (bowgpu_argsort / bowgpu_take / bowgpu_sort_by_col, bow_amd/csrc/sort.hip) through the C ABI.
Expected results: the reference's own test literals (tests/golden/sort_vectors.json) and numpy - np.argsort(kind="stable") on the
key image the header defines (x ^ 2^63 for Int64; the sign-flip map for Float64 with -0 folded onto +0) - with every comparison
exact: permutations index for index, columns bit for bit (values, validity bits, null counts, zeroed null slots, clear padding)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import psutil
import pytest

from bow_amd import capi
from test_sort_cpu import sort_vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = {"float64": capi.FLOAT64, "int64": capi.INT64}
SIGN = np.uint64(1 << 63)


def image(key):
    """the unsigned 64-bit image whose order is Buffer.Less (bowbuffer.go:126-139)"""
    key = np.ascontiguousarray(key)
    bits = key.view(np.uint64).copy()
    if key.dtype == np.float64:
        bits[(bits << np.uint64(1)) == 0] = 0                      # -0.0 == +0.0 under Less
        neg = (bits >> np.uint64(63)) == 1
        return np.where(neg, ~bits, bits ^ SIGN)
    return bits ^ SIGN


def stable_perm(key):
    return np.argsort(image(key), kind="stable").astype(np.int64)


def col_of(values, valid=None, typ=None, offset=0, length=None):
    """a host Column; valid: bool mask over the whole buffer (None: no bitmap)"""
    bm = None if valid is None else np.packbits(valid, bitorder="little")
    return capi.Column(values, bm, typ, offset, length, -1)


def place(col, residency):
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


def compare_taken(name, got, values, valid, perm, typ):
    """got: OutColumn; want: values[perm] / valid[perm] of the logical column"""
    n = len(perm)
    assert got.length == n and got.type == typ, (name, got.length, got.type)
    gv, gb = got.host_arrays()
    gm = got.valid_mask()
    wm = np.ones(n, bool) if valid is None else valid[perm]
    assert np.array_equal(gm, wm), (name, np.flatnonzero(gm != wm)[:10])
    assert got.null_count == int((~wm).sum()), (name, got.null_count)
    gbits, wbits = gv.view(np.uint64), np.ascontiguousarray(values).view(np.uint64)[perm]
    assert not gbits[~gm].any(), name                      # null slots hold 0
    bad = np.flatnonzero(gbits[gm] != wbits[wm])
    assert bad.size == 0, (name, bad[:10])
    if n % 8:
        assert (gb[-1] >> (n % 8)) == 0, name              # padding bits of the last validity byte stay clear


def check_argsort(name, key, residency=capi.HOST, out_residency=capi.HOST, offset=0, length=None):
    typ = capi.INT64 if key.dtype == np.int64 else capi.FLOAT64
    col = place(capi.Column(key, None, typ, offset, length), residency)
    logical = key[offset:offset + col.length]
    want = stable_perm(logical)
    img = image(logical)
    is_sorted = not (img[1:] < img[:-1]).any()
    perm, said = capi.argsort(col, out_residency)
    assert said == is_sorted, (name, said, is_sorted)
    if is_sorted:
        assert perm is None
        return
    if out_residency == capi.DEVICE:
        perm = perm.to_numpy(np.int64, col.length)
    bad = np.flatnonzero(perm != want)
    assert bad.size == 0, (name, bad[:10], perm[bad[:5]], want[bad[:5]])
    if residency == capi.HOST_PINNED:
        col.unpin()


# ------------------------------------------------------------------ the reference's own tables
def test_golden_vectors():
    for case in sort_vectors()["cases"]:
        cols = [capi.Column.from_list(c["data"], c["type"]) for c in case["cols"]]
        if "error" in case:
            with pytest.raises(capi.BowGpuError) as e:
                capi.sort_by_col(cols, case["key_col"])
            assert e.value.code == case["error"]["code"] and e.value.message == case["error"]["message"], case["name"]
            continue
        for res in (capi.HOST, capi.DEVICE):
            outs, unchanged = capi.sort_by_col([place(c, res) for c in cols], case["key_col"], out_residency=res)
            assert unchanged == ("unchanged" in case), case["name"]
            if unchanged:
                continue
            n = len(case["cols"][0]["data"])
            for c, o in zip(case["expected"], outs):
                assert o.to_list() == c["data"], (case["name"], c["name"], o.to_list())
                vals, valid = np.array([0 if x is None else x for x in c["data"]], np.int64 if c["type"] == "int64" else np.float64), \
                    np.array([x is not None for x in c["data"]], bool)
                compare_taken(case["name"] + " " + c["name"], o, np.where(valid, vals, 0).astype(vals.dtype), valid, np.arange(n), T[c["type"]])


# ------------------------------------------------------------------ argsort against the stable permutation of the image
SIZES = [0, 1, 2, 63, 64, 65, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 1_000_007]


def _int_keys(rng, n):
    i64 = np.iinfo(np.int64)
    yield "unique shuffled", rng.permutation(n).astype(np.int64)
    yield "ties 0..15", rng.integers(0, 16, n).astype(np.int64)
    mixed = rng.integers(i64.min, i64.max, n, dtype=np.int64, endpoint=True)
    if n >= 4:
        mixed[rng.integers(0, n, 2)] = i64.min
        mixed[rng.integers(0, n, 2)] = i64.max
        mixed[rng.integers(0, n)] = 0
        mixed[rng.integers(0, n)] = -1
    yield "negative and positive, extremes", mixed
    yield "top byte only", (rng.integers(-128, 128, n).astype(np.int64) << 56) | 0x1234
    yield "lowest byte only", rng.integers(0, 256, n).astype(np.int64) + (0x1122334455 << 8)
    yield "byte 3 only", (rng.integers(0, 256, n).astype(np.int64) << 24) | 0x5500AABBCC
    yield "reversed", np.arange(n, 0, -1, dtype=np.int64)
    yield "sorted with ties", np.sort(rng.integers(0, max(n // 3, 1), n)).astype(np.int64)


def _float_keys(rng, n):
    f = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 0.0, -0.0, 1.0, -1.0])
    if n >= 4:
        at = rng.integers(0, n, min(n, 200))
        f[at] = special[rng.integers(0, len(special), len(at))]
    yield "floats with +-0, +-inf, subnormals", f
    yield "zeros of both signs", np.where(rng.random(n) < 0.5, 0.0, -0.0)
    yield "float ties", rng.integers(-3, 4, n).astype(np.float64) / 2


@pytest.mark.parametrize("n", SIZES)
def test_argsort_matches_stable_numpy(n):
    rng = np.random.default_rng(1000 + n)
    for name, key in _int_keys(rng, n):
        check_argsort("%s n=%d" % (name, n), key)
    for name, key in _float_keys(rng, n):
        check_argsort("%s n=%d" % (name, n), key)


def test_argsort_16m_rows_device_resident():
    n = 16_000_000
    rng = np.random.default_rng(16)
    check_argsort("unique shuffled 1.6e7", rng.permutation(n).astype(np.int64), capi.DEVICE, capi.DEVICE)
    check_argsort("ties 1.6e7", rng.integers(0, 16, n).astype(np.int64), capi.DEVICE, capi.DEVICE)
    check_argsort("floats 1.6e7", rng.standard_normal(n), capi.DEVICE, capi.HOST)


def test_argsort_sliced_columns_and_residencies():
    rng = np.random.default_rng(5)
    base = rng.integers(-1000, 1000, 70_000).astype(np.int64)
    fbase = rng.standard_normal(70_000)
    for off, length in ((1, 4097), (3, 65_537), (7, 69_000), (13, 1), (63, 64), (4095, 4098)):
        for res in (capi.HOST, capi.DEVICE, capi.HOST_PINNED):
            check_argsort("slice int off=%d" % off, base, res, capi.HOST, off, length)
            check_argsort("slice float off=%d" % off, fbase, res, capi.DEVICE, off, length)


# ------------------------------------------------------------------ whole frames
def _frame(rng, n, ncols, null_frac):
    """column 0: Int64 key with ties; the rest alternate Float64 / Int64; null_frac None: no bitmap at all"""
    key = rng.integers(-n // 2, n // 2 + 1, n).astype(np.int64)
    cols = [(key, None, capi.INT64)]
    for c in range(1, ncols):
        if c % 2:
            v = rng.standard_normal(n)
            nan_at = rng.integers(0, n, max(n // 50, 1))
            payload = (np.uint64(0x7FF0000000000001) | (rng.integers(1, 1 << 40, len(nan_at)).astype(np.uint64) << np.uint64(3)) |
                       (rng.integers(0, 2, len(nan_at)).astype(np.uint64) << np.uint64(63)))
            v.view(np.uint64)[nan_at] = payload            # NaNs with payloads and signs: the bits must survive
            typ = capi.FLOAT64
        else:
            v = rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64)
            typ = capi.INT64
        valid = None if null_frac is None else rng.random(n) >= null_frac
        cols.append((v, valid, typ))
    return cols


@pytest.mark.parametrize("ncols", [1, 3, 9])
def test_sort_by_col_frames(ncols):
    n = 50_003
    for null_frac in (None, 0.0, 0.3, 1.0):
        rng = np.random.default_rng(ncols * 10 + int((null_frac or 0) * 10))
        frame = _frame(rng, n, ncols, null_frac)
        perm = stable_perm(frame[0][0])
        for res in (capi.HOST, capi.DEVICE, capi.HOST_PINNED):
            for out_res in (capi.HOST, capi.DEVICE):
                cols = [place(col_of(v, m, t), res) for v, m, t in frame]
                outs, unchanged = capi.sort_by_col(cols, 0, out_residency=out_res)
                assert not unchanged
                for i, ((v, m, t), o) in enumerate(zip(frame, outs)):
                    want_vals = v if m is None else np.where(m, v.view(np.uint64), np.uint64(0)).view(v.dtype)
                    compare_taken("ncols=%d nulls=%s res=%d/%d col %d" % (ncols, null_frac, res, out_res, i), o, want_vals, m, perm, t)
                assert capi.is_col_sorted(capi.out_as_column(outs[0]))
                if res == capi.HOST_PINNED:
                    for c in cols:
                        c.unpin()


def test_sort_by_col_other_key_column_float_key_and_odd_offsets():
    rng = np.random.default_rng(77)
    total, off, n = 20_000, 13, 19_001
    key = rng.integers(-50, 50, total).astype(np.float64) / 4
    key[rng.integers(0, total, 50)] = -0.0
    a = rng.integers(0, 1000, total).astype(np.int64)
    b = rng.standard_normal(total)
    ma, mb = rng.random(total) > 0.3, rng.random(total) > 0.5
    perm = stable_perm(key[off:off + n])
    for res in (capi.HOST, capi.DEVICE):
        cols = [place(col_of(a, ma, capi.INT64, off, n), res), place(col_of(b, mb, capi.FLOAT64, off, n), res),
                place(capi.Column(key, None, capi.FLOAT64, off, n), res)]
        outs, unchanged = capi.sort_by_col(cols, 2, out_residency=res)
        assert not unchanged
        for name, o, v, m, t in (("a", outs[0], a, ma, capi.INT64), ("b", outs[1], b, mb, capi.FLOAT64), ("key", outs[2], key, None, capi.FLOAT64)):
            lv = v[off:off + n]
            lm = None if m is None else m[off:off + n]
            want = lv if lm is None else np.where(lm, lv.view(np.uint64), np.uint64(0)).view(lv.dtype)
            compare_taken("float key %s res=%d" % (name, res), o, want, lm, perm, t)   # (-0.0 / +0.0 keep their own bits and their input order)


# ------------------------------------------------------------------ frames wider than one gather launch, mixed inside a group
MOVE_ROWS = [1, 63, 64, 65, 4095, 4096, 4097]          # validity-word and tile edges
RES3 = (capi.HOST, capi.HOST_PINNED, capi.DEVICE)


@pytest.mark.parametrize("n", MOVE_ROWS)
@pytest.mark.parametrize("ncols,key_col", [(5, 4), (9, 5)], ids=["5cols-key4", "9cols-key5"])
def test_sort_by_col_key_in_the_second_group_mixed_columns(ncols, key_col, n):
    """Launch groups of 4 + 1 and 4 + 4 + 1 columns.  The key, staged once for the sort, is moved with the second group; inside every
    group the inputs differ in residency and in having nulls, the outputs in residency"""
    rng = np.random.default_rng(100 * ncols + n)
    frame = _frame(rng, n, ncols, 0.3)
    frame[0], frame[key_col] = frame[key_col], frame[0]
    frame = [(v, m if i % 2 and i != key_col else None, t) for i, (v, m, t) in enumerate(frame)]
    key = frame[key_col][0]
    perm = stable_perm(key)
    is_sorted = not (image(key)[1:] < image(key)[:-1]).any()
    cols = [place(col_of(v, m, t), RES3[i % 3]) for i, (v, m, t) in enumerate(frame)]
    outs = [capi.OutColumn(n, (capi.HOST, capi.DEVICE)[(i // 2) % 2]) for i in range(ncols)]
    try:
        outs, unchanged = capi.sort_by_col(cols, key_col, outs=outs)
        assert unchanged == is_sorted and is_sorted == (n == 1)
        if not unchanged:
            for i, ((v, m, t), o) in enumerate(zip(frame, outs)):
                want_vals = v if m is None else np.where(m, v.view(np.uint64), np.uint64(0)).view(v.dtype)
                compare_taken("ncols=%d key=%d n=%d col %d" % (ncols, key_col, n, i), o, want_vals, m, perm, t)
    finally:
        for c in cols:
            if c.residency == capi.HOST_PINNED:
                c.unpin()


@pytest.mark.parametrize("idx_res", RES3, ids=["idx-host", "idx-pinned", "idx-device"])
def test_take_index_list_residencies(idx_res):
    """the index list as pageable host memory (staged), registered host memory (read in place) and device memory; capi.take
    passes the first and the last only, so the call is made here"""
    rng = np.random.default_rng(31)
    n = 5000
    v = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
    m = rng.random(n) > 0.3
    col = col_of(v, m, capi.INT64).to_device()
    want_vals = np.where(m, v, 0)
    for k, n_idx in enumerate(MOVE_ROWS):
        idx = rng.integers(0, n, n_idx).astype(np.int64)
        held = idx
        if idx_res == capi.DEVICE:
            held = capi.DeviceBuffer.from_numpy(idx)
        elif idx_res == capi.HOST_PINNED:
            held = capi.page_aligned(n_idx, np.int64)
            held[:] = idx
            capi.host_register(held)
        out = capi.OutColumn(n_idx, (capi.HOST, capi.DEVICE)[k % 2])
        o, c = out.c(), col.c()
        try:
            ptr = C.c_void_p(held.ptr) if idx_res == capi.DEVICE else held.ctypes.data_as(C.c_void_p)
            capi.check(capi.lib().bowgpu_take(C.byref(c), ptr, C.c_int64(n_idx), idx_res, C.byref(o)))
        finally:
            if idx_res == capi.HOST_PINNED:
                capi.host_unregister(held)
        out.absorb(o)
        compare_taken("take idx_res=%d n_idx=%d" % (idx_res, n_idx), out, want_vals, m, idx, capi.INT64)


def _sentinel_outs(n, ncols, residency):
    outs = [capi.OutColumn(n, residency) for _ in range(ncols)]
    if residency == capi.DEVICE:
        for o in outs:
            capi.check(capi.lib().bowgpu_memset(C.c_void_p(o.values.ptr), 0x5A, C.c_int64(8 * n)))
            capi.check(capi.lib().bowgpu_memset(C.c_void_p(o.validity.ptr), 0xA5, C.c_int64((n + 7) // 8)))
    return outs


def _untouched(outs, n):
    for o in outs:
        assert o.null_count == -1 and o.type == 0 and o.length == n
        if o.residency == capi.DEVICE:
            vals, bm = o.values.to_numpy(np.uint64, n), o.validity.to_numpy(np.uint8, (n + 7) // 8)
        else:
            vals, bm = o.values[:n], o.validity[:(n + 7) // 8]
        assert (vals == 0x5A5A5A5A5A5A5A5A).all() and (bm == 0xA5).all()


def test_already_sorted_is_unchanged_and_writes_nothing():
    n = 100_001
    rng = np.random.default_rng(3)
    val = rng.standard_normal(n)
    for name, key in (("strictly ascending", np.arange(n, dtype=np.int64) * 3 - 1000), ("ascending with ties", np.sort(rng.integers(0, 100, n)).astype(np.int64)),
                      ("all equal", np.full(n, 7, np.int64)), ("float zeros of both signs then ones", np.r_[np.where(rng.random(n - 5) < 0.5, 0.0, -0.0), np.ones(5)])):
        typ = capi.INT64 if key.dtype == np.int64 else capi.FLOAT64
        for res in (capi.HOST, capi.DEVICE):
            cols = [place(capi.Column(key, None, typ), res), place(capi.Column(val, None, capi.FLOAT64), res)]
            outs = _sentinel_outs(n, 2, res)
            _, unchanged = capi.sort_by_col(cols, 0, outs=outs)
            assert unchanged, name
            _untouched(outs, n)
            perm, is_sorted = capi.argsort(cols[0])
            assert is_sorted and perm is None, name
    # one row out of place at the very end / the very start / across a 64-row boundary
    for at in (n - 1, 1, 64, 4096, 65_536):
        key = np.arange(n, dtype=np.int64)
        key[at] = key[at - 1] - 1
        check_argsort("one descent at %d" % at, key, capi.DEVICE)
    key = np.arange(n, 0, -1, dtype=np.int64)
    outs, unchanged = capi.sort_by_col([capi.Column(key, None, capi.INT64), capi.Column(val, None, capi.FLOAT64)], 0)
    assert not unchanged
    compare_taken("reversed key", outs[0], key, None, np.arange(n - 1, -1, -1), capi.INT64)
    compare_taken("reversed val", outs[1], val, None, np.arange(n - 1, -1, -1), capi.FLOAT64)


def test_declines():
    key = np.array([3.0, np.nan, 1.0, 2.0])
    for res in (capi.HOST, capi.DEVICE):
        with pytest.raises(capi.BowGpuError) as e:
            capi.argsort(place(capi.Column(key, None, capi.FLOAT64), res))
        assert e.value.code == -9, res
        with pytest.raises(capi.BowGpuError) as e:
            capi.sort_by_col([place(capi.Column(key, None, capi.FLOAT64), res)], 0)
        assert e.value.code == -9, res
    # a NaN is UNSUPPORTED even where the rest of the key is in order
    with pytest.raises(capi.BowGpuError) as e:
        capi.argsort(capi.Column(np.array([1.0, 2.0, np.nan]), None, capi.FLOAT64))
    assert e.value.code == -9
    # nulls in a device-resident key whose null count the caller does not know
    n = 10_000
    valid = np.ones(n, bool)
    valid[[17, 4096, 9999]] = False
    dev = col_of(np.arange(n, 0, -1, dtype=np.int64), valid, capi.INT64).to_device()
    assert dev.null_count == -1
    for call in (lambda: capi.argsort(dev), lambda: capi.sort_by_col([dev], 0)):
        with pytest.raises(capi.BowGpuError) as e:
            call()
        assert e.value.code == -16 and e.value.message == "column to sort by has 3 nil values"


def test_take():
    rng = np.random.default_rng(9)
    n = 30_000
    v = rng.standard_normal(n)
    m = rng.random(n) > 0.4
    for res in (capi.HOST, capi.DEVICE):
        col = place(col_of(v, m, capi.FLOAT64), res)
        # repeated indices, n_idx != length; the last: 65 rows into the second round of the gather's grid-stride loop (its grid is capped
        # at 2048 workgroups of 256 threads)
        for n_idx in (1, 63, 64, 65, 7, 100_003, 2048 * 256 + 65):
            idx = rng.integers(0, n, n_idx).astype(np.int64)
            want_vals = np.where(m, v.view(np.uint64), np.uint64(0)).view(np.float64)
            compare_taken("take host idx n=%d" % n_idx, capi.take(col, idx, out_residency=res), want_vals, m, idx, capi.FLOAT64)
            d_idx = capi.DeviceBuffer.from_numpy(idx)
            compare_taken("take device idx n=%d" % n_idx, capi.take(col, d_idx, n_idx, out_residency=capi.DEVICE), want_vals, m, idx, capi.FLOAT64)
        for bad in (n, -1, 1 << 40, -(1 << 62)):
            idx = rng.integers(0, n, 1000).astype(np.int64)
            idx[rng.integers(0, 1000)] = bad
            with pytest.raises(capi.BowGpuError) as e:
                capi.take(col, idx)
            assert e.value.code == -10, bad
    # a slice at an odd offset: indices are relative to the slice
    sl = col_of(v, m, capi.FLOAT64, 5, 1000).to_device()
    idx = rng.integers(0, 1000, 777).astype(np.int64)
    compare_taken("take from a slice", capi.take(sl, idx), np.where(m, v.view(np.uint64), np.uint64(0)).view(np.float64)[5:1005], m[5:1005], idx, capi.FLOAT64)
    with pytest.raises(capi.BowGpuError) as e:
        capi.take(sl, np.array([1000], np.int64))
    assert e.value.code == -10


def _raw(outs):
    blobs = []
    for o in outs:
        v, b = o.host_arrays()
        blobs.append((v.view(np.uint64).copy(), b.copy(), o.null_count))
    return blobs


def test_same_call_twice_gives_the_same_bytes():
    rng = np.random.default_rng(21)
    frame = _frame(rng, 300_007, 3, 0.3)
    frame[0] = (rng.integers(0, 40, 300_007).astype(np.int64), None, capi.INT64)     # long runs of ties: where an unstable scatter would show
    cols = [col_of(v, m, t).to_device() for v, m, t in frame]
    first = _raw(capi.sort_by_col(cols, 0, out_residency=capi.DEVICE)[0])
    p1 = capi.argsort(cols[0])[0]
    for _ in range(3):
        again = _raw(capi.sort_by_col(cols, 0, out_residency=capi.DEVICE)[0])
        for (v0, b0, n0), (v1, b1, n1) in zip(first, again):
            assert np.array_equal(v0, v1) and np.array_equal(b0, b1) and n0 == n1
        assert np.array_equal(p1, capi.argsort(cols[0])[0])


def test_two_threads_sort_different_frames_at_once():
    frames = {t: _frame(np.random.default_rng(500 + t), 120_000 + 1111 * t, 3, 0.3) for t in range(2)}
    errors = []
    start = threading.Barrier(2)

    def worker(t):
        try:
            frame = frames[t]
            perm = stable_perm(frame[0][0])
            start.wait()
            for rep in range(6):
                res = capi.DEVICE if rep % 2 else capi.HOST
                outs, unchanged = capi.sort_by_col([place(col_of(v, m, ty), res) for v, m, ty in frame], 0, out_residency=res)
                assert not unchanged
                for i, ((v, m, ty), o) in enumerate(zip(frame, outs)):
                    want = v if m is None else np.where(m, v.view(np.uint64), np.uint64(0)).view(v.dtype)
                    compare_taken("thread %d rep %d col %d" % (t, rep, i), o, want, m, perm, ty)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ------------------------------------------------------------------ the reason for the feature
def test_shuffled_frame_sorted_on_the_device_feeds_rolling_aggregate():
    rng = np.random.default_rng(2024)
    n = 200_003
    ts = np.cumsum(rng.integers(1, 5, n)).astype(np.int64)        # unique timestamps
    val = np.round(rng.standard_normal(n), 2)
    valid = rng.random(n) > 0.3
    aggs = [("WindowStart", 0), ("ArithmeticMean", 1), ("Min", 1), ("Count", 1)]
    ordered = [capi.Column(ts, None, capi.INT64).to_device(), col_of(val, valid, capi.FLOAT64).to_device()]
    want, _ = capi.rolling_aggregate(ordered, 0, 100, aggs)
    shuffle = np.r_[0, 1 + rng.permutation(n - 2), n - 1]          # (first and last row stay: the window plan is the ordered frame's)
    shuffled = [capi.Column(ts[shuffle], None, capi.INT64).to_device(), col_of(val[shuffle], valid[shuffle], capi.FLOAT64).to_device()]
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate(shuffled, 0, 100, aggs)
    assert e.value.code == -14
    outs, unchanged = capi.sort_by_col(shuffled, 0, out_residency=capi.DEVICE)
    assert not unchanged
    back = [capi.out_as_column(o) for o in outs]
    assert back[0].residency == capi.DEVICE and capi.is_col_sorted(back[0])
    got, _ = capi.rolling_aggregate(back, 0, 100, aggs)
    for (name, _c), g, w in zip(aggs, got, want):
        gv, gb = g.host_arrays()
        wv, wb = w.host_arrays()
        assert g.length == w.length and g.null_count == w.null_count and g.type == w.type, name
        assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)) and np.array_equal(gb, wb), name


# ------------------------------------------------------------------ full size
def test_full_size_1e8_rows_nothing_large_on_the_host():
    """gen_dense's ts[i] = i / val = f(seed, i) shuffled in HBM through take (a permutation uploaded once), sorted back by
    sort_by_col: the outputs must be the two generated buffers - position-dependent checksums and six million rows compared on the host"""
    n = 100_000_000
    need_gpu, need_host = 8 * n * 7 + 25 * n, 8 * n * 2.5
    if capi.mem_info()[0] < need_gpu:
        pytest.skip("GPU has %.1f GB free, %.1f GB needed" % (capi.mem_info()[0] / 1e9, need_gpu / 1e9))
    if psutil.virtual_memory().available < need_host:
        pytest.skip("host has %.1f GB available, %.1f GB needed for the permutation" % (psutil.virtual_memory().available / 1e9, need_host / 1e9))
    ts, val = capi.gen_dense(0, n, seed=11)
    perm = np.random.default_rng(11).permutation(n)                  # int64, 8e8 B: uploaded once
    d_perm = capi.DeviceBuffer.from_numpy(perm)
    want_first = perm[:1000].copy()
    del perm
    s_ts = capi.take(ts, d_perm, n, out_residency=capi.DEVICE)
    s_val = capi.take(val, d_perm, n, out_residency=capi.DEVICE)
    d_perm.free()
    assert s_ts.null_count == 0 and s_val.null_count == 0
    assert np.array_equal(s_ts.values.to_numpy(np.int64, 1000), want_first)       # ts[i] = i: the shuffled key IS the permutation
    want_ts, want_val = capi.checksum64(ts.values, n), capi.checksum64(val.values, n)
    assert capi.checksum64(s_ts.values, n) != want_ts
    outs, unchanged = capi.sort_by_col([capi.out_as_column(s_ts), capi.out_as_column(s_val)], 0, out_residency=capi.DEVICE)
    assert not unchanged
    print("sort_by_col 1e8 rows x 2 columns: %.2f ms on the device, %s" % (capi.last_kernel_ms(), capi.last_kernel_instance()))
    assert outs[0].null_count == 0 and outs[1].null_count == 0 and outs[0].length == n
    assert capi.checksum64(outs[0].values, n) == want_ts
    assert capi.checksum64(outs[1].values, n) == want_val
    nb = (n + 7) // 8
    for o in outs:
        bm = o.validity.to_numpy(np.uint8, nb)
        assert (bm == 0xFF).all()
    # D2H compare of six million rows: the middle and both ends
    got_ts, got_val = outs[0].values.to_numpy(np.int64, 4_000_000, 48_000_000), outs[1].values.to_numpy(np.uint64, 4_000_000, 48_000_000)
    assert np.array_equal(got_ts, np.arange(48_000_000, 52_000_000, dtype=np.int64))
    assert np.array_equal(got_val, val.values.to_numpy(np.uint64, 4_000_000, 48_000_000))
    for lo in (0, n - 1_000_000):
        assert np.array_equal(outs[0].values.to_numpy(np.int64, 1_000_000, lo), np.arange(lo, lo + 1_000_000, dtype=np.int64))
        assert np.array_equal(outs[1].values.to_numpy(np.uint64, 1_000_000, lo), val.values.to_numpy(np.uint64, 1_000_000, lo))


# ------------------------------------------------------------------ the C++ mirror's SortByCol
def test_cpp_mirror_replays_the_sort_tables():
    exe = os.path.join(ROOT, "tests", "cpp", "test_sort")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
