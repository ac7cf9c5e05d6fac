"""bowgpu_parquet_write on the device.  Every comparison is exact.  The independent reader is pyarrow; the page walk of
tests/parquet_page_walk.py shows the level and value bytes of every page, which are compared with what the header's contract says
they are (the definition-level forms; PLAIN; tests/parquet_pages.encode_delta(values, 128, 4), the unique DELTA_BINARY_PACKED bytes
under the contract's rules); the library's own loader reads every file back as well.  verify() does all three for every file any
test here writes."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import frame_model as fm
import parquet_page_walk as walk
import parquet_pages as pp
from bow_amd import capi
from test_parquet_loader import expect

pytestmark = pytest.mark.gpu

PLAIN, DELTA = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
RES = (capi.HOST, capi.HOST_PINNED, capi.DEVICE)


# ------------------------------------------------------------------ columns in memory
class Frame:
    """columns placed in memory for a call: [(name, values, valid)] as numpy, the capi Columns, and the registrations to undo"""

    def __init__(self):
        self.names, self.data, self.cols, self.pinned = [], [], [], []

    def add(self, name, values, valid, offset=0, res=capi.HOST, bitmap=True, known=False):
        """values: int64 / float64 array; valid: bool array or None (no bitmap).  The slice lies `offset` rows into longer buffers with
        junk values and stray validity bits around it."""
        values = np.ascontiguousarray(values)
        n, dt = len(values), values.dtype
        all_valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        buf = np.concatenate([np.full(offset, -77, dt), values, np.full(3, -78, dt)])
        if valid is not None and bitmap:
            bm = np.packbits(np.concatenate([np.arange(offset) % 2 == 0, all_valid, np.ones(5, bool)]), bitorder="little")
            nulls = int((~all_valid).sum()) if known else -1
        else:
            assert all_valid.all()
            bm, nulls = None, 0
        typ = capi.INT64 if dt == np.int64 else capi.FLOAT64
        if res == capi.HOST_PINNED:
            pv, pb = capi.page_aligned(len(buf), dt), None if bm is None else capi.page_aligned(len(bm), np.uint8)
            pv[:] = buf
            if bm is not None:
                pb[:] = bm
            c = capi.Column(pv, pb, typ, offset, n, nulls).pin()
            self.pinned.append(c)
        else:
            c = capi.Column(buf, bm, typ, offset, n, nulls)
            if res == capi.DEVICE:
                c = c.to_device()
        self.names.append(name)
        self.data.append((values, all_valid))
        self.cols.append(c)
        return self

    def release(self):
        for c in self.pinned:
            c.unpin()
        self.pinned = []


def write(path, fr, **kw):
    try:
        return capi.write_parquet(path, fr.cols, fr.names, **kw)
    finally:
        fr.release()


# ------------------------------------------------------------------ what a file must hold
def uleb(v):
    return pp._uleb(v)


def want_levels(valid):
    n, k = len(valid), int(valid.sum())
    if k == n or k == 0:
        return uleb(n << 1) + (b"\x01" if k else b"\x00")
    return uleb((((n + 7) // 8) << 1) | 1) + np.packbits(valid, bitorder="little").tobytes()


def verify(path, data, names, page_rows, rg_rows, encodings=None, info=None, statistics=True):
    """data: [(values, valid)] per column.  pyarrow's reading, the structure, every page's bytes, the library's loader."""
    ncols, n = len(data), len(data[0][0])
    encodings = encodings or [PLAIN] * ncols
    assert os.listdir(os.path.dirname(path)).count(os.path.basename(path) + ".tmp") == 0
    f = pq.ParquetFile(path)
    md = f.metadata
    groups = [(a, min(a + rg_rows, n)) for a in range(0, n, rg_rows)]
    assert md.num_rows == n and md.num_columns == ncols and md.num_row_groups == len(groups)
    assert [md.row_group(g).num_rows for g in range(len(groups))] == [b - a for a, b in groups]
    assert [md.schema.column(i).name for i in range(ncols)] == list(names)
    table = f.read()
    assert table.schema.names == list(names)
    npages = 0
    for i, (values, valid) in enumerate(data):
        sc = md.schema.column(i)
        assert sc.physical_type == ("INT64" if values.dtype == np.int64 else "DOUBLE") and sc.max_definition_level == 1   # OPTIONAL, whatever the nulls
        gv, gm = expect(table, names[i])
        assert np.array_equal(gm, valid), (names[i], np.flatnonzero(gm != valid)[:10])
        assert np.array_equal(np.asarray(gv).view(np.uint64)[valid], values.view(np.uint64)[valid]), names[i]
        for g, (a, b) in enumerate(groups):
            ch = md.row_group(g).column(i)
            assert ch.num_values == b - a and ch.compression == "UNCOMPRESSED"
            assert ("DELTA_BINARY_PACKED" if encodings[i] == DELTA else "PLAIN") in ch.encodings and "RLE" in ch.encodings
            assert ch.statistics.null_count == int((~valid[a:b]).sum())
            if not statistics:
                assert not ch.statistics.has_min_max
            pages = list(walk.pages(path, ch))
            assert [pg[0] for pg in pages] == [min(page_rows, b - r) for r in range(a, b, page_rows)]
            for pg, r in zip(pages, range(a, b, page_rows)):
                ok, v = valid[r:min(r + page_rows, b)], values[r:min(r + page_rows, b)]
                assert pg[1] == encodings[i]
                assert pg[2] == want_levels(ok), (names[i], g, r)
                assert pg[3] == (pp.encode_delta(v[ok], 128, 4) if encodings[i] == DELTA else pp.encode_plain(v[ok])), (names[i], g, r)
            npages += len(pages)
    if info is not None:
        assert (info.rows, info.row_groups, info.data_pages, info.file_bytes) == (n, len(groups), npages, os.path.getsize(path))
    # the library's own loader
    lf = capi.ParquetFile(path)
    assert lf.num_rows == n and [c[0] for c in lf.columns] == list(names) and all(c[2] for c in lf.columns)
    for i, (values, valid) in enumerate(data):
        if n:
            assert lf.check_column(i) == (capi.PARQUET_ENC_DELTA_BINARY_PACKED if encodings[i] == DELTA else capi.PARQUET_ENC_PLAIN)
        out = lf.read_column(i)
        assert out.length == n and out.null_count == int((~valid).sum())
        assert out.type == (capi.INT64 if values.dtype == np.int64 else capi.FLOAT64)
        assert np.array_equal(out.valid_mask(), valid)
        assert np.array_equal(out.host_arrays()[0].view(np.uint64)[valid], values.view(np.uint64)[valid])
    lf.close()
    return md


# ------------------------------------------------------------------ values and validity shapes
def int_values(n, rng):
    x = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    sp = np.array([I64_MIN, I64_MAX, 0, -1, 1], dtype=np.int64)
    at = rng.choice(n, min(n, len(sp)), replace=False) if n else np.zeros(0, int)
    x[at] = sp[:len(at)]
    return x


def float_values(n, rng):
    x = rng.standard_normal(n)
    sp = np.array([0x7ff8000000000000, 0xfff8dead0000beef, 0, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 1], dtype=np.uint64)
    at = rng.choice(n, min(n, len(sp)), replace=False) if n else np.zeros(0, int)
    x.view(np.uint64)[at] = sp[:len(at)]
    return x


VALIDITY = ("none", "all", "allnull", "p30", "one", "hole")


def validity(kind, n, page, rng):
    if kind == "none":
        return None
    if kind == "all":
        return np.ones(n, bool)
    if kind == "allnull":
        return np.zeros(n, bool)
    if kind == "one":   # exactly one valid row per page
        v = np.zeros(n, bool)
        for p, r in enumerate(range(0, n, page)):
            v[r + (p * 7) % min(page, n - r)] = True
        return v
    v = rng.random(n) >= 0.3
    if kind == "hole":   # an all-null page between two mixed ones
        v[page:2 * page] = False
    return v


# ------------------------------------------------------------------ 1. PLAIN, structure (and 2, 5 through verify)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 200, 385])
def test_plain_structure(tmp_path, n):
    rng = np.random.default_rng(100 + n)
    for oi, offset in enumerate((0, 3, 8, 13)):
        fr = Frame()
        for vi, kind in enumerate(VALIDITY):
            for ti, gen in enumerate((int_values, float_values)):
                res = RES[(vi + ti + oi) % 3]   # every (validity, type) meets every residency over the offsets
                fr.add("%s_%s" % (kind, "if"[ti]), gen(n, rng), validity(kind, n, 64, rng), offset=offset, res=res, known=bool((vi + oi) % 2))
        path = str(tmp_path / ("plain_%d_%d.parquet" % (n, offset)))
        info = write(path, fr, page_rows=64, row_group_rows=128)
        md = verify(path, fr.data, fr.names, 64, 128, info=info)
        assert md.num_row_groups == -(-n // 128)


# ------------------------------------------------------------------ 2. levels
@pytest.mark.parametrize("offset", [0, 3, 13])
def test_level_forms_at_bit_offsets(tmp_path, offset):
    rng = np.random.default_rng(7)
    n = 64 * 4 + 37
    valid = rng.random(n) >= 0.4
    valid[0:64] = True      # page 0: one run of 1
    valid[64:128] = False   # page 1: one run of 0
    fr = Frame()
    for res in RES:
        fr.add("c%d" % res, int_values(n, rng), valid, offset=offset, res=res)
    path = str(tmp_path / "levels.parquet")
    write(path, fr, page_rows=64, row_group_rows=192)
    md = verify(path, fr.data, fr.names, 64, 192)
    for i in range(3):
        pages = list(walk.pages(path, md.row_group(0).column(i))) + list(walk.pages(path, md.row_group(1).column(i)))
        assert pages[0][2] == bytes([128, 1, 1]) and pages[1][2] == bytes([128, 1, 0])
        for p in range(2, 5):
            ok = valid[64 * p:64 * p + 64]
            assert 0 < ok.sum() < len(ok)
            assert pages[p][2][1:] == np.packbits(ok, bitorder="little").tobytes()   # behind the run header: the page's bits from bit 0


# ------------------------------------------------------------------ 3. DELTA bytes
def delta_shapes(n, rng):
    return {"constant": np.full(n, 1234567, dtype=np.int64),
            "arange": np.arange(n, dtype=np.int64) * 1000 + 5,                                         # width 0
            "timestamps": np.cumsum(rng.integers(1, 20, n) * rng.choice([1, 1, 1, 10 ** 6], n)).astype(np.int64),   # ascending, with gaps
            "full_range": rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64),                           # wrapping differences, width 64
            "alternating": np.tile(np.array([I64_MIN, I64_MAX], dtype=np.int64), n // 2 + 1)[:n],
            "descending": (10 ** 15 - np.cumsum(rng.integers(1, 5000, n))).astype(np.int64)}


@pytest.mark.parametrize("shape", ["constant", "arange", "timestamps", "full_range", "alternating", "descending"])
def test_delta_bytes_at_block_and_miniblock_edges(tmp_path, shape):
    """one page per count of non-null values: 0, 1, 2, 33, 34 (a miniblock's edge), 129, 130 (a block's), 257, 258, a page without a
    null, and a short last page without one"""
    rng = np.random.default_rng(11)
    page = 512
    counts = [0, 1, 2, 33, 34, 129, 130, 257, 258, page, page - 100]
    n = page * len(counts) - 100
    valid = np.zeros(n, bool)
    for p, k in enumerate(counts):
        rows = min(page, n - p * page)
        valid[p * page + np.sort(rng.choice(rows, k, replace=False))] = True
    values = np.zeros(n, dtype=np.int64)
    values[valid] = delta_shapes(int(valid.sum()), rng)[shape]
    values[~valid] = rng.integers(I64_MIN, I64_MAX, int((~valid).sum()), dtype=np.int64)   # (what lies under a null is not written)
    for res, offset in ((capi.DEVICE, 0), (capi.HOST, 5)):
        fr = Frame().add("ts", values, valid, offset=offset, res=res)
        path = str(tmp_path / ("delta_%s_%d.parquet" % (shape, res)))
        info = write(path, fr, page_rows=page, row_group_rows=page * 4, encodings=[DELTA])
        md = verify(path, fr.data, fr.names, page, page * 4, encodings=[DELTA], info=info)
        assert all("DELTA_BINARY_PACKED" in md.row_group(g).column(0).encodings for g in range(md.num_row_groups))
        got = pq.read_table(path).column(0).combine_chunks()
        assert np.array_equal(np.asarray(got.fill_null(0))[valid], values[valid])


def test_delta_without_nulls_and_next_to_a_plain_column(tmp_path):
    rng = np.random.default_rng(12)
    n = 3000
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], None, res=capi.DEVICE)
    fr.add("v", float_values(n, rng), rng.random(n) >= 0.3, offset=3, res=capi.DEVICE)
    fr.add("full", delta_shapes(n, rng)["full_range"], np.ones(n, bool), offset=9, res=capi.HOST)
    enc = [DELTA, PLAIN, DELTA]
    path = str(tmp_path / "mixed.parquet")
    info = write(path, fr, page_rows=512, row_group_rows=1024, encodings=enc)
    verify(path, fr.data, fr.names, 512, 1024, encodings=enc, info=info)


# ------------------------------------------------------------------ 4. statistics
def stats_of(path, g=0):
    md = pq.read_metadata(path)
    return [md.row_group(g).column(i).statistics for i in range(md.num_columns)]


def test_statistics_equal_pyarrows_own(tmp_path):
    nan = float("nan")
    rng = np.random.default_rng(13)
    big = rng.standard_normal(700)
    big[rng.choice(700, 50, replace=False)] = nan
    cases = {"with_nan": (np.array([3.5, nan, -2.25, nan, 7.0]), None),
             "all_nan": (np.array([nan, nan, nan]), None),
             "all_null": (np.array([1.0, 2.0]), np.zeros(2, bool)),
             "only_pz": (np.array([0.0, 0.0]), None),
             "only_nz": (np.array([-0.0, -0.0, -0.0]), None),
             "both_zeroes": (np.array([-0.0, 0.0, -5.0]), np.array([True, True, False])),
             "infs": (np.array([np.inf, 1.0, -np.inf, nan]), None),
             "nan_under_null": (np.array([nan, 4.0, -9.0]), np.array([False, True, False])),
             "many": (big, rng.random(700) >= 0.3),
             "int_nulls": (np.array([5, I64_MIN, -3, I64_MAX, 9], dtype=np.int64), np.array([True, False, True, False, True])),
             "int_extremes": (np.array([I64_MAX, 0, I64_MIN], dtype=np.int64), None),
             "int_many": (rng.integers(I64_MIN, I64_MAX, 700, dtype=np.int64), rng.random(700) >= 0.5)}
    for k, (name, (values, valid)) in enumerate(cases.items()):
        ok = np.ones(len(values), bool) if valid is None else valid
        ref = str(tmp_path / ("ref_%s.parquet" % name))
        pq.write_table(pa.table({name: pa.array(values, mask=~ok)}), ref, compression="none", use_dictionary=False)
        want = stats_of(ref)[0]
        fr = Frame().add(name, values, valid, offset=k % 4, res=RES[k % 3])
        path = str(tmp_path / ("stats_%s.parquet" % name))
        enc = [DELTA if values.dtype == np.int64 and k % 2 else PLAIN]
        write(path, fr, page_rows=64, row_group_rows=1024, encodings=enc)
        verify(path, fr.data, fr.names, 64, 1024, encodings=enc)
        got = stats_of(path)[0]
        assert got.has_null_count and got.null_count == want.null_count, name
        assert got.has_min_max == want.has_min_max, name
        if want.has_min_max:
            assert got.min == want.min and got.max == want.max, (name, got.min, got.max, want.min, want.max)
            if values.dtype == np.float64:
                assert np.signbit(got.min) == np.signbit(want.min) and np.signbit(got.max) == np.signbit(want.max), name
        # and with statistics = 0: the null count alone
        fr = Frame().add(name, values, valid)
        write(path, fr, page_rows=64, row_group_rows=1024, statistics=False)
        verify(path, fr.data, fr.names, 64, 1024, statistics=False)
        got = stats_of(path)[0]
        assert not got.has_min_max and got.null_count == want.null_count, name


def test_statistics_are_per_column_chunk(tmp_path):
    rng = np.random.default_rng(14)
    n = 1000
    v, ok = float_values(n, rng), rng.random(n) >= 0.2
    fr = Frame().add("v", v, ok, offset=5, res=capi.DEVICE)
    path = str(tmp_path / "chunks.parquet")
    write(path, fr, page_rows=64, row_group_rows=256)
    verify(path, fr.data, fr.names, 64, 256)
    for g, a in enumerate(range(0, n, 256)):
        x = v[a:a + 256][ok[a:a + 256]]
        x = x[~np.isnan(x)]
        st = stats_of(path, g)[0]
        assert st.has_min_max and st.min == x.min() and st.max == x.max() and st.null_count == int((~ok[a:a + 256]).sum())


# ------------------------------------------------------------------ 6. a device-resident chain
def test_drop_nils_sort_write_without_leaving_the_device(tmp_path):
    rng = np.random.default_rng(15)
    n = 3000
    M = fm.Model()
    frame = [fm.mcol(rng.permutation(n).astype(np.int64) * 7 - 1000, rng.random(n) >= 0.2),
             fm.mcol(rng.standard_normal(n), rng.random(n) >= 0.3),
             fm.mcol(rng.integers(-50, 50, n).astype(np.int64), rng.random(n) >= 0.1)]
    cols = [capi.Column(fm.vals(c).copy(), np.packbits(c.valid, bitorder="little"), c.typ, 0, n, -1).to_device() for c in frame]
    outs, first, count, contiguous = capi.drop_nils(cols, [0], out_residency=capi.DEVICE)
    want = M.drop_nils(frame, [0])
    assert not contiguous and not want.contiguous and count == want.count
    kept = [capi.out_as_column(o) for o in outs]
    assert all(c.residency == capi.DEVICE for c in kept)
    outs2, unchanged = capi.sort_by_col(kept, 0, out_residency=capi.DEVICE)
    want2 = M.sort_by_col(want.cols, 0)
    assert not unchanged and not want2.unchanged
    srt = [capi.out_as_column(o) for o in outs2]
    assert all(c.residency == capi.DEVICE for c in srt)
    names = ["key", "v", "i"]
    enc = [DELTA, PLAIN, DELTA]
    path = str(tmp_path / "chain.parquet")
    info = capi.write_parquet(path, srt, names, page_rows=128, row_group_rows=1024, encodings=enc)
    data = [(fm.vals(c), c.valid) for c in want2.cols]
    verify(path, data, names, 128, 1024, encodings=enc, info=info)
    assert info.rows == count


# ------------------------------------------------------------------ 7. metadata
def test_metadata_names_and_no_temporary(tmp_path):
    rng = np.random.default_rng(16)
    names = ["time", "a column with spaces", "ünï", "x" * 200]
    fr = Frame()
    for k, nm in enumerate(names):
        fr.add(nm, int_values(50, rng) if k % 2 else float_values(50, rng), rng.random(50) >= 0.3)
    meta = {"bow_meta": "{\"k\": [1, 2, 3]}", "empty": "", "ünï": "ключ"}
    path = str(tmp_path / "meta.parquet")
    info = write(path, fr, metadata=meta)   # every other option at its default: one page, one row group
    md = verify(path, fr.data, fr.names, 65536, 1 << 24, info=info)
    assert md.metadata == {k.encode(): v.encode() for k, v in meta.items()}
    assert md.created_by.startswith("bowgpu") and md.format_version == "1.0"
    assert os.listdir(str(tmp_path)) == ["meta.parquet"]
    # without pairs: no key_value_metadata at all
    fr = Frame().add("c", int_values(5, rng), None)
    write(path, fr)
    assert pq.read_metadata(path).metadata is None
    assert os.listdir(str(tmp_path)) == ["meta.parquet"]


def test_failure_to_create_the_file_is_an_argument_error(tmp_path):
    fr = Frame().add("c", np.arange(10, dtype=np.int64), None)
    with pytest.raises(capi.BowGpuError) as e:
        write(str(tmp_path / "no_such_directory" / "x.parquet"), fr)
    assert e.value.code == -10 and "No such file or directory" in e.value.message
    assert os.listdir(str(tmp_path)) == []


# ------------------------------------------------------------------ 8. fuzz
SEEDS = int(os.environ.get("BOW_FUZZ_SEEDS", "64"))


def fuzz_frame(seed):
    rng = np.random.default_rng(1000 + seed)
    ncols = int(rng.integers(1, 5))
    n = int(rng.choice([0, 1, int(rng.integers(2, 200)), int(rng.integers(200, 5001))], p=[0.03, 0.03, 0.34, 0.6]))
    page = int(rng.choice([64, 128, 512]))
    rg = page * int(rng.integers(1, 9))
    fr, enc = Frame(), []
    for i in range(ncols):
        is_int = bool(rng.integers(0, 2))
        density = float(rng.choice([0.0, 0.05, 0.5, 0.95, 1.0]))
        kind = rng.choice(["none", "bitmap"], p=[0.2, 0.8])
        valid = None if kind == "none" else rng.random(n) < density
        if valid is not None and n > 2 * page and rng.random() < 0.5:   # whole pages of one kind among the mixed ones
            p = int(rng.integers(0, n // page))
            valid[p * page:(p + 1) * page] = bool(rng.integers(0, 2))
        if is_int:
            shape = rng.choice(["constant", "arange", "timestamps", "full_range", "alternating", "descending"])
            values = delta_shapes(n, rng)[shape]
        else:
            values = float_values(n, rng)
        enc.append(DELTA if is_int and rng.random() < 0.6 else PLAIN)
        fr.add("c%d" % i, values, valid, offset=int(rng.integers(0, 70)), res=RES[int(rng.integers(0, 3))], known=bool(rng.integers(0, 2)))
    return fr, enc, page, rg


def test_fuzz_against_pyarrow_and_the_loader(tmp_path):
    ran = 0
    for seed in range(SEEDS):
        fr, enc, page, rg = fuzz_frame(seed)
        path = str(tmp_path / ("fuzz%d.parquet" % seed))
        info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, statistics=bool(seed % 2))
        verify(path, fr.data, fr.names, page, rg, encodings=enc, info=info, statistics=bool(seed % 2))
        os.remove(path)
        ran += 1
    assert ran == SEEDS


# ------------------------------------------------------------------ 9. determinism
def test_the_same_call_twice_gives_identical_files(tmp_path):
    rng = np.random.default_rng(17)
    n = 4000
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], rng.random(n) >= 0.1, offset=3, res=capi.DEVICE)
    fr.add("full", delta_shapes(n, rng)["full_range"], rng.random(n) >= 0.5, offset=11, res=capi.DEVICE)
    fr.add("v", float_values(n, rng), rng.random(n) >= 0.3, offset=6, res=capi.HOST)
    enc = [DELTA, DELTA, PLAIN]
    files = []
    for k in range(2):
        path = str(tmp_path / ("twice%d.parquet" % k))
        capi.write_parquet(path, fr.cols, fr.names, page_rows=128, row_group_rows=1024, encodings=enc, metadata={"k": "v"})
        files.append(open(path, "rb").read())
    assert files[0] == files[1]
    verify(str(tmp_path / "twice1.parquet"), fr.data, fr.names, 128, 1024, encodings=enc)
