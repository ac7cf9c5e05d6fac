"""bowgpu_parquet_write_bool on the device: a bit-packed Boolean column written as a Parquet BOOLEAN column.  Every comparison is
exact.  verify() runs for every file a test here writes: pyarrow reads the values and the mask; the page walk
(tests/parquet_page_walk.py, under SNAPPY tests/parquet_snappy_walk.py) shows every page's level bytes and value bytes, which must
be the definition-level forms of the contract and np.packbits(values[valid], bitorder="little") (tests/parquet_bool_pages.plain_bits:
padding bits 0); the statistics equal those pyarrow writes for the same table; the library's own loader reads the column back bit
for bit (null rows' value bits 0, the exact null count) and its check says PLAIN."""
import filecmp
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_bool_pages as pb
import parquet_page_walk as walk
import parquet_pages as pp
import parquet_snappy_walk as swalk
from bow_amd import capi
from test_gpu_parquet_bool import assert_column
from test_gpu_parquet_write import delta_shapes, float_values, int_values, want_levels
from test_parquet_loader import expect

pytestmark = pytest.mark.gpu

PLAIN, DELTA, DICT = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_RLE_DICTIONARY
RES = (capi.HOST, capi.HOST_PINNED, capi.DEVICE)
OFFSETS = (0, 1, 7, 8, 31, 33, 63, 65)
TYPE_NAMES = {np.dtype(bool): "BOOLEAN", np.dtype(np.int64): "INT64", np.dtype(np.float64): "DOUBLE"}


# ------------------------------------------------------------------ columns in memory
class Frame:
    """columns placed in memory for a call: [(values, valid)] per column as numpy (bool values: a Boolean column), the capi Columns,
    and the registrations to undo"""

    def __init__(self, seed=0):
        self.names, self.data, self.cols, self.pinned = [], [], [], []
        self.rng = np.random.default_rng(9000 + seed)

    def _place(self, vbuf, bm, typ, offset, n, nulls, res):
        if res == capi.HOST_PINNED:
            pv, pbm = capi.page_aligned(len(vbuf), vbuf.dtype), None if bm is None else capi.page_aligned(len(bm), np.uint8)
            pv[:] = vbuf
            if bm is not None:
                pbm[:] = bm
            c = capi.Column(pv, pbm, typ, offset, n, nulls).pin()
            self.pinned.append(c)
            return c
        c = capi.Column(vbuf, bm, typ, offset, n, nulls)
        return c.to_device() if res == capi.DEVICE else c

    def add(self, name, values, valid, offset=0, res=capi.HOST, known=False, odd_address=False):
        """values: bool (a Boolean column, bit-packed here), int64 or float64 array; valid: bool array or None (no bitmap).  The
        slice lies `offset` rows into longer buffers: a Boolean column has random value bits under its nulls and stray bits in front
        of and behind the slice, in values and validity; odd_address: its host buffers begin at an odd byte address."""
        values = np.ascontiguousarray(values)
        n = len(values)
        all_valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        nulls = 0 if valid is None else int((~all_valid).sum()) if known else -1
        bm = None
        if valid is not None:
            bm = np.packbits(np.concatenate([self.rng.random(offset) < 0.5, all_valid, np.ones(5, bool)]), bitorder="little")
        if values.dtype == bool:
            under = np.where(all_valid, values, self.rng.random(n) < 0.5)
            vbuf = np.packbits(np.concatenate([self.rng.random(offset) < 0.5, under, self.rng.random(11) < 0.5]), bitorder="little")
            if odd_address:
                vbuf = np.concatenate([np.zeros(1, np.uint8), vbuf])[1:]
                bm = None if bm is None else np.concatenate([np.zeros(3, np.uint8), bm])[3:]
            typ = capi.BOOLEAN
        else:
            vbuf = np.concatenate([np.full(offset, -77, values.dtype), values, np.full(3, -78, values.dtype)])
            typ = capi.INT64 if values.dtype == np.int64 else capi.FLOAT64
        self.names.append(name)
        self.data.append((values, all_valid))
        self.cols.append(self._place(vbuf, bm, typ, offset, n, nulls, res))
        return self

    def release(self):
        for c in self.pinned:
            c.unpin()
        self.pinned = []


def write(path, fr, **kw):
    try:
        return capi.write_parquet(path, fr.cols, fr.names, booleans=True, **kw)
    finally:
        fr.release()


# ------------------------------------------------------------------ what a file must hold
def pyarrow_bool_stats(tmp, data, names, rg_rows):
    """{column: [Statistics per row group]} as pyarrow writes them for the Boolean columns of the same table"""
    cols = {names[i]: pa.array(v, mask=~ok) for i, (v, ok) in enumerate(data) if v.dtype == bool}
    if not cols or not len(data[0][0]):
        return {}
    ref = os.path.join(tmp, "pyarrow_ref.parquet")
    pq.write_table(pa.table(cols), ref, use_dictionary=False, compression="none", row_group_size=rg_rows)
    md = pq.read_metadata(ref)
    return {nm: [md.row_group(g).column(k).statistics for g in range(md.num_row_groups)] for k, nm in enumerate(cols)}


def want_section(values, ok, encoding):
    if values.dtype == bool:
        return pb.plain_bits(values[ok])
    return pp.encode_delta(values[ok], 128, 4) if encoding == DELTA else pp.encode_plain(values[ok])


def verify(path, data, names, page_rows, rg_rows, encodings=None, info=None, statistics=True, codec=0):
    """data: [(values, valid)] per column"""
    ncols, n = len(data), len(data[0][0])
    encodings = encodings or [PLAIN] * ncols
    tmp = os.path.dirname(path)
    assert os.listdir(tmp).count(os.path.basename(path) + ".tmp") == 0
    f = pq.ParquetFile(path)
    md = f.metadata
    groups = [(a, min(a + rg_rows, n)) for a in range(0, n, rg_rows)]
    assert md.num_rows == n and md.num_columns == ncols and md.num_row_groups == len(groups)
    assert [md.row_group(g).num_rows for g in range(len(groups))] == [b - a for a, b in groups]
    assert [md.schema.column(i).name for i in range(ncols)] == list(names)
    table = f.read()
    ref_stats = pyarrow_bool_stats(tmp, data, names, rg_rows)
    npages = value_bytes = 0
    for i, (values, valid) in enumerate(data):
        is_bool = values.dtype == bool
        sc = md.schema.column(i)
        assert sc.physical_type == TYPE_NAMES[values.dtype] and sc.max_definition_level == 1 and sc.max_repetition_level == 0, names[i]
        if is_bool:
            assert table.schema.field(i).type == pa.bool_()
            col = table.column(i).combine_chunks()
            gm = ~np.asarray(col.is_null())
            gv = np.asarray(col.fill_null(False)).astype(bool)
            assert np.array_equal(gm, valid), (names[i], np.flatnonzero(gm != valid)[:10])
            assert np.array_equal(gv, values & valid), (names[i], np.flatnonzero(gv != (values & valid))[:10])
        else:
            gv, gm = expect(table, names[i])
            assert np.array_equal(gm, valid), names[i]
            assert np.array_equal(np.asarray(gv).view(np.uint64)[valid], values.view(np.uint64)[valid]), names[i]
        for g, (a, b) in enumerate(groups):
            ch = md.row_group(g).column(i)
            assert ch.num_values == b - a and ch.compression == ("SNAPPY" if codec else "UNCOMPRESSED")
            st = ch.statistics
            assert st.has_null_count and st.null_count == int((~valid[a:b]).sum())
            if not statistics:
                assert not st.has_min_max
            if is_bool:
                assert set(ch.encodings) == {"PLAIN", "RLE"}
                want = ref_stats[names[i]][g]
                assert st.null_count == want.null_count
                assert st.has_min_max == (want.has_min_max and statistics), (names[i], g)
                if st.has_min_max:
                    assert (st.min, st.max) == (want.min, want.max), (names[i], g, st.min, st.max, want.min, want.max)
            rows = [min(page_rows, b - r) for r in range(a, b, page_rows)]
            npages += len(rows)
            if encodings[i] == DICT:   # (its pages are tests/test_gpu_parquet_dictionary.py's business: pyarrow and the loader read them here)
                value_bytes = None
                continue
            pages = list(swalk.pages(path, ch)) if codec else list(walk.pages(path, ch))
            assert [pg[0] for pg in pages] == rows, (names[i], g)
            for pg, r in zip(pages, range(a, b, page_rows)):
                ok, v = valid[r:min(r + page_rows, b)], values[r:min(r + page_rows, b)]
                assert pg[1] == encodings[i]
                assert pg[2] == want_levels(ok), (names[i], g, r)
                assert pg[3] == want_section(v, ok, encodings[i]), (names[i], g, r, int(ok.sum()))
                if value_bytes is not None:
                    value_bytes += len(pg[3])
    if info is not None:
        assert (info.rows, info.row_groups, info.data_pages, info.file_bytes) == (n, len(groups), npages, os.path.getsize(path))
        if value_bytes is not None:
            assert info.value_bytes == value_bytes
    # the library's own loader
    lf = capi.ParquetFile(path)
    assert lf.num_rows == n and [c[0] for c in lf.columns] == list(names) and all(c[2] for c in lf.columns)
    for i, (values, valid) in enumerate(data):
        if values.dtype == bool:
            assert lf.columns[i][1] == capi.BOOLEAN
            if n:
                assert lf.check_bool_column(i) == capi.PARQUET_ENC_PLAIN
            assert_column(names[i], lf.read_bool_column(i), values, valid)
        else:
            out = lf.read_column(i)
            assert out.length == n and out.null_count == int((~valid).sum())
            assert np.array_equal(out.valid_mask(), valid)
            assert np.array_equal(out.host_arrays()[0].view(np.uint64)[valid], values.view(np.uint64)[valid])
    lf.close()
    return md


# ------------------------------------------------------------------ validity shapes
VALIDITY = ("none", "all", "allnull", "p30", "first", "last", "mid", "hole")


def validity(kind, n, page, rng):
    if kind == "none":
        return None
    if kind == "all":
        return np.ones(n, bool)
    v = np.zeros(n, bool)
    if kind == "allnull" or n == 0:
        return v
    if kind == "first":    # exactly one valid row in the column: the first row, the last row, the middle of its page
        v[0] = True
    elif kind == "last":
        v[n - 1] = True
    elif kind == "mid":
        r0 = (n - 1) // page * page
        v[r0 + (n - r0) // 2] = True
    else:
        v = rng.random(n) >= 0.3
        if kind == "hole":   # a whole null page between mixed ones
            v[page:2 * page] = False
    return v


# ------------------------------------------------------------------ 1. row counts, page sizes, validity shapes, residencies
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 129, 327, 1000])
def test_row_counts_validity_shapes_and_residencies(tmp_path, n):
    rng = np.random.default_rng(200 + n)
    for k, (page, rg) in enumerate(((64, 128), (128, 256))):
        fr = Frame(n + k)
        for vi, kind in enumerate(VALIDITY):
            fr.add("%s" % kind, rng.random(n) < 0.5, validity(kind, n, page, rng), offset=OFFSETS[(vi + 3 * k) % 8], res=RES[(vi + k) % 3],
                   known=bool((vi + k) % 2), odd_address=bool(vi % 2))
        path = str(tmp_path / ("rows_%d_%d.parquet" % (n, page)))
        info = write(path, fr, page_rows=page, row_group_rows=rg, codec=k)
        md = verify(path, fr.data, fr.names, page, rg, info=info, codec=k)
        assert md.num_row_groups == -(-n // rg)


# ------------------------------------------------------------------ 2. Arrow offsets; what lies under a null never reaches the file
@pytest.mark.parametrize("offset", OFFSETS)
def test_bit_offsets_and_junk_under_nulls(tmp_path, offset):
    rng = np.random.default_rng(300 + offset)
    n = 327
    flags, valid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    files = []
    for k in range(2):   # the same rows twice: other junk bits, another residency order
        fr = Frame(100 * k + offset)
        for j in range(3):
            fr.add("c%d" % j, flags, valid, offset=offset, res=RES[(j + k) % 3], known=bool(k), odd_address=bool(k))
        fr.add("nobitmap", flags, None, offset=offset, res=RES[k])
        path = str(tmp_path / ("offset_%d.parquet" % k))
        info = write(path, fr, page_rows=64, row_group_rows=128)
        verify(path, fr.data, fr.names, 64, 128, info=info)
        files.append(path)
    assert filecmp.cmp(files[0], files[1], shallow=False)   # every byte is a function of the rows alone


# ------------------------------------------------------------------ 3. pages of k = 1, 7, 8, 9, 63, 64 valid rows
@pytest.mark.parametrize("page", [64, 128])
def test_valid_counts_at_the_byte_and_word_edges(tmp_path, page):
    rng = np.random.default_rng(400 + page)
    ks = [1, 7, 8, 9, 63, 64, 0, 65 if page > 64 else 64]
    n = page * len(ks) - 30
    valid = np.zeros(n, bool)
    for p, k in enumerate(ks):
        rows = min(page, n - p * page)
        valid[p * page + np.sort(rng.choice(rows, min(k, rows), replace=False))] = True
    for codec in (0, 1):
        fr = Frame(page + codec)
        for j, flags in enumerate((rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool))):
            fr.add("f%d" % j, flags, valid, offset=OFFSETS[2 * j + 1], res=RES[(j + codec) % 3])
        path = str(tmp_path / ("k_%d.parquet" % codec))
        info = write(path, fr, page_rows=page, row_group_rows=2 * page, codec=codec)
        verify(path, fr.data, fr.names, page, 2 * page, info=info, codec=codec)


# ------------------------------------------------------------------ 4. a page longer than one trip of the workgroup
def test_page_longer_than_a_trip_carries_its_bit_position(tmp_path):
    rng = np.random.default_rng(500)
    n, page = 70_001, 32768   # a workgroup takes 16384 rows a trip: two trips a page, the second starts mid-word
    flags, valid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    dense = valid.copy()
    dense[page:page + 16384] = True   # a trip without a null in front of a mixed one
    for codec in (0, 1):
        fr = Frame(codec)
        fr.add("dev", flags, valid, offset=5, res=capi.DEVICE)
        fr.add("host", flags, dense, offset=33, res=capi.HOST, known=True)
        fr.add("nobitmap", flags, None, offset=7, res=capi.DEVICE)
        path = str(tmp_path / ("long_%d.parquet" % codec))
        info = write(path, fr, page_rows=page, row_group_rows=2 * page, codec=codec)
        verify(path, fr.data, fr.names, page, 2 * page, info=info, codec=codec)


# ------------------------------------------------------------------ 5. next to Int64 / Float64 columns and their encodings
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("statistics", [True, False])
def test_mixed_frame(tmp_path, codec, statistics):
    rng = np.random.default_rng(600)
    n = 3000
    fr = Frame(codec)
    fr.add("ts", delta_shapes(n, rng)["timestamps"], rng.random(n) >= 0.1, offset=3, res=capi.DEVICE)
    fr.add("flag", rng.random(n) < 0.4, rng.random(n) >= 0.3, offset=9, res=capi.DEVICE)
    fr.add("v", np.round(rng.standard_normal(n), 1), rng.random(n) >= 0.3, offset=6, res=capi.HOST)
    fr.add("all_true", np.ones(n, bool), rng.random(n) >= 0.5, offset=1, res=capi.HOST_PINNED, known=True)
    enc = [DELTA, PLAIN, DICT, PLAIN]
    path = str(tmp_path / "mixed.parquet")
    info = write(path, fr, page_rows=512, row_group_rows=1024, encodings=enc, codec=codec, statistics=statistics, metadata={"k": "v"})
    md = verify(path, fr.data, fr.names, 512, 1024, encodings=enc, info=info, codec=codec, statistics=statistics)
    assert md.metadata == {b"k": b"v"}
    assert all("RLE_DICTIONARY" in md.row_group(g).column(2).encodings for g in range(md.num_row_groups))
    if statistics:   # a chunk whose valid rows are all true: min = max = true
        st = md.row_group(0).column(3).statistics
        assert st.min is True and st.max is True


def test_frame_without_a_boolean_column_is_the_codec_entry_points_file(tmp_path):
    rng = np.random.default_rng(700)
    n = 2000
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], rng.random(n) >= 0.1, offset=3, res=capi.DEVICE)
    fr.add("v", float_values(n, rng), rng.random(n) >= 0.3, offset=6, res=capi.HOST)
    fr.add("i", int_values(n, rng), None, res=capi.DEVICE)
    enc = [DELTA, DICT, PLAIN]
    for codec in (0, 1):
        a, b = str(tmp_path / ("bool_%d.parquet" % codec)), str(tmp_path / ("codec_%d.parquet" % codec))
        kw = dict(page_rows=128, row_group_rows=512, encodings=enc, codec=codec, metadata={"k": "v"})
        ia = capi.write_parquet(a, fr.cols, fr.names, booleans=True, **kw)
        ib = capi.write_parquet(b, fr.cols, fr.names, **kw)
        assert filecmp.cmp(a, b, shallow=False)
        assert (ia.file_bytes, ia.data_pages, ia.level_bytes, ia.value_bytes) == (ib.file_bytes, ib.data_pages, ib.level_bytes, ib.value_bytes)
        verify(a, fr.data, fr.names, 128, 512, encodings=enc, info=ia, codec=codec)


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("kind", ["none", "allnull", "p30"])
def test_every_route_through_one_hand_over_at_its_edges(tmp_path, kind, codec):
    """DELTA, RLE_DICTIONARY, PLAIN and Boolean chunks in one call; the second row group is one page of 2 rows.  allnull: no
    values image on any route, no Snappy fragment, and the dictionary request comes out PLAIN; none: no levels image comes back."""
    rng = np.random.default_rng(650)
    n, page, rg = 130, 64, 128
    fr = Frame(codec)
    columns = (delta_shapes(n, rng)["timestamps"], np.round(rng.standard_normal(n), 1), int_values(n, rng), rng.random(n) < 0.5)
    for name, values, offset in zip(("delta", "dict", "plain", "flag"), columns, (0, 3, 9, 1)):
        fr.add(name, values, validity(kind, n, page, rng), offset=offset, res=capi.DEVICE)
    enc = [DELTA, DICT, PLAIN, PLAIN]
    path = str(tmp_path / "routes.parquet")
    info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, codec=codec)
    # (a dictionary chunk without a value is a PLAIN chunk: verify walks its pages too)
    md = verify(path, fr.data, fr.names, page, rg, encodings=[DELTA, PLAIN, PLAIN, PLAIN] if kind == "allnull" else enc, info=info, codec=codec)
    assert md.num_row_groups == 2 and md.row_group(1).num_rows == 2
    has_value = [bool(fr.data[1][1][a:a + rg].any()) for a in (0, rg)]   # a chunk has a dictionary exactly when it has a value
    assert [("RLE_DICTIONARY" in md.row_group(g).column(1).encodings) for g in range(2)] == has_value


# ------------------------------------------------------------------ 6. parquet -> Boolean reducer -> parquet, in HBM throughout
def test_flag_column_in_reduced_and_out_again_without_leaving_the_device(tmp_path):
    from oracle import pyoracle as orc
    rng = np.random.default_rng(800)
    n = 20_000
    src = str(tmp_path / "in.parquet")
    pb.write_pyarrow(src, rng.random(n) < 0.4, rng.random(n) >= 0.3, "plain_v1", extra={"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64))})
    f = capi.ParquetFile(src)
    ts = f.read_column(0, out_residency=capi.DEVICE)
    flag = f.read_bool_column(1, out_residency=capi.DEVICE)
    f.close()
    cols = [capi.Column(ts.values, None, capi.INT64, 0, n, 0), capi.Column(flag.values, flag.validity, capi.BOOLEAN, 0, n, flag.null_count)]
    aggs = [("WindowStart", 0), ("Last", 1)]
    got, _ = capi.rolling_aggregate(cols, 0, 50, aggs, out_residency=capi.DEVICE)
    assert got[1].type == capi.BOOLEAN and got[1].residency == capi.DEVICE
    tv = np.asarray(pq.read_table(src).column("ts")).astype(np.int64)
    vals, valid = pb.read_back(src, "flag")
    ocols = [orc.Column(tv, None, orc.INT64), orc.Column(np.packbits(vals, bitorder="little"), np.packbits(valid, bitorder="little"), orc.BOOLEAN, 0, n)]
    want, _ = orc.aggregate(ocols, 0, 50, aggs)
    w = want[1].length
    data = [(np.asarray(want[0].values[:w]).astype(np.int64), want[0].valid_mask()), (orc.unpack_validity(want[1].values, w).astype(bool), want[1].valid_mask())]
    assert 0 < int((~data[1][1]).sum()) < w
    names = ["start", "last_flag"]
    path = str(tmp_path / "out.parquet")
    info = capi.write_parquet(path, [capi.out_as_column(o) for o in got], names, page_rows=256, row_group_rows=2048, codec=1, booleans=True)
    md = verify(path, data, names, 256, 2048, info=info, codec=1)
    assert md.schema.column(1).physical_type == "BOOLEAN"


# ------------------------------------------------------------------ 7. fuzz
SEEDS = 32


def fuzz_frame(seed):
    rng = np.random.default_rng(2000 + seed)
    ncols = int(rng.integers(1, 5))
    n = int(rng.choice([0, 1, int(rng.integers(2, 200)), int(rng.integers(200, 2049))], p=[0.03, 0.03, 0.34, 0.6]))
    page = int(rng.choice([64, 128, 512]))
    rg = page * int(rng.integers(1, 5))
    fr, enc = Frame(seed), []
    for i in range(ncols):
        kind = "bif"[int(rng.choice(3, p=[0.6, 0.2, 0.2]))] if i else "b"   # (at least one Boolean column)
        density = float(rng.choice([0.0, 0.05, 0.5, 0.95, 1.0]))
        valid = None if rng.random() < 0.2 else rng.random(n) < density
        if valid is not None and n > 2 * page and rng.random() < 0.5:   # whole pages of one kind among the mixed ones
            p = int(rng.integers(0, n // page))
            valid[p * page:(p + 1) * page] = bool(rng.integers(0, 2))
        if kind == "b":
            values = rng.random(n) < float(rng.choice([0.0, 0.1, 0.5, 1.0]))
            enc.append(PLAIN)
        elif kind == "i":
            values = delta_shapes(n, rng)[str(rng.choice(["constant", "timestamps", "full_range"]))]
            enc.append(DELTA if rng.random() < 0.6 else PLAIN)
        else:
            values = float_values(n, rng)
            enc.append(PLAIN)
        fr.add("c%d" % i, values, valid, offset=int(rng.integers(0, 70)), res=RES[int(rng.integers(0, 3))], known=bool(rng.integers(0, 2)),
               odd_address=bool(rng.integers(0, 2)))
    return fr, enc, page, rg


def test_fuzz_against_pyarrow_and_the_loader(tmp_path):
    ran = 0
    for seed in range(SEEDS):
        fr, enc, page, rg = fuzz_frame(seed)
        path = str(tmp_path / ("fuzz%d.parquet" % seed))
        info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, statistics=bool(seed % 2), codec=(seed // 2) % 2)
        verify(path, fr.data, fr.names, page, rg, encodings=enc, info=info, statistics=bool(seed % 2), codec=(seed // 2) % 2)
        os.remove(path)
        ran += 1
    assert ran == SEEDS
