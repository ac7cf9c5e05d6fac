"""DELTA_BINARY_PACKED (INT64) and BYTE_STREAM_SPLIT (INT64 / DOUBLE) pages decoded on the device (delta_pages_kernel /
bss_pages_kernel in parquet_decode.hip).  The expectation is always pyarrow.parquet.read_table of the same file.  Files: what
pyarrow writes (block 256 / 4 miniblocks) over value counts at its block and miniblock edges, value shapes that reach every bit
width from 0 to 64, nulls, page sizes, row groups, page versions and codecs; and files written page by page by
tests/parquet_pages.py for what pyarrow cannot write (other block layouts, a chunk that mixes encodings)."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_pages as pp
from bow_amd import capi
from test_parquet_loader import check_file, expect

pytestmark = pytest.mark.gpu

WRAP = np.array([0, 2 ** 63 - 1, -2 ** 63, -1, 2 ** 63 - 1, 0], dtype=np.int64)


def write(table, path, encoding, **kw):
    kw.setdefault("compression", "none")
    kw.setdefault("data_page_version", "1.0")
    pq.write_table(table, path, use_dictionary=False, column_encoding={name: encoding for name in table.schema.names}, **kw)
    md = pq.ParquetFile(path).metadata
    for g in range(md.num_row_groups):
        for j in range(md.num_columns):
            assert encoding in md.row_group(g).column(j).encodings   # the writer did what it was asked
    return path


def with_nulls(values, n_valid_rows_extra, rng):
    """an OPTIONAL column holding exactly `values` as its non-null values, nulls spread between them"""
    rows = len(values) + n_valid_rows_extra
    valid = np.zeros(rows, dtype=bool)
    valid[rng.choice(rows, len(values), replace=False)] = True
    full = np.zeros(rows, dtype=values.dtype)
    full[valid] = values
    return pa.array(full, mask=~valid)


def test_delta_value_counts_at_block_and_miniblock_edges(tmp_path):
    """pyarrow: 256 values per block, 64 per miniblock, after the first value.  1: no block; 2: one delta; 257 / 258: one full block
    / one value into a second; 321 / 322: a miniblock edge of the second block"""
    rng = np.random.default_rng(31)
    for n in (1, 2, 257, 258, 321, 322, 100_000):
        ts = np.cumsum(rng.integers(1, 20, n)).astype(np.int64)
        req = pa.table({"req": pa.array(ts)}, schema=pa.schema([pa.field("req", pa.int64(), nullable=False)]))
        assert check_file(write(req, str(tmp_path / ("req%d.parquet" % n)), "DELTA_BINARY_PACKED"), req) == 1
        opt = pa.table({"opt": with_nulls(ts, n // 3 + 2, rng)})
        assert opt.column(0).null_count == n // 3 + 2
        assert check_file(write(opt, str(tmp_path / ("opt%d.parquet" % n)), "DELTA_BINARY_PACKED"), opt) == 1


def test_delta_value_shapes(tmp_path):
    rng = np.random.default_rng(32)
    n = 60_000
    cols = {"ascending": np.cumsum(rng.integers(1, 20, n)).astype(np.int64),                  # narrow widths
            "constant": np.full(n, 1234567, dtype=np.int64),                                    # width 0
            "descending": (10 ** 12 - np.cumsum(rng.integers(1, 5000, n))).astype(np.int64),    # negative min_delta
            "full_range": rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64),               # width 64
            "wrap": np.tile(WRAP, n // len(WRAP))}                                              # differences that wrap
    table = pa.table({k: pa.array(v) for k, v in cols.items()})
    assert check_file(write(table, str(tmp_path / "shapes.parquet"), "DELTA_BINARY_PACKED"), table) == 5


@pytest.mark.parametrize("null_frac", [0.3, 1.0])
def test_delta_with_nulls(tmp_path, null_frac):
    """value count != row count; at density 1.0 every page holds nulls only"""
    rng = np.random.default_rng(33)
    n = 50_000
    table = pa.table({"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64), mask=rng.random(n) < null_frac),
                      "full": pa.array(rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), mask=rng.random(n) < null_frac)})
    assert check_file(write(table, str(tmp_path / "nulls.parquet"), "DELTA_BINARY_PACKED", data_page_size=4096), table) == 2


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_delta_page_sizes_row_groups_versions_codecs(tmp_path, version, compression):
    """small pages start anywhere inside an output validity word; check_file reads into HOST and into DEVICE outputs"""
    rng = np.random.default_rng(34)
    n = 100_003
    table = pa.table({"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64)),
                      "i": pa.array(rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64), mask=rng.random(n) < 0.3),
                      "runs": pa.array(np.repeat(rng.integers(0, 100, n // 50 + 1), 50)[:n].astype(np.int64), mask=rng.random(n) < 0.3)})
    for page, rg in ((1024, 50_002), (4096, 33_400)):   # two and three row groups
        path = write(table, str(tmp_path / ("p%d.parquet" % page)), "DELTA_BINARY_PACKED", data_page_size=page, row_group_size=rg,
                     data_page_version=version, compression=compression)
        assert pq.ParquetFile(path).metadata.num_row_groups == -(-n // rg)
        assert check_file(path, table) == 3


def edge_counts(block, minis):
    v = block // minis
    return [1, 2, v, v + 1, v + 2, block, block + 1, block + 2, block + v + 1, block + v + 2, 2 * block + 1, 3 * block + 7]


@pytest.mark.parametrize("block,minis", [(128, 4), (256, 8), (1024, 4)])
def test_hand_written_delta_block_layouts(tmp_path, block, minis):
    """parquet-mr's 128 / 4 and two more legal layouts: one page per value count, the counts at this layout's own edges"""
    rng = np.random.default_rng(35)
    kw = {"block_size": block, "miniblocks": minis}
    req, opt = [], []
    for k, n in enumerate(edge_counts(block, minis)):
        vals = (np.cumsum(rng.integers(-3, 1 << (k * 5 % 50), n)).astype(np.int64), rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), np.tile(WRAP, n // 6 + 1)[:n])[k % 3]
        req.append((pp.DELTA_BINARY_PACKED, vals, None, kw))
        rows = n + n // 2 + 1   # the same count of non-null values among more rows
        valid = np.zeros(rows, dtype=bool)
        valid[rng.choice(rows, n, replace=False)] = True
        full = np.zeros(rows, dtype=np.int64)
        full[valid] = vals
        opt.append((pp.DELTA_BINARY_PACKED, full, valid, kw))
    for name, pages, optional in (("req", req, False), ("opt", opt, True)):
        path = str(tmp_path / ("%s_%d_%d.parquet" % (name, block, minis)))
        pp.write_file(path, pages, optional=optional)
        assert check_file(path) == 1


@pytest.mark.parametrize("optional", [False, True])
def test_hand_written_chunk_that_mixes_plain_delta_and_bss_pages(tmp_path, optional):
    rng = np.random.default_rng(36)
    ts = np.cumsum(rng.integers(1, 20, 5000)).astype(np.int64)
    full = rng.integers(-2 ** 63, 2 ** 63 - 1, 777, dtype=np.int64)

    def v(n):
        return (rng.random(n) >= 0.3) if optional else None
    pages = [(pp.PLAIN, ts[:501], v(501)), (pp.DELTA_BINARY_PACKED, ts[501:1700], v(1199)), (pp.BYTE_STREAM_SPLIT, full, v(777)),
             (pp.DELTA_BINARY_PACKED, ts[1700:], v(3300), {"block_size": 256, "miniblocks": 8}), (pp.PLAIN, full[:3], v(3)),
             (pp.BYTE_STREAM_SPLIT, ts[:65], v(65))]
    path = str(tmp_path / "mixed.parquet")
    pp.write_file(path, pages, optional=optional)
    f = capi.ParquetFile(path)
    assert f.check_column(0) == capi.PARQUET_ENC_PLAIN | capi.PARQUET_ENC_DELTA_BINARY_PACKED | capi.PARQUET_ENC_BYTE_STREAM_SPLIT
    f.close()
    assert check_file(path) == 1


def special_doubles(n, rng):
    x = rng.standard_normal(n)
    bits = x.view(np.uint64)
    specials = np.array([0x7ff8000000000000, 0x7ff0000000000001, 0xfff8dead0000beef, 0x7ff4000000000123,   # NaNs with payloads
                         0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000,   # +-0, +-Inf
                         0x0000000000000001, 0xffffffffffffffff], dtype=np.uint64)
    at = rng.choice(n, min(n, 4 * len(specials)), replace=False)
    bits[at] = specials[np.arange(len(at)) % len(specials)]
    return x


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_byte_stream_split(tmp_path, version, compression):
    """DOUBLE and INT64, with and without nulls; the DOUBLE values include NaN payloads, +-0 and +-Inf (check_file compares bits)"""
    rng = np.random.default_rng(37)
    for n in (1, 7, 64, 65, 100_000):
        d, i = special_doubles(n, rng), rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
        table = pa.table({"d": pa.array(d), "i": pa.array(i), "d_nulls": pa.array(d, mask=rng.random(n) < 0.3),
                          "i_nulls": pa.array(i, mask=rng.random(n) < 0.3)},
                         schema=pa.schema([pa.field("d", pa.float64(), nullable=False), pa.field("i", pa.int64(), nullable=False),
                                           pa.field("d_nulls", pa.float64()), pa.field("i_nulls", pa.int64())]))
        got = pa.table({"d": table.column("d")}).column(0).to_numpy()
        assert np.array_equal(got.view(np.uint64), d.view(np.uint64))   # (arrow kept the NaN payloads)
        path = write(table, str(tmp_path / ("bss%d.parquet" % n)), "BYTE_STREAM_SPLIT", data_page_version=version, compression=compression,
                     data_page_size=8192)
        assert check_file(path, table) == 4


def test_damaged_delta_files_come_back_clean(tmp_path):
    """bytes flipped inside the column chunks of a small delta file: every call returns - with an error or with some decode of the
    damaged data - and an intact file decodes correctly afterwards (the kernels bound every read by the page's size)"""
    rng = np.random.default_rng(38)
    n = 1000
    table = pa.table({"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64)),
                      "i": pa.array(rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64), mask=rng.random(n) < 0.3)})
    good_path = write(table, str(tmp_path / "good.parquet"), "DELTA_BINARY_PACKED", data_page_size=1024)
    good = open(good_path, "rb").read()
    md = pq.ParquetFile(good_path).metadata
    lo = min(md.row_group(0).column(j).data_page_offset for j in range(2))
    hi = max(md.row_group(0).column(j).data_page_offset + md.row_group(0).column(j).total_compressed_size for j in range(2))
    errors = 0
    for k in range(20):
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 5))):
            b[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
        if k % 2:   # and one in the first bytes of a chunk: its page header, the delta header, the first block's min delta and widths
            b[int(md.row_group(0).column(k // 2 % 2).data_page_offset + rng.integers(0, 48))] = int(rng.integers(0, 256))
        path = str(tmp_path / ("bad%d.parquet" % k))
        open(path, "wb").write(bytes(b))
        f = capi.ParquetFile(path)
        for i in range(2):
            try:
                f.read_column(i)
            except capi.BowGpuError as e:
                assert e.code in (-10, -9), e  # malformed page data / a page that now claims another encoding
                errors += 1
        f.close()
    print("damaged copies: %d of 40 column reads came back as errors" % errors)
    assert check_file(good_path, table) == 2


def test_delta_and_bss_columns_to_rolling_mean_without_leaving_the_device(tmp_path):
    """a delta-encoded timestamp column and a BYTE_STREAM_SPLIT value column are decoded into HBM and aggregated there; the
    expectation is the oracle over pyarrow's decode of the same file"""
    from oracle import pyoracle as orc
    from test_gpu_aggregate import compare
    rng = np.random.default_rng(39)
    n = 50_000
    table = pa.table({"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64)),
                      "val": pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.3)})
    path = str(tmp_path / "pipeline.parquet")
    pq.write_table(table, path, use_dictionary=False, compression="snappy", data_page_version="2.0",
                   column_encoding={"ts": "DELTA_BINARY_PACKED", "val": "BYTE_STREAM_SPLIT"})
    f = capi.ParquetFile(path)
    assert f.check_column(0) == capi.PARQUET_ENC_DELTA_BINARY_PACKED and f.check_column(1) == capi.PARQUET_ENC_BYTE_STREAM_SPLIT
    ts = f.read_column(0, out_residency=capi.DEVICE)
    val = f.read_column(1, out_residency=capi.DEVICE)
    assert ts.null_count == 0
    cols = [capi.Column(ts.values, None, capi.INT64, 0, n, 0), capi.Column(val.values, val.validity, capi.FLOAT64, 0, n, val.null_count)]
    aggs = [("WindowStart", 0), ("ArithmeticMean", 1)]
    back = pq.read_table(path)
    tv, _ = expect(back, "ts")
    vv, vm = expect(back, "val")
    ocols = [orc.Column(tv, None, orc.INT64), orc.Column(vv, np.packbits(vm, bitorder="little"), orc.FLOAT64)]
    got, info = capi.rolling_aggregate(cols, 0, 10, aggs, out_residency=capi.DEVICE)
    want, _ = orc.aggregate(ocols, 0, 10, aggs)
    for (k, _), g, w in zip(aggs, got, want):
        compare("delta + bss %s I=10" % k, g, w)
    f.close()
