"""DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT without a GPU: the hand page writer of tests/parquet_pages.py is checked against pyarrow
(an independent reader - it validates the yardstick the GPU tests use), and bowgpu_parquet_column_check - the loader's walk over a
column's page headers, on the host alone - accepts and declines what bowgpu_parquet_read_column would."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_pages as pp
from bow_amd import capi

WRAP = np.array([0, 2 ** 63 - 1, -2 ** 63, -1, 2 ** 63 - 1, 0], dtype=np.int64)


def helper_files(tmp_path):
    """name -> (path, values, valid, physical type, optional, encodings mask)"""
    rng = np.random.default_rng(21)
    ts = np.cumsum(rng.integers(1, 20, 3000)).astype(np.int64)
    full = rng.integers(-2 ** 63, 2 ** 63 - 1, 700, dtype=np.int64)
    dbl = rng.standard_normal(1000)
    D, B, P = capi.PARQUET_ENC_DELTA_BINARY_PACKED, capi.PARQUET_ENC_BYTE_STREAM_SPLIT, capi.PARQUET_ENC_PLAIN
    out = {}

    def add(name, pages, ptype=pp.INT64, optional=False, mask=0):
        path = str(tmp_path / (name + ".parquet"))
        vals, valid = pp.write_file(path, pages, ptype=ptype, optional=optional)
        out[name] = (path, vals, valid, ptype, optional, mask)

    for bs, mb in ((128, 4), (256, 4), (256, 8), (1024, 4)):
        kw = {"block_size": bs, "miniblocks": mb}
        add("delta_%d_%d" % (bs, mb), [(pp.DELTA_BINARY_PACKED, ts, None, kw), (pp.DELTA_BINARY_PACKED, full, None, kw),
                                       (pp.DELTA_BINARY_PACKED, np.tile(WRAP, 50), None, kw)], mask=D)
    add("bss_int64", [(pp.BYTE_STREAM_SPLIT, full, None), (pp.BYTE_STREAM_SPLIT, ts, None)], mask=B)
    add("bss_double", [(pp.BYTE_STREAM_SPLIT, dbl, None), (pp.BYTE_STREAM_SPLIT, dbl[:65], None)], ptype=pp.DOUBLE, mask=B)
    add("mixed", [(pp.PLAIN, ts[:500], None), (pp.DELTA_BINARY_PACKED, ts[500:1700], None), (pp.BYTE_STREAM_SPLIT, full, None),
                  (pp.DELTA_BINARY_PACKED, ts[1700:], None, {"block_size": 256, "miniblocks": 8}), (pp.PLAIN, full[:3], None)], mask=P | D | B)
    valid = rng.random(3000) >= 0.3
    valid[1000:1500] = False   # the second page holds nulls only
    add("optional_nulls", [(pp.DELTA_BINARY_PACKED, ts[:1000], valid[:1000]), (pp.DELTA_BINARY_PACKED, ts[1000:1500], valid[1000:1500]),
                           (pp.BYTE_STREAM_SPLIT, ts[1500:2500], valid[1500:2500]), (pp.PLAIN, ts[2500:], valid[2500:])], optional=True, mask=P | D | B)
    return out


def read_back(path):
    c = pq.read_table(path).column(0).combine_chunks()
    valid = ~np.asarray(c.is_null())
    return np.asarray(c.fill_null(0)), valid


def test_pyarrow_reads_the_hand_written_files_back(tmp_path):
    files = helper_files(tmp_path)
    assert len(files) == 8
    for name, (path, vals, valid, ptype, optional, _) in files.items():
        got, gvalid = read_back(path)
        assert got.dtype == (np.int64 if ptype == pp.INT64 else np.float64), name
        assert np.array_equal(gvalid, valid), name
        assert np.array_equal(got.view(np.uint64)[valid], vals.view(np.uint64)[valid]), name
        md = pq.ParquetFile(path).metadata
        assert md.num_rows == len(vals) and md.num_row_groups == 1, name
        assert (not valid.all()) == (name == "optional_nulls")


def test_check_column_accepts_the_hand_written_files(tmp_path):
    for name, (path, vals, valid, ptype, optional, mask) in helper_files(tmp_path).items():
        f = capi.ParquetFile(path)
        assert f.num_rows == len(vals) and f.columns == [("c", capi.INT64 if ptype == pp.INT64 else capi.FLOAT64, optional)], name
        assert f.check_column(0) == mask, name
        f.close()


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("compression", ["snappy", "none"])
def test_check_column_accepts_what_pyarrow_writes(tmp_path, version, compression):
    rng = np.random.default_rng(22)
    n = 20_000
    t = pa.table({"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64)),
                  "i": pa.array(rng.integers(0, 1000, n).astype(np.int64), mask=rng.random(n) < 0.3),
                  "f": pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.3)})
    kw = dict(compression=compression, data_page_version=version, data_page_size=8192, row_group_size=7000)
    D, B, P = capi.PARQUET_ENC_DELTA_BINARY_PACKED, capi.PARQUET_ENC_BYTE_STREAM_SPLIT, capi.PARQUET_ENC_PLAIN
    dict_bits = capi.PARQUET_ENC_PLAIN_DICTIONARY | capi.PARQUET_ENC_RLE_DICTIONARY
    cases = {"delta": (dict(use_dictionary=False, column_encoding={"ts": "DELTA_BINARY_PACKED", "i": "DELTA_BINARY_PACKED", "f": "PLAIN"}), [D, D, P]),
             "bss": (dict(use_dictionary=False, column_encoding={"ts": "BYTE_STREAM_SPLIT", "i": "BYTE_STREAM_SPLIT", "f": "BYTE_STREAM_SPLIT"}), [B, B, B]),
             "plain": (dict(use_dictionary=False), [P, P, P]),
             "dict": (dict(use_dictionary=["i"]), [P, None, P])}
    for name, (extra, want) in cases.items():
        path = str(tmp_path / (name + ".parquet"))
        pq.write_table(t, path, **kw, **extra)
        f = capi.ParquetFile(path)
        for i, w in enumerate(want):
            got = f.check_column(i)
            if w is None:   # dictionary pages: PLAIN_DICTIONARY from a v1 writer, RLE_DICTIONARY from a v2 one
                assert got and not (got & ~dict_bits), (name, i, got)
            else:
                assert got == w, (name, i, got)
        f.close()


def test_check_column_declines_what_read_column_declines(tmp_path):
    t = pa.table({"a": pa.array(np.arange(1000, dtype=np.int64) % 7), "b": pa.array(np.arange(1000) % 2 == 0)})
    p = str(tmp_path / "zstd.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="zstd")
    f = capi.ParquetFile(p)
    with pytest.raises(capi.BowGpuError) as e:
        f.check_column(0)
    assert e.value.code == -9 and "codec" in e.value.message
    f.close()
    p = str(tmp_path / "bool.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="none")
    f = capi.ParquetFile(p)
    assert f.check_column(0) == capi.PARQUET_ENC_PLAIN
    with pytest.raises(capi.BowGpuError) as e:
        f.check_column(1)   # the Boolean column
    assert e.value.code == -9 and "INT64 / DOUBLE" in e.value.message
    for i in (-1, 2):
        with pytest.raises(capi.BowGpuError) as e:
            f.check_column(i)
        assert e.value.code == -6, i
    f.close()
    # a DOUBLE column whose pages claim DELTA_BINARY_PACKED: the message names the encoding and the type
    p = str(tmp_path / "delta_double.parquet")
    pp.write_file(p, [(pp.DELTA_BINARY_PACKED, np.arange(100, dtype=np.int64), None)], ptype=pp.DOUBLE)
    f = capi.ParquetFile(p)
    with pytest.raises(capi.BowGpuError) as e:
        f.check_column(0)
    assert e.value.code == -9 and "DELTA_BINARY_PACKED" in e.value.message and "DOUBLE" in e.value.message
    f.close()
