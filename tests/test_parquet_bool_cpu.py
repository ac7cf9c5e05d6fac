"""The Parquet loader's BOOLEAN entry points without a GPU: bowgpu_parquet_read_bool_column / bowgpu_parquet_bool_column_check in the
header and the binding under the unchanged ABI version, what the host-only check accepts and reports (pyarrow's PLAIN and RLE files,
the hand-built ones of tests/parquet_bool_pages.py), every decline with its code and the column's name, the INT64 / DOUBLE entry
points declining a BOOLEAN column as they always did, and the proof of the builders: pyarrow reads the well-formed hand-built files
back as built and refuses the damaged ones."""
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_bool_pages as pb
import parquet_streams as ps
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, ARG = -9, -10


def declined(f, i, code=UNSUPPORTED):
    with pytest.raises(capi.BowGpuError) as e:
        f.check_bool_column(i)
    assert e.value.code == code, e.value.message
    return e.value.message


def test_header_and_binding_hold_the_two_symbols_under_abi_14():
    src = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    assert re.search(r"\bint\s+bowgpu_parquet_read_bool_column\s*\(\s*bowgpu_parquet\s*\*\s*handle,\s*int32_t\s+i,\s*bowgpu_out\s*\*\s*out\s*\)", src)
    assert re.search(r"\bint\s+bowgpu_parquet_bool_column_check\s*\(\s*const\s+bowgpu_parquet\s*\*\s*handle,\s*int32_t\s+i,\s*uint32_t\s*\*\s*value_encodings\s*\)", src)
    assert re.search(r"#define\s+BOWGPU_ABI_VERSION\s+14\b", src)
    assert "(still 14): bowgpu_parquet_read_bool_column" in src
    assert re.search(r"BOWGPU_PARQUET_ENC_RLE\s*=\s*8\b", src)
    assert "bowgpu_parquet_read_bool_column" in capi.SYMBOLS and "bowgpu_parquet_bool_column_check" in capi.SYMBOLS
    assert capi.PARQUET_ENC_RLE == 1 << 3
    L = capi.lib()
    assert hasattr(L, "bowgpu_parquet_read_bool_column") and hasattr(L, "bowgpu_parquet_bool_column_check")
    assert hasattr(capi.ParquetFile, "read_bool_column") and hasattr(capi.ParquetFile, "check_bool_column")


@pytest.mark.parametrize("mode,mask", [("plain_v1", capi.PARQUET_ENC_PLAIN), ("rle_v1", capi.PARQUET_ENC_RLE), ("rle_v2", capi.PARQUET_ENC_RLE)])
def test_check_reports_the_encoding_pyarrow_wrote(tmp_path, mode, mask):
    rng = np.random.default_rng(3)
    n = 1000
    vals, valid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    for k, (vd, kw) in enumerate([(valid, {}), (None, {}),
                                  (valid, dict(write_batch_size=100, data_page_size=16, row_group_size=330, compression="snappy"))]):
        p = str(tmp_path / ("%s_%d.parquet" % (mode, k)))
        pb.write_pyarrow(p, vals, vd, mode, **kw)
        f = capi.ParquetFile(p)
        assert f.columns == [("flag", capi.BOOLEAN, vd is not None)]
        assert f.check_bool_column(0) == mask, (mode, k)
        f.close()


def test_hand_built_files_are_accepted_and_pyarrow_reads_them_as_built(tmp_path):
    """the proof of tests/parquet_bool_pages.py: pyarrow decodes every well-formed file to the values and nulls the builder meant
    (but the one with a zero-length run in mid-stream, which pyarrow refuses: see parquet_bool_pages.well_formed)"""
    files = pb.well_formed(np.random.default_rng(11))
    assert {"padded_last_group", "zero_length_runs", "one_rle_run", "mixed_codec0", "mixed_codec1"} <= set(files)
    for name, (pages, optional, codec, vals, valid) in files.items():
        p = str(tmp_path / (name + ".parquet"))
        pb.write_file(p, pages, optional, codec)
        if name in pb.NO_PYARROW:
            with pytest.raises(OSError, match="Unexpected end of stream"):
                pq.read_table(p)
        else:
            gv, gm = pb.read_back(p, "flag")
            assert np.array_equal(gm, valid), name
            assert np.array_equal(gv, vals & valid), name
        f = capi.ParquetFile(p)
        want = capi.PARQUET_ENC_PLAIN | capi.PARQUET_ENC_RLE if name.startswith("mixed") else capi.PARQUET_ENC_RLE
        assert f.check_bool_column(0) == want, name
        f.close()


def test_damaged_files_pyarrow_refuses_and_the_host_check_finds_what_a_stored_page_shows(tmp_path):
    """The judge of a damaged file is the format specification: each of these is short of bytes, runs or levels it promises, and
    bowgpu_parquet_read_bool_column must return BOWGPU_ERR_ARG for each (tests/test_gpu_parquet_bool.py).  What pyarrow 25 does with
    them, recorded here:
      plain_short_required / _optional / _snappy     OSError "Unexpected end of stream"
      rle_prefix_past_page / _snappy                 OSError "Received invalid number of bytes : 19 (corrupt data page?)"
      rle_stream_ends_early_bp / _rle                OSError "Unexpected end of stream"
      rle_run_past_prefix                            OSError "Unexpected end of stream"
      levels_end_early / levels_end_early_v2_rle     OSError "Number of decoded rep / def levels do not match num_values in page header"
      implausible_size                               OSError "Page didn't decompress to expected size"
    The host-only check reports the ones it can see without a device - sizes in the headers, and in a stored page the length prefix
    and a REQUIRED column's PLAIN bytes; what needs the levels counted or a page decompressed is the kernel's (a status bit)."""
    files = pb.damaged(np.random.default_rng(12))
    assert len(files) == 11
    host_sees = {"plain_short_required": "PLAIN page of column 'flag'", "rle_prefix_past_page": "RLE length prefix",
                 "implausible_size": "implausible page header in column 'flag'"}
    for name, (pages, optional, codec) in files.items():
        p = str(tmp_path / (name + ".parquet"))
        pb.write_file(p, pages, optional, codec)
        with pytest.raises(OSError):
            pq.read_table(p)
        f = capi.ParquetFile(p)
        if name in host_sees:
            msg = declined(f, 0, ARG)
            assert host_sees[name] in msg and "'flag'" in msg, (name, msg)
        else:
            assert f.check_bool_column(0) in (capi.PARQUET_ENC_PLAIN, capi.PARQUET_ENC_RLE), name
        f.close()


def test_every_decline_has_its_code_and_names_the_column(tmp_path):
    rng = np.random.default_rng(5)
    n = 500
    vals, valid = rng.random(n) < 0.5, rng.random(n) >= 0.3
    extra = {"t": pa.array(np.arange(n, dtype=np.int64)), "x": pa.array(rng.standard_normal(n))}
    # a column that is not BOOLEAN: the message points to the INT64 / DOUBLE entry point
    p = str(tmp_path / "mixed_types.parquet")
    pb.write_pyarrow(p, vals, valid, extra=extra)
    f = capi.ParquetFile(p)
    for i, name in ((0, "t"), (1, "x")):
        msg = declined(f, i)
        assert "'%s'" % name in msg and "not BOOLEAN" in msg and "bowgpu_parquet_read_column" in msg, msg
    assert f.check_bool_column(2) == capi.PARQUET_ENC_PLAIN
    for i in (-1, 3):
        declined(f, i, -6)
    f.close()
    # another codec
    p = str(tmp_path / "zstd.parquet")
    pb.write_pyarrow(p, vals, valid, compression="zstd")
    f = capi.ParquetFile(p)
    msg = declined(f, 0)
    assert "codec" in msg and "'flag'" in msg, msg
    f.close()
    # a dictionary page and dictionary-encoded data pages (no writer emits them for BOOLEAN; the headers can still claim them)
    p = str(tmp_path / "dictionary.parquet")
    ps.write_file(p, [ps.dict_page([("bp", [0, 1, 1, 0])], 1, 4)], ptype=pb.BOOLEAN, dictionary=np.array([0, 1], dtype=np.int64), name="flag")
    f = capi.ParquetFile(p)
    msg = declined(f, 0)
    assert "dictionary" in msg and "'flag'" in msg, msg
    f.close()
    # any other value encoding, RLE_DICTIONARY without a dictionary page among them
    for enc in (2, 4, 5, 8, 9):
        p = str(tmp_path / ("enc%d.parquet" % enc))
        pb.write_file(p, [pb.bool_page(pb.plain_bits(vals[:64]), 64, enc)])
        f = capi.ParquetFile(p)
        msg = declined(f, 0)
        assert "value encoding %d" % enc in msg and "'flag'" in msg and "PLAIN and RLE" in msg, msg
        f.close()
    # a definition-level encoding other than RLE on a v1 page (BIT_PACKED = 4): the header of a hand-built page, patched
    p = str(tmp_path / "bit_packed_levels.parquet")
    pb.write_file(p, [pb.plain_page(vals[:32], valid[:32])], optional=True)
    data = bytearray(open(p, "rb").read())
    hdr = bytes([0x15, 32 << 1, 0x15, pb.PLAIN << 1, 0x15, 3 << 1, 0x15, 3 << 1])   # DataPageHeader: num_values, encoding, def, rep
    at = bytes(data).index(hdr)
    data[at + 5] = 4 << 1
    open(p, "wb").write(bytes(data))
    f = capi.ParquetFile(p)
    msg = declined(f, 0)
    assert "definition-level encoding 4" in msg and "'flag'" in msg, msg
    f.close()
    # a schema that is not flat
    p = str(tmp_path / "repeated.parquet")
    pb.write_file(p, [pb.plain_page(vals[:64], valid[:64])], optional=True)
    pb.make_repeated(p)
    f = capi.ParquetFile(p)
    msg = declined(f, 0)
    assert "nested / repeated schema" in msg and "'flag'" in msg, msg
    f.close()


def test_the_int64_double_entry_points_decline_a_boolean_column_as_before(tmp_path):
    rng = np.random.default_rng(6)
    n = 300
    p = str(tmp_path / "flag.parquet")
    pb.write_pyarrow(p, rng.random(n) < 0.5, rng.random(n) >= 0.3, extra={"t": pa.array(np.arange(n, dtype=np.int64))})
    f = capi.ParquetFile(p)
    assert f.check_column(0) == capi.PARQUET_ENC_PLAIN
    for call in (f.check_column, f.read_column):   # (the type gate comes before any device)
        with pytest.raises(capi.BowGpuError) as e:
            call(1)
        assert e.value.code == UNSUPPORTED
        assert e.value.message == "parquet: column 'flag' is not INT64 / DOUBLE (physical type 0)"
    f.close()


def test_long_runs_are_three_rle_runs(tmp_path):
    """the file the long-run case of tests/test_gpu_parquet_bool.py reads holds what it is meant to hold: 5000 true, 3000 false, 77 true as three RLE runs"""
    path = str(tmp_path / "runs.parquet")
    pb.write_pyarrow(path, np.concatenate([np.ones(5000, bool), np.zeros(3000, bool), np.ones(77, bool)]), None, "rle_v1")
    data = open(path, "rb").read()
    body = b"".join(bytes([(c << 1) & 0x7f | 0x80, (c << 1) >> 7, v]) for c, v in ((5000, 1), (3000, 0))) + bytes([77 << 1 & 0x7f | 0x80, 77 << 1 >> 7, 1])
    assert body in data


def test_a_file_without_rows_checks_clean(tmp_path):
    p = str(tmp_path / "empty.parquet")
    pb.write_pyarrow(p, np.zeros(0, bool), np.zeros(0, bool))
    f = capi.ParquetFile(p)
    assert f.num_rows == 0 and f.check_bool_column(0) == 0
    f.close()
