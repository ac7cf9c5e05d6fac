"""The builders of tests/parquet_streams.py, proved without a GPU: pyarrow - an independent reader - reads every well-formed file of
tests/parquet_stream_cases.py back as the intended column, decompresses every hand-built Snappy block to the intended bytes (and so
does the plain decoder beside the builders), and refuses every damaged file and block.  The device tests
(tests/test_gpu_parquet_streams.py) read the same files.  pyarrow 25 accepts none of the damaged cases, so none was dropped."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_stream_cases as cases
import parquet_streams as ps
from bow_amd import capi


def read_back(path):
    c = pq.read_table(path).column(0).combine_chunks()
    return np.asarray(c.fill_null(0)), ~np.asarray(c.is_null())


def test_builders_restate_the_formats():
    """bytes worked out by hand from the format descriptions"""
    assert ps.literal(b"ab") == b"\x04ab" and ps.literal(b"ab", 1) == b"\xf0\x01ab" and ps.literal(b"ab", 4) == b"\xfc\x01\x00\x00\x00ab"
    assert ps.literal(b"x" * 61)[:2] == b"\xf0\x3c" and ps.literal_forms(60) == [0, 1, 2, 3, 4] and ps.literal_forms(257) == [2, 3, 4]
    assert ps.literal_forms(65537) == [3, 4]
    assert ps.copy(0x123, 7, 1) == bytes([1 | (3 << 2) | (1 << 5), 0x23])
    assert ps.copy(0x1234, 64, 2) == b"\xfe\x34\x12" and ps.copy(3, 11, 3) == b"\x2b\x03\x00\x00\x00"
    assert ps.copy_forms(3, 11) == [1, 2, 3] and ps.copy_forms(65, 64) == [2, 3] and ps.copy_forms(7, 12) == [2, 3]
    s = ps.Snappy().literal(b"abc").copy(3, 7, 1).copy(1, 4, 2)
    assert bytes(s.out) == b"abcabcabcaaaaa" and s.stream()[0] == 14
    # the hybrid: an RLE run of 9 threes at width 3; one bit-packed group 0 .. 7 at width 3 (the specification's own example)
    assert ps.hybrid([("rle", 3, 9)], 3) == b"\x12\x03" and ps.hybrid([("bp", range(8))], 3) == b"\x03\x88\xc6\xfa"
    assert ps.hybrid([("rle", 0, 5), ("bp", [0] * 9)], 0) == b"\x0a\x05" and ps.hybrid([("rle", 2 ** 31, 2)], 32) == b"\x04\x00\x00\x00\x80"
    assert ps.hybrid([("bp", [1, 0, 1])], 1) == b"\x03\x05"
    assert list(ps.expand([("rle", 4, 2), ("bp", [1, 2, 3])], 12)) == [4, 4, 1, 2, 3, 0, 0, 0, 0, 0]


def test_pyarrow_and_the_plain_decoder_decompress_the_hand_built_blocks():
    codec = pa.Codec("snappy")
    blocks = cases.good_blocks()
    for name, s in blocks.items():
        stream, want = s.stream(), bytes(s.out)
        assert codec.decompress(stream, decompressed_size=len(want)).to_pybytes() == want, name
        assert ps.snappy_decode(stream) == want, name
    # what the list is there for: every copy form, the 4-byte literal length, every (off, len) pair
    tags = {n.split("_off")[0] for n in blocks if n.startswith("copy_form")}
    assert tags == {"copy_form1", "copy_form2", "copy_form3"} and "literal_65537_form4" in blocks and "literal_1_form4" in blocks
    for off in cases.COPY_OFFSETS:
        for n in cases.COPY_LENGTHS:
            assert "copy_form3_off%d_len%d" % (off, n) in blocks and "copy_form2_off%d_len%d" % (off, n) in blocks
            assert ("copy_form1_off%d_len%d" % (off, n) in blocks) == (n <= 11)


def test_pyarrow_and_the_plain_decoder_refuse_the_damaged_blocks():
    codec = pa.Codec("snappy")
    blocks = cases.damaged_blocks()
    assert len(blocks) == 9
    for name, (stream, size) in blocks.items():
        with pytest.raises(Exception):
            codec.decompress(stream, decompressed_size=size)
        with pytest.raises(ps.SnappyError):
            got = ps.snappy_decode(stream)
            if len(got) != size:   # (a block that is whole in itself, under a page header that states another size)
                raise ps.SnappyError(name)


def test_pyarrow_reads_the_hand_built_files_back(tmp_path):
    files = cases.good_files(tmp_path)
    assert len(files) == 32
    for name, (path, vals, valid) in files.items():
        got, gvalid = read_back(path)
        assert got.dtype == vals.dtype, name
        assert np.array_equal(gvalid, valid), name
        assert np.array_equal(got.view(np.uint64), vals.view(np.uint64)), name
        md = pq.ParquetFile(path).metadata
        assert md.num_rows == len(vals) and md.num_row_groups == 1, name
        col = md.row_group(0).column(0)
        assert col.compression == ("SNAPPY" if "codec1" in name or name.startswith("snappy") else "UNCOMPRESSED"), name
        assert col.has_dictionary_page == (name.startswith("indices") or ("chunk" in name and "dictionary_page_offset" not in name
                                                                          and "nulls_only" not in name)), name


def test_the_uncompressed_length_preamble_takes_one_two_and_three_bytes(tmp_path):
    path, vals, _ = cases.good_files(tmp_path)["snappy_preambles"]
    raw = open(path, "rb").read()
    rows = [15, 16, 2047, 2048, 2049]
    assert len(vals) == sum(rows)
    at = 0
    for n, width in zip(rows, [1, 2, 2, 3, 3]):
        body = vals[at:at + n].astype("<i8").tobytes()
        at += n
        assert len(ps._uleb(len(body))) == width and ps.one_literal(body) in raw, n


def test_pyarrow_refuses_the_damaged_files_and_reads_their_twins(tmp_path):
    bad, twins = cases.damaged_files(tmp_path)
    assert len(bad) == 9 + 2 * 6 + 4 and len(twins) == 4
    for name, (path, twin) in bad.items():
        with pytest.raises(Exception):
            pq.read_table(path)
    for name, (path, vals, valid) in twins.items():
        got, gvalid = read_back(path)
        assert np.array_equal(gvalid, valid) and np.array_equal(got.view(np.uint64), vals.view(np.uint64)), name


def test_the_loaders_page_walk_accepts_the_hand_built_files(tmp_path):
    """bowgpu_parquet_column_check: the host half of bowgpu_parquet_read_column (page headers, sizes, the page table)"""
    D = capi.PARQUET_ENC_RLE_DICTIONARY
    P = capi.PARQUET_ENC_PLAIN
    for name, (path, vals, valid) in cases.good_files(tmp_path).items():
        f = capi.ParquetFile(path)
        assert f.num_rows == len(vals), name
        want = D if name.startswith("indices") else P if "nulls_only" in name or not name.startswith("chunk") else D | P
        assert f.check_column(0) == want, name
        f.close()


@pytest.mark.parametrize("v2", [False, True])
@pytest.mark.parametrize("claim", [64 + 8, 64 - 8, 64 + (1 << 20)])
def test_a_stored_page_that_claims_another_size_than_it_holds_is_refused(tmp_path, v2, claim):
    """a page that is not compressed is read where it lies, up to the uncompressed size its header states: the walk refuses a header
    whose two sizes differ (codec 0, and a v2 page with is_compressed = false inside a SNAPPY chunk).  pyarrow reads such a page by
    the size the chunk holds, so it is no reference here."""
    vals = np.arange(8, dtype=np.int64)
    path = str(tmp_path / "claim.parquet")
    ps.write_file(path, [ps.plain_page(vals, v2=v2, stored=v2, claim=claim)], codec=1 if v2 else 0)
    f = capi.ParquetFile(path)
    with pytest.raises(capi.BowGpuError) as e:
        f.check_column(0)
    assert e.value.code == -10 and "stored page" in e.value.message
    f.close()
