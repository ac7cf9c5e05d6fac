"""bowgpu_parquet_write_codec with SNAPPY on the device.  Every comparison is exact.  Each file is written twice, with codec 1 and
with codec 0, and verify() reads the codec-1 file three ways: pyarrow (table, compression, statistics equal to the codec-0
file's), the page walk of tests/parquet_snappy_walk.py (every page's decompressed bytes equal the codec-0 file's page bytes as
tests/parquet_page_walk.py shows them; every element obeys the header's rules; the size bound), and the library's own loader.

F below is the fragment size of bow_amd/csrc/snappy_encode.hip (kSnFrag); the shapes are the smallest around its edges."""
import ctypes as C
import os

import numpy as np
import pyarrow.parquet as pq
import pytest

import parquet_page_walk as walk
import parquet_snappy_walk as swalk
from bow_amd import capi
from test_gpu_parquet_write import Frame, delta_shapes, float_values, int_values
from test_parquet_loader import expect

pytestmark = pytest.mark.gpu

PLAIN, DELTA, SNAPPY = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_CODEC_SNAPPY
RES = (capi.HOST, capi.HOST_PINNED, capi.DEVICE)
F = 4096
LIT, COPY = swalk.LITERAL, swalk.COPY


def write_both(tmp_path, name, fr, **kw):
    """the frame with codec 1 and with codec 0; returns (path, path0, info)"""
    path, path0 = str(tmp_path / (name + ".parquet")), str(tmp_path / (name + "_plain.parquet"))
    try:
        info = capi.write_parquet(path, fr.cols, fr.names, codec=SNAPPY, **kw)
        capi.write_parquet(path0, fr.cols, fr.names, **kw)
    finally:
        fr.release()
    return path, path0, info


def literal_cost(n):
    return n + (1 if n <= 60 else 2 if n <= 256 else 3 if n <= 65536 else 4)


def check_elements(vals, n):
    """the rules of a values stream of n bytes: elements stay inside their fragment of F bytes, copies hold 4 .. 64 bytes and reach
    neither further back than F nor before their fragment's start, tags are the 1-, 2- or 3-byte forms"""
    at = 0
    for kind, ln, d, pos, t in vals:
        assert pos == at and ln >= 1
        frag = pos // F * F
        assert pos + ln <= min(frag + F, n), (kind, ln, d, pos)
        if kind == COPY:
            assert 4 <= ln <= 64 and 1 <= d <= pos - frag and d < F and t in (2, 3), (ln, d, pos, t)
            assert t == 3 or (ln <= 11 and d < 2048)
        else:
            assert t <= 3
        at += ln
    assert at == n


def verify(path, path0, data, names, encodings=None, info=None):
    """data: [(values, valid)] per column.  Returns {(column, row group): [values elements per page]}."""
    ncols, n = len(data), len(data[0][0])
    encodings = encodings or [PLAIN] * ncols
    assert sorted(os.listdir(os.path.dirname(path))).count(os.path.basename(path) + ".tmp") == 0
    f, md0 = pq.ParquetFile(path), pq.read_metadata(path0)
    md = f.metadata
    assert md.num_rows == n and md.num_columns == ncols and md.num_row_groups == md0.num_row_groups
    table = f.read()
    assert table.schema.names == list(names)
    out, level_bytes, value_bytes, npages = {}, 0, 0, 0
    for i, (values, valid) in enumerate(data):
        gv, gm = expect(table, names[i])
        assert np.array_equal(gm, valid), (names[i], np.flatnonzero(gm != valid)[:10])
        assert np.array_equal(np.asarray(gv).view(np.uint64)[valid], values.view(np.uint64)[valid]), names[i]
        for g in range(md.num_row_groups):
            ch, ch0 = md.row_group(g).column(i), md0.row_group(g).column(i)
            assert ch.compression == "SNAPPY" and ch0.compression == "UNCOMPRESSED"
            assert ch.num_values == ch0.num_values and ch.encodings == ch0.encodings and ch.physical_type == ch0.physical_type
            # (total_uncompressed_size counts the page headers, which differ by the bytes of compressed_page_size: the walker sums it)
            assert ch0.total_uncompressed_size == ch0.total_compressed_size and ch.total_compressed_size > 0
            st, st0 = ch.statistics, ch0.statistics
            assert (st.null_count, st.has_min_max) == (st0.null_count, st0.has_min_max)
            if st0.has_min_max:
                assert np.array([st.min, st.max]).tobytes() == np.array([st0.min, st0.max]).tobytes()
            pages, pages0 = list(swalk.pages(path, ch)), list(walk.pages(path0, ch0))
            assert len(pages) == len(pages0)
            per_page = []
            for pg, pg0 in zip(pages, pages0):
                assert pg[:4] == pg0 and pg[1] == encodings[i]
                nv, lv = len(pg[3]), 4 + len(pg[2])
                vals = swalk.values_elements(pg[5], len(pg[2]))
                check_elements(vals, nv)
                # the section: the preamble, the levels as one literal, and at most 32 + n + n / 6 bytes for the n bytes of values
                assert len(pg[4]) <= len(walk_varint(lv + nv)) + literal_cost(lv) + (32 + nv + nv // 6 if nv else 0)
                per_page.append(vals)
                level_bytes, value_bytes, npages = level_bytes + lv, value_bytes + nv, npages + 1
            out[(i, g)] = per_page
    if info is not None:
        assert (info.rows, info.row_groups, info.data_pages, info.file_bytes) == (n, md.num_row_groups, npages, os.path.getsize(path))
        assert (info.level_bytes, info.value_bytes) == (level_bytes, value_bytes)   # the uncompressed section sizes
    lf = capi.ParquetFile(path)
    assert lf.num_rows == n and [c[0] for c in lf.columns] == list(names)
    for i, (values, valid) in enumerate(data):
        got = lf.read_column(i)
        assert got.length == n and got.null_count == int((~valid).sum())
        assert np.array_equal(got.valid_mask(), valid)
        assert np.array_equal(got.host_arrays()[0].view(np.uint64)[valid], values.view(np.uint64)[valid])
    lf.close()
    return out


def walk_varint(v):
    b = bytearray()
    while v >= 0x80:
        b.append((v & 0x7f) | 0x80)
        v >>= 7
    b.append(v)
    return bytes(b)


def from_bytes(b, dtype=np.int64):
    assert len(b) % 8 == 0
    return np.frombuffer(bytes(b), dtype=dtype).copy()


# ------------------------------------------------------------------ 1. edges of the fragment
EDGE_ROWS = [0, 1, F // 8 - 1, F // 8, F // 8 + 1, 2 * (F // 8) + 1]


@pytest.mark.parametrize("n", EDGE_ROWS)
def test_fragment_edges_over_random_and_constant_values(tmp_path, n):
    rng = np.random.default_rng(200 + n)
    fr = Frame()
    fr.add("ri", rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64), None, res=capi.DEVICE)
    fr.add("rf", rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64).view(np.float64), None, offset=3, res=capi.HOST)   # (any bit pattern)
    fr.add("ci", np.full(n, -123456789012345, dtype=np.int64), None, offset=5, res=capi.HOST)
    fr.add("cf", np.full(n, 2.718281828), None, res=capi.DEVICE)
    path, path0, info = write_both(tmp_path, "edge%d" % n, fr, page_rows=1088, row_group_rows=1088)
    els = verify(path, path0, fr.data, fr.names, info=info)
    if n == 0:
        assert els == {}
        return
    frags = [min(F, 8 * n - a) for a in range(0, 8 * n, F)]
    for i in (0, 1):   # random values: one literal per fragment
        assert [(e[0], e[1]) for e in els[(i, 0)][0]] == [(LIT, k) for k in frags]
    for i in (2, 3):   # a constant: per fragment the first value as a literal, then overlapping copies of 64 at distance 8 and the rest
        want = []
        for k in frags:
            want.append((LIT, 8, 0))
            left = k - 8
            want += [(COPY, 64, 8)] * (left // 64) + ([(COPY, left % 64, 8)] if left % 64 else [])
        assert [e[:3] for e in els[(i, 0)][0]] == want


# ------------------------------------------------------------------ 2. literal length forms
@pytest.mark.parametrize("lit,tag", [(60, 1), (61, 2), (256, 2), (257, 3)])
def test_literal_length_forms_end_where_a_match_begins(tmp_path, lit, tag):
    """`lit` random bytes, then the bytes from 8 back repeated: the literal holds exactly `lit` bytes.  (65 536 and 65 537 do not
    occur: a fragment holds 4096 bytes.)"""
    rng = np.random.default_rng(300 + lit)
    b = bytearray(rng.integers(0, 256, lit, dtype=np.uint8).tobytes())
    while len(b) < lit + 40 or len(b) % 8:
        b.append(b[-8])
    fr = Frame().add("c", from_bytes(b), None, res=capi.DEVICE)
    path, path0, info = write_both(tmp_path, "lit%d" % lit, fr, page_rows=64, row_group_rows=64)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]
    assert vals[0] == (LIT, lit, 0, 0, tag)
    assert all(e[0] == COPY and e[2] == 8 for e in vals[1:]) and sum(e[1] for e in vals[1:]) == len(b) - lit


# ------------------------------------------------------------------ 3. copy forms
@pytest.mark.parametrize("length", [4, 5, 11, 12, 63, 64, 65, 66, 67, 68, 127, 131, 132, 200])
def test_match_of_any_length_splits_into_copies_of_4_to_64(tmp_path, length):
    """24 random bytes, `length` bytes that repeat what lies 8 back, one byte that does not, random bytes to the end"""
    rng = np.random.default_rng(400 + length)
    b = bytearray(rng.integers(0, 256, 24, dtype=np.uint8).tobytes())
    for _ in range(length):
        b.append(b[-8])
    b.append(b[-8] ^ 0xFF)
    b += rng.integers(0, 256, (-len(b)) % 8 + 16, dtype=np.uint8).tobytes()
    fr = Frame().add("c", from_bytes(b), None)
    path, path0, info = write_both(tmp_path, "match%d" % length, fr, page_rows=64, row_group_rows=64)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]
    copies = [e for e in vals if e[0] == COPY]
    assert vals[0][:2] == (LIT, 24) and copies[0][3] == 24 and all(e[2] == 8 for e in copies)
    assert sum(e[1] for e in copies) == length and all(4 <= e[1] <= 64 for e in copies)
    assert len(copies) == -(-length // 64)   # 64 .. 64, then the rest; where the rest alone would hold 1 .. 3 bytes: 60 and rest + 4
    assert vals[len(copies) + 1][0] == LIT   # and a literal goes on behind the match


def test_constant_column_meets_the_size_condition(tmp_path):
    """8192 rows of one Float64 value in one page: per fragment 9 + 3 * ceil((F - 8) / 64) bytes, at most 0.06 of the 65 536"""
    fr = Frame().add("c", np.full(8192, 1013.25), None, res=capi.DEVICE)
    path, path0, info = write_both(tmp_path, "constant", fr, page_rows=8192, row_group_rows=8192)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]
    stream = sum(e[4] + (e[1] if e[0] == LIT else 0) for e in vals)
    assert stream == (65536 // F) * (9 + 3 * -(-(F - 8) // 64))
    assert stream <= 0.06 * 65536
    copies = [e for e in vals if e[0] == COPY]
    assert all(e[2] == 8 for e in copies) and min(e[1] for e in copies) >= 4 and max(e[1] for e in copies) == 64


def test_period_three_values_copy_at_multiples_of_24(tmp_path):
    rng = np.random.default_rng(41)
    base = rng.integers(-2 ** 63, 2 ** 63 - 1, 3, dtype=np.int64)
    fr = Frame().add("c", np.tile(base, 400)[:1100], None, res=capi.DEVICE)
    path, path0, info = write_both(tmp_path, "period3", fr, page_rows=1152, row_group_rows=1152)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]
    copies = [e for e in vals if e[0] == COPY]
    assert copies and all(e[2] % 24 == 0 for e in copies)
    assert sum(e[1] for e in vals if e[0] == LIT) <= 3 * 64   # per fragment: what is probed before the first period has been seen


def test_repeat_at_a_distance_of_2560_takes_the_two_byte_offset_form(tmp_path):
    rng = np.random.default_rng(42)
    b = bytearray(rng.integers(0, 256, 2560 + 256 + 64, dtype=np.uint8).tobytes())
    b[2560:2560 + 256] = b[0:256]
    fr = Frame().add("c", from_bytes(b), None)
    path, path0, info = write_both(tmp_path, "far", fr, page_rows=384, row_group_rows=384)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]
    copies = [e for e in vals if e[0] == COPY]
    assert copies and all(e[2] == 2560 and e[4] == 3 for e in copies)
    # (the table holds one position per hash, so the match may be found some bytes into the repeat; it then runs to its end)
    assert 2560 <= copies[0][3] < 2560 + 128 and copies[0][3] + sum(e[1] for e in copies) == 2560 + 256


def test_repeat_that_lies_in_the_previous_fragment_is_not_referenced(tmp_path):
    rng = np.random.default_rng(43)
    b = bytearray(rng.integers(0, 256, F + 1024, dtype=np.uint8).tobytes())
    b[F:F + 256] = b[F - 256:F]   # the second fragment begins with the end of the first
    fr = Frame().add("c", from_bytes(b), None, res=capi.DEVICE)
    path, path0, info = write_both(tmp_path, "previous", fr, page_rows=640, row_group_rows=640)
    vals = verify(path, path0, fr.data, fr.names, info=info)[(0, 0)][0]   # (check_elements: no copy reaches before its fragment)
    assert [(e[0], e[1], e[3]) for e in vals] == [(LIT, F, 0), (LIT, 1024, F)]


# ------------------------------------------------------------------ 4. nulls and levels
@pytest.mark.parametrize("offset", [0, 3, 13])
def test_level_forms_nulls_and_residencies(tmp_path, offset):
    rng = np.random.default_rng(50 + offset)
    n = 64 * 5 + 40
    valid = rng.random(n) >= 0.3
    valid[0:64] = True       # one run of 1
    valid[128:192] = False   # an all-null page between mixed pages
    fr = Frame()
    for k, res in enumerate(RES):
        fr.add("i%d" % res, int_values(n, rng) if k != 1 else np.full(n, 7, dtype=np.int64), valid, offset=offset, res=res)
        fr.add("f%d" % res, float_values(n, rng), valid if k else rng.random(n) >= 0.3, offset=offset, res=res, known=bool(k % 2))
    enc = [PLAIN, PLAIN, DELTA, PLAIN, PLAIN, PLAIN]
    path, path0, info = write_both(tmp_path, "levels", fr, page_rows=64, row_group_rows=192, encodings=enc)
    els = verify(path, path0, fr.data, fr.names, encodings=enc, info=info)
    assert els[(4, 0)][2] == []   # the all-null page: the preamble and the levels literal alone
    md = pq.read_metadata(path)
    pages = list(swalk.pages(path, md.row_group(0).column(4)))
    assert pages[0][2] == bytes([128, 1, 1]) and pages[2][2] == bytes([128, 1, 0])
    assert pages[1][2][1:] == np.packbits(valid[64:128], bitorder="little").tobytes()
    assert pages[2][4] == bytes([7, 6 << 2, 3, 0, 0, 0, 128, 1, 0])


# ------------------------------------------------------------------ 5. DELTA_BINARY_PACKED + SNAPPY
@pytest.mark.parametrize("n", [1, 2, 33, 129, 258])
def test_delta_pages_of_byte_lengths_that_are_no_multiple_of_8(tmp_path, n):
    rng = np.random.default_rng(60 + n)
    page = 320
    rows = 3 * page
    valid = np.zeros(rows, bool)
    valid[np.sort(rng.choice(page, n, replace=False))] = True           # page 0: n values
    valid[page:2 * page] = True                                         # page 1: a full page
    valid[2 * page + np.sort(rng.choice(page, n, replace=False))] = True
    ts = np.cumsum(rng.integers(1, 2000, rows)).astype(np.int64) + 1_600_000_000_000
    fr = Frame().add("ts", ts, valid, offset=n % 7, res=RES[n % 3]).add("c", np.full(rows, 5, dtype=np.int64), valid, res=capi.DEVICE)
    enc = [DELTA, DELTA]
    path, path0, info = write_both(tmp_path, "delta%d" % n, fr, page_rows=page, row_group_rows=2 * page, encodings=enc)
    verify(path, path0, fr.data, fr.names, encodings=enc, info=info)
    lens = [len(pg[3]) for g in range(2) for pg in walk.pages(path0, pq.read_metadata(path0).row_group(g).column(0))]
    assert n == 1 or any(k % 8 for k in lens), lens


# ------------------------------------------------------------------ 6. row groups and pages
@pytest.mark.parametrize("n,page,rg", [(1000, 64, 256), (70001, 0, 0)])
def test_row_groups_and_pages(tmp_path, n, page, rg):
    rng = np.random.default_rng(70)
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], None, res=capi.DEVICE)
    fr.add("v", np.round(np.cumsum(rng.standard_normal(n)), 2), rng.random(n) >= 0.3, offset=3, res=capi.DEVICE)
    fr.add("flag", rng.integers(0, 2, n).astype(np.int64), rng.random(n) >= 0.1, offset=9, res=capi.HOST)
    enc = [DELTA, PLAIN, PLAIN]
    path, path0, info = write_both(tmp_path, "groups", fr, page_rows=page, row_group_rows=rg, encodings=enc)
    verify(path, path0, fr.data, fr.names, encodings=enc, info=info)
    md = pq.read_metadata(path)
    assert md.num_row_groups == (4 if rg else 1) and info.data_pages == 3 * (16 if page else 2)
    assert os.path.getsize(path) < os.path.getsize(path0)


# ------------------------------------------------------------------ 7. codec 0 through the new entry point, determinism
def write_through_codec_entry(path, fr, codec, page_rows, row_group_rows, encodings, metadata):
    o = capi.ParquetWriteOptions()
    o.row_group_rows, o.page_rows, o.statistics, o.reserved = row_group_rows, page_rows, 1, 0
    enc = (C.c_int32 * len(encodings))(*encodings)
    o.encodings = C.cast(enc, C.POINTER(C.c_int32))
    keys = (C.c_char_p * len(metadata))(*[k.encode() for k in metadata])
    vals = (C.c_char_p * len(metadata))(*[v.encode() for v in metadata.values()])
    o.meta_keys, o.meta_values, o.n_meta = C.cast(keys, C.POINTER(C.c_char_p)), C.cast(vals, C.POINTER(C.c_char_p)), len(metadata)
    names = (C.c_char_p * len(fr.names))(*[nm.encode() for nm in fr.names])
    info = capi.ParquetWriteInfo()
    capi.check(capi.lib().bowgpu_parquet_write_codec(os.fsencode(path), capi._cols(fr.cols), names, len(fr.cols), C.byref(o), C.c_int32(codec), C.byref(info)))
    return info


def mixed_frame(seed, n=4000):
    rng = np.random.default_rng(seed)
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], rng.random(n) >= 0.1, offset=3, res=capi.DEVICE)
    fr.add("small", rng.integers(0, 100, n).astype(np.int64), rng.random(n) >= 0.5, offset=11, res=capi.DEVICE)
    fr.add("v", float_values(n, rng), rng.random(n) >= 0.3, offset=6, res=capi.HOST)
    return fr, [DELTA, PLAIN, PLAIN]


def test_codec_0_through_the_new_entry_point_is_the_old_file(tmp_path):
    fr, enc = mixed_frame(80)
    meta = {"k": "v"}
    old, new = str(tmp_path / "old.parquet"), str(tmp_path / "new.parquet")
    i0 = capi.write_parquet(old, fr.cols, fr.names, page_rows=128, row_group_rows=1024, encodings=enc, metadata=meta)
    i1 = write_through_codec_entry(new, fr, 0, 128, 1024, enc, meta)
    assert open(old, "rb").read() == open(new, "rb").read()
    assert [getattr(i0, k) for k, _ in i0._fields_] == [getattr(i1, k) for k, _ in i1._fields_]
    # and with no options and no info, as the old entry point takes them
    names = (C.c_char_p * 3)(*[nm.encode() for nm in fr.names])
    capi.check(capi.lib().bowgpu_parquet_write(os.fsencode(old), capi._cols(fr.cols), names, 3, None, None))
    capi.check(capi.lib().bowgpu_parquet_write_codec(os.fsencode(new), capi._cols(fr.cols), names, 3, None, C.c_int32(0), None))
    assert open(old, "rb").read() == open(new, "rb").read()


def test_two_snappy_writes_give_identical_files(tmp_path):
    fr, enc = mixed_frame(81)
    files = []
    for k in range(2):
        path = str(tmp_path / ("twice%d.parquet" % k))
        capi.write_parquet(path, fr.cols, fr.names, page_rows=1024, row_group_rows=2048, encodings=enc, metadata={"k": "v"}, codec=SNAPPY)
        files.append(open(path, "rb").read())
    assert files[0] == files[1]
    capi.write_parquet(str(tmp_path / "plain.parquet"), fr.cols, fr.names, page_rows=1024, row_group_rows=2048, encodings=enc, metadata={"k": "v"})
    verify(str(tmp_path / "twice1.parquet"), str(tmp_path / "plain.parquet"), fr.data, fr.names, encodings=enc)


# ------------------------------------------------------------------ 8. the chain
def test_chain_boolean_to_int64_on_the_device_to_a_snappy_file(tmp_path):
    rng = np.random.default_rng(90)
    n = 3000
    flags, valid = rng.random(n) < 0.2, rng.random(n) >= 0.1
    col = capi.Column(np.packbits(flags, bitorder="little"), np.packbits(valid, bitorder="little"), capi.BOOLEAN, 0, n, -1).to_device()
    as_int = capi.convert([col], [capi.INT64], out_residency=capi.DEVICE)[0]
    assert as_int.type == capi.INT64
    cols, names = [capi.out_as_column(as_int)], ["flag"]
    assert cols[0].residency == capi.DEVICE
    path, path0 = str(tmp_path / "chain.parquet"), str(tmp_path / "chain_plain.parquet")
    info = capi.write_parquet(path, cols, names, page_rows=1024, row_group_rows=2048, codec=SNAPPY)
    capi.write_parquet(path0, cols, names, page_rows=1024, row_group_rows=2048)
    verify(path, path0, [(flags.astype(np.int64), valid)], names, info=info)
    assert info.file_bytes < 0.5 * os.path.getsize(path0)


# ------------------------------------------------------------------ 9. fuzz
SEEDS = 32


def fuzz_values(kind, n, rng):
    if kind == "random":
        return int_values(n, rng) if rng.random() < 0.5 else float_values(n, rng)
    if kind == "constant":
        return np.full(n, rng.standard_normal()) if rng.random() < 0.5 else np.full(n, int(rng.integers(-10 ** 12, 10 ** 12)), dtype=np.int64)
    if kind == "flags":
        return rng.integers(0, 2, n).astype(np.int64)
    if kind == "small":
        return rng.integers(0, 100, n).astype(np.int64)
    if kind == "timestamps":
        return (1_600_000_000_000 + np.cumsum(rng.integers(1, 2000, n))).astype(np.int64)
    return np.round(20.0 + np.cumsum(0.1 * rng.standard_normal(n)), 2)   # a rounded walk


def fuzz_frame(seed):
    rng = np.random.default_rng(5000 + seed)
    ncols = int(rng.integers(1, 4))
    n = int(rng.choice([0, 1, int(rng.integers(2, 200)), int(rng.integers(200, 5001))], p=[0.03, 0.03, 0.24, 0.7]))
    page = int(rng.choice([64, 128, 512, 1024]))
    rg = page * int(rng.integers(1, 9))
    fr, enc = Frame(), []
    for i in range(ncols):
        values = fuzz_values(rng.choice(["random", "constant", "flags", "small", "timestamps", "walk"]), n, rng)
        valid = None if rng.random() < 0.2 else rng.random(n) < float(rng.choice([0.0, 0.05, 0.5, 0.95, 1.0]))
        if valid is not None and n > 2 * page and rng.random() < 0.5:
            p = int(rng.integers(0, n // page))
            valid[p * page:(p + 1) * page] = bool(rng.integers(0, 2))
        enc.append(DELTA if values.dtype == np.int64 and rng.random() < 0.5 else PLAIN)
        fr.add("c%d" % i, values, valid, offset=int(rng.integers(0, 70)), res=RES[int(rng.integers(0, 3))], known=bool(rng.integers(0, 2)))
    return fr, enc, page, rg


def test_fuzz_read_back_three_ways(tmp_path):
    ran = 0
    for seed in range(SEEDS):
        fr, enc, page, rg = fuzz_frame(seed)
        path, path0, info = write_both(tmp_path, "fuzz%d" % seed, fr, page_rows=page, row_group_rows=rg, encodings=enc)
        verify(path, path0, fr.data, fr.names, encodings=enc, info=info)
        os.remove(path)
        os.remove(path0)
        ran += 1
    assert ran == SEEDS
