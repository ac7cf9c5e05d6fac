"""RLE_DICTIONARY in bowgpu_parquet_write without a GPU: the contract's restatement (tests/parquet_dict_walk.py) proved against
pyarrow's own dictionary pages, the cap in the header and the binding under the unchanged ABI version, encoding 8 taken by the
call's checks (no device: BOWGPU_ERR_NO_DEVICE, where the parent of this change said BOWGPU_ERR_UNSUPPORTED) while encoding 2 stays
declined, and the file assembly (bow_amd/csrc/parquet_write.cpp, PqWriter::add_chunk with a dictionary) driven from host-made
dictionaries and index sections by a stand-alone C++ program built with AddressSanitizer + UBSan, whose file pyarrow and the
library's loader read back.  Every comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_dict_walk as dwalk
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, NO_DEVICE = -9, -11
DICT = capi.PARQUET_ENC_RLE_DICTIONARY


def test_header_and_binding_hold_the_cap_under_the_same_abi_version():
    src = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    assert re.search(r"#define BOWGPU_PARQUET_DICT_MAX 65536\b", src)
    assert re.search(r"#define BOWGPU_ABI_VERSION 14\b", src)
    assert capi.lib().bowgpu_abi_version() == 14
    assert capi.PARQUET_RLE_DICTIONARY == 8 and capi.PARQUET_DICT_MAX == 65536 == dwalk.DICT_MAX
    assert DICT == 1 << capi.PARQUET_RLE_DICTIONARY


# ---------------------------------------------------------------- the restatement against pyarrow
def _decoded(path, valid, g_rows):
    """every chunk of column 0 walked from its dictionary page: the values its index sections decode to against its dictionary"""
    md = pq.read_metadata(path)
    out, r = [], 0
    for g in range(md.num_row_groups):
        ch = md.row_group(g).column(0)
        dictionary, pages = dwalk.chunk_pages(path, ch)
        assert dictionary is not None
        for rows, enc, _, section in pages:
            assert enc in (2, 8)   # PLAIN_DICTIONARY (what pyarrow writes into a v1 page header) and RLE_DICTIONARY: the same bytes
            k = int(valid[r:r + rows].sum())
            idx, used = dwalk.decode_section(section, k)
            assert used == len(section) or k == 0
            out.append(dictionary[idx])
            r += rows
    assert r == len(valid)
    return np.concatenate(out)


@pytest.mark.parametrize("compression", ["none", "snappy"])
@pytest.mark.parametrize("entries", [1, 2, 3, 5, 17, 256, 257, 1000])
def test_restated_sections_decode_as_pyarrows_do(tmp_path, entries, compression):
    rng = np.random.default_rng(entries)
    n = 3000
    pool = rng.integers(-2 ** 63, 2 ** 63 - 1, entries, dtype=np.int64)
    pool[:min(entries, 4)] = np.array([-1, 0, 2 ** 63 - 1, -2 ** 63], dtype=np.int64)[:min(entries, 4)]
    for dt in (np.int64, np.float64):
        values = pool[rng.integers(0, entries, n)]
        values[:entries] = pool   # (every entry occurs)
        valid = rng.random(n) >= 0.3
        valid[:entries] = True
        valid[1024:1536] = False
        col = values.view(dt)
        path = str(tmp_path / ("pa_%s.parquet" % np.dtype(dt).name))
        pq.write_table(pa.table({"c": pa.array(col, mask=~valid)}), path, use_dictionary=True, compression=compression, data_page_version="1.0",
                       row_group_size=2048, data_page_size=1024, write_statistics=False)
        dense = values[valid].view(np.uint64)
        # pyarrow's own pages, walked and decoded here, give the values back: the walker and the decoder read the format
        assert np.array_equal(_decoded(path, valid, 2048), dense)
        # the restated bytes, decoded the same way, give them back as well
        for a in range(0, n, 2048):
            chunk = values[a:a + 2048][valid[a:a + 2048]]
            d = dwalk.expected_dictionary(chunk)
            assert d.dtype == np.uint64 and np.all(d[1:] > d[:-1]) and set(d.tolist()) == set(chunk.view(np.uint64).tolist())
            for b in range(0, len(chunk) + 1, 100):   # pages of 100 values, a short last one, an empty one at the end
                page = chunk[b:b + 100]
                s = dwalk.expected_section(page, d)
                k = len(page)
                w = dwalk.width_of(len(d))
                assert s[0] == w and len(s) == (1 if k == 0 else 1 + len(_uleb((((k + 7) // 8) << 1) | 1)) + ((k + 7) // 8) * w)
                idx, used = dwalk.decode_section(s, k)
                assert used == len(s) or k == 0
                assert np.array_equal(d[idx], page.view(np.uint64))


def _uleb(v):
    out = b""
    while v >= 0x80:
        out, v = out + bytes([(v & 0x7f) | 0x80]), v >> 7
    return out + bytes([v])


def test_the_order_is_unsigned_for_both_types():
    i = np.array([5, -1, 0, -2 ** 63, 2 ** 63 - 1, -1], dtype=np.int64)
    assert dwalk.expected_dictionary(i).view(np.int64).tolist() == [0, 5, 2 ** 63 - 1, -2 ** 63, -1]
    f = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], dtype=np.float64)
    assert dwalk.expected_dictionary(f).view(np.float64).tolist() == [0.0, 1.0, np.inf, -0.0, -1.0, -np.inf]
    assert [dwalk.width_of(k) for k in (1, 2, 3, 4, 5, 255, 256, 257, 65535, 65536)] == [1, 1, 2, 2, 3, 8, 8, 9, 16, 16]


# ---------------------------------------------------------------- the call's checks
def _col(n=100, typ=capi.INT64):
    return capi.Column(np.arange(n, dtype=np.int64 if typ == capi.INT64 else np.float64) % 7)


def _no_gpu():
    try:
        return capi.device_count() == 0
    except capi.BowGpuError:
        return True


@pytest.mark.parametrize("codec", [capi.PARQUET_CODEC_UNCOMPRESSED, capi.PARQUET_CODEC_SNAPPY])
@pytest.mark.parametrize("typ", [capi.INT64, capi.FLOAT64], ids=["int64", "float64"])
def test_encoding_8_passes_the_checks_and_needs_a_device(tmp_path, typ, codec):
    if not _no_gpu():
        return   # (tests/test_gpu_parquet_dictionary.py is this box's half)
    for rows in (0, 100):
        with pytest.raises(capi.BowGpuError) as e:
            capi.write_parquet(str(tmp_path / "x.parquet"), [_col(rows, typ), _col(rows)], ["a", "b"], page_rows=64, row_group_rows=128,
                               encodings=[capi.PARQUET_RLE_DICTIONARY, capi.PARQUET_PLAIN], codec=codec)
        assert e.value.code == NO_DEVICE, e.value
        assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("codec", [capi.PARQUET_CODEC_UNCOMPRESSED, capi.PARQUET_CODEC_SNAPPY])
def test_plain_dictionary_and_the_other_declines_stay(tmp_path, codec):
    for cols, enc in (([_col()], [2]), ([_col(), _col()], [8, 2]), ([_col()], [9]), ([_col()], [-1]), ([_col(), _col(typ=capi.FLOAT64)], [8, 5]),
                      ([_col(), capi.Column(np.zeros(100, np.uint8), None, capi.BOOLEAN, 0, 100)], [8, 8])):
        with pytest.raises(capi.BowGpuError) as e:
            capi.write_parquet(str(tmp_path / "x.parquet"), cols, ["c%d" % i for i in range(len(cols))], encodings=enc, codec=codec)
        assert e.value.code == UNSUPPORTED, (enc, e.value)
        assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------- the file assembly, sanitized
GROUP_PAGES = [[64, 64, 40], [24]]   # tests/cpp/test_parquet_dict_assemble.cpp


def _valid(col, group, page, r):
    if group == 1:
        return r % 2 == 0 if col == 0 else True
    if col == 0:
        return True if page == 0 else False if page == 1 else r % 3 != 0
    return r % 5 != 1 if page == 0 else page == 1


def _value(col, group, r):
    if col == 0:
        return ((7 * r) % 5) * 1000 - 2000 if group == 0 else r % 3 - 1
    return 0.25 * (r % 9) if group == 0 else 0.5 * r


@pytest.fixture(scope="module")
def assemble_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dict_assemble") / "test_parquet_dict_assemble")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DBOWGPU_PARQUET_ASSEMBLE_ONLY", os.path.join(ROOT, "tests", "cpp", "test_parquet_dict_assemble.cpp"),
                           os.path.join(ROOT, "bow_amd", "csrc", "parquet_write.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("codec", [0, 1], ids=["uncompressed", "snappy"])
def test_sanitized_dictionary_assembly_program_writes_what_pyarrow_reads(tmp_path, assemble_exe, codec):
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    path = str(out_dir / "assembled.parquet")
    p = subprocess.run([assemble_exe, path, str(codec)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.listdir(str(out_dir)) == ["assembled.parquet"]   # no temporary, neither of the finished nor of the declined writers
    totals = dict(zip(p.stdout.split()[0::2], map(int, p.stdout.split()[1::2])))

    valid, want = [[], []], [[], []]
    for g, plist in enumerate(GROUP_PAGES):
        r0 = sum(sum(q) for q in GROUP_PAGES[:g])
        for col in range(2):
            r = r0
            for pg, n in enumerate(plist):
                valid[col] += [_valid(col, g, pg, r + k) for k in range(n)]
                want[col] += [_value(col, g, r + k) for k in range(n)]
                r += n
    rows = len(valid[0])
    valid = [np.array(v, dtype=bool) for v in valid]
    want = [np.array(want[0], dtype=np.int64), np.array(want[1], dtype=np.float64)]

    f = pq.ParquetFile(path)
    md = f.metadata
    assert md.num_rows == rows == 192 and md.num_row_groups == 2 and md.num_columns == 2
    table = f.read()
    for i in range(2):
        col = table.column(i).combine_chunks()
        assert np.array_equal(np.asarray(col.is_valid()), valid[i])
        got = col.to_numpy(zero_copy_only=False)
        assert np.array_equal(np.asarray(got[valid[i]], dtype=want[i].dtype).view(np.uint64), want[i][valid[i]].view(np.uint64))
    a, chunk_end, level_bytes, value_bytes, dict_bytes, npages = 0, 4, 0, 0, 0, 0
    for g in range(2):
        b = a + md.row_group(g).num_rows
        raw_group = 0
        for i in range(2):
            ch = md.row_group(g).column(i)
            ok, v = valid[i][a:b], want[i][a:b]
            plain = (g, i) == (1, 1)
            assert ch.physical_type == ("INT64", "DOUBLE")[i] and ch.compression == ("UNCOMPRESSED", "SNAPPY")[codec] and ch.num_values == b - a
            assert ch.encodings == (("PLAIN", "RLE") if plain else ("RLE_DICTIONARY", "PLAIN", "RLE"))
            st = ch.statistics
            assert st.null_count == int((~ok).sum()) and st.has_min_max and st.min == v[ok].min() and st.max == v[ok].max()
            # the chunks lie end to end from byte 4 on; a dictionary chunk starts at its dictionary page, both totals count it in
            assert ch.has_dictionary_page == (not plain)
            if plain:
                assert ch.data_page_offset == chunk_end
            else:
                assert ch.dictionary_page_offset == chunk_end and ch.data_page_offset >= ch.dictionary_page_offset + 4
            chunk_end += ch.total_compressed_size
            raw_group += ch.total_uncompressed_size
            dictionary, pages = dwalk.chunk_pages(path, ch)   # (checks both totals against the pages it walks)
            assert [pg[0] for pg in pages] == GROUP_PAGES[g]
            if plain:
                assert dictionary is None
            else:
                assert np.array_equal(dictionary, dwalk.expected_dictionary(v[ok]))
                dict_bytes += 8 * len(dictionary)
                if codec == 0:
                    assert ch.total_compressed_size == ch.total_uncompressed_size
            r = a
            for pg in pages:
                okp, vp = valid[i][r:r + pg[0]], want[i][r:r + pg[0]]
                assert pg[1] == (0 if plain else 8)
                assert pg[3] == (vp[okp].tobytes() if plain else dwalk.expected_section(vp[okp], dictionary))
                level_bytes += 4 + len(pg[2])
                value_bytes += len(pg[3])
                r += pg[0]
            npages += len(pages)
        assert md.row_group(g).total_byte_size == raw_group
        a = b
    with open(path, "rb") as fh:
        fh.seek(-8, os.SEEK_END)
        footer = int.from_bytes(fh.read(4), "little")
    assert chunk_end + footer + 8 == os.path.getsize(path)
    assert totals["file_bytes"] == os.path.getsize(path) and totals["rows"] == rows and totals["row_groups"] == 2
    assert totals["data_pages"] == npages == 8                     # data pages only
    assert totals["dict_bytes"] == dict_bytes == 8 * (5 + 9 + 3)
    assert totals["value_bytes"] == value_bytes + dict_bytes       # the dictionary pages' bodies count as values
    assert totals["level_bytes"] == level_bytes

    # the library's own footer and page-header parser (no device): the chunk structure holds, and the masks say what each column holds
    lf = capi.ParquetFile(path)
    assert lf.num_rows == rows
    assert lf.check_column(0) == DICT
    assert lf.check_column(1) == DICT | capi.PARQUET_ENC_PLAIN
    lf.close()
