"""bowgpu_parquet_write_codec without a GPU: the symbol in the header and the binding under the unchanged ABI version, the codecs
it declines, every decline of bowgpu_parquet_write through the new entry point, and the SNAPPY file assembly
(bow_amd/csrc/parquet_write.cpp, PqWriter::add_chunk with codec 1) driven from host-made element streams by a stand-alone C++
program built with AddressSanitizer + UBSan, whose file pyarrow reads back."""
import os
import re
import subprocess

import numpy as np
import pyarrow.parquet as pq
import pytest

import parquet_snappy_walk as swalk
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPPY = capi.PARQUET_CODEC_SNAPPY
UNSUPPORTED, ARG, NO_DEVICE = -9, -10, -11


def test_header_and_binding_hold_the_symbol_under_the_same_abi_version():
    src = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bowgpu_parquet_write_codec\s*\(", src)
    assert re.search(r"\bint\s+bowgpu_parquet_write\s*\(", src)
    assert "bowgpu_parquet_write_codec" in capi.SYMBOLS and "bowgpu_parquet_write" in capi.SYMBOLS
    assert hasattr(capi.lib(), "bowgpu_parquet_write_codec")
    assert re.search(r"#define BOWGPU_ABI_VERSION 14\b", src)
    assert capi.lib().bowgpu_abi_version() == 14
    assert SNAPPY == 1


def _col(n=100, typ=capi.INT64):
    if typ in (capi.INT64, capi.FLOAT64):
        return capi.Column(np.arange(n, dtype=np.int64 if typ == capi.INT64 else np.float64))
    return capi.Column(np.zeros(max(n, 8), np.uint8), None, typ, 0, n)


@pytest.mark.parametrize("codec", [2, -1, 3, 6, 1 << 20])
def test_other_codecs_are_unsupported_and_leave_nothing(tmp_path, codec):
    with pytest.raises(capi.BowGpuError) as e:
        capi.write_parquet(str(tmp_path / "x.parquet"), [_col(), _col(typ=capi.FLOAT64)], ["a", "b"], codec=codec)
    assert e.value.code == UNSUPPORTED, e.value
    assert os.listdir(str(tmp_path)) == []


# the declines of bowgpu_parquet_write (tests/test_parquet_write_cpu.py, DECLINES), restated
DECLINES = [
    ("boolean column", UNSUPPORTED, lambda: dict(cols=[_col(), _col(typ=capi.BOOLEAN)], names=["a", "b"])),
    ("string column", UNSUPPORTED, lambda: dict(cols=[_col(typ=capi.STRING)], names=["a"])),
    ("delta on float64", UNSUPPORTED, lambda: dict(cols=[_col(), _col(typ=capi.FLOAT64)], names=["a", "b"], encodings=[5, 5])),
    ("byte stream split", UNSUPPORTED, lambda: dict(cols=[_col()], names=["a"], encodings=[9])),
    ("negative encoding", UNSUPPORTED, lambda: dict(cols=[_col()], names=["a"], encodings=[-1])),
    ("unequal lengths", ARG, lambda: dict(cols=[_col(100), _col(99)], names=["a", "b"])),
    ("no column", ARG, lambda: dict(cols=[], names=[])),
    ("null name", ARG, lambda: dict(cols=[_col()], names=[None])),
    ("empty name", ARG, lambda: dict(cols=[_col(), _col()], names=["a", ""])),
    ("name twice", ARG, lambda: dict(cols=[_col(), _col(), _col()], names=["a", "b", "a"])),
    ("page_rows no multiple of 64", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=100)),
    ("page_rows negative", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=-64)),
    ("page_rows too large", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=(1 << 20) + 64)),
    ("row group no multiple of the page", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=128, row_group_rows=192)),
    ("row group below the default page", ARG, lambda: dict(cols=[_col()], names=["a"], row_group_rows=128)),
    ("row group too large", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=1 << 20, row_group_rows=(1 << 27) + (1 << 20))),
    ("row group negative", ARG, lambda: dict(cols=[_col()], names=["a"], page_rows=64, row_group_rows=-64)),
    ("reserved", ARG, lambda: dict(cols=[_col()], names=["a"], reserved=1)),
]


@pytest.mark.parametrize("what,code,make", DECLINES, ids=[d[0] for d in DECLINES])
def test_declines_of_the_writer_come_back_through_the_codec_entry_point(tmp_path, what, code, make):
    with pytest.raises(capi.BowGpuError) as e:
        capi.write_parquet(str(tmp_path / "declined.parquet"), codec=SNAPPY, **make())
    assert e.value.code == code, (what, e.value)
    assert os.listdir(str(tmp_path)) == []


def test_well_formed_snappy_call_without_a_gpu_is_no_device(tmp_path):
    try:
        n = capi.device_count()
    except capi.BowGpuError:
        n = 0
    if n > 0:
        return   # (tests/test_gpu_parquet_snappy.py is this box's half)
    for rows in (0, 100):
        with pytest.raises(capi.BowGpuError) as e:
            capi.write_parquet(str(tmp_path / "x.parquet"), [_col(rows), _col(rows, capi.FLOAT64)], ["a", "b"], page_rows=64, row_group_rows=128,
                               encodings=[5, 0], metadata={"k": "v"}, codec=SNAPPY)
        assert e.value.code == NO_DEVICE
        assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------- the file assembly, sanitized, from host-made element streams
GROUP_PAGES = [[64, 64, 40], [24]]   # tests/cpp/test_parquet_snappy_assemble.cpp


def _valid(col, group, page, r):
    if group == 1:
        return r % 2 == 0 if col == 0 else True
    if col == 0:
        return True if page == 0 else False if page == 1 else r % 3 != 0
    return r % 5 != 1 if page == 0 else page == 1


def test_walker_parses_the_element_forms():
    lit70 = bytes(range(70))
    stream = bytes([80]) + bytes([60 << 2, 69]) + lit70 + bytes([1 | (2 << 2) | (1 << 5), 4]) + bytes([2 | (3 << 2), 70, 0])
    size, els = swalk.elements(stream)
    assert size == 80
    assert els == [(swalk.LITERAL, 70, 0, 0, 2), (swalk.COPY, 6, 260, 70, 2), (swalk.COPY, 4, 70, 76, 3)]


def test_sanitized_snappy_assembly_program_writes_what_pyarrow_reads(tmp_path):
    exe = str(tmp_path / "test_parquet_snappy_assemble")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DBOWGPU_PARQUET_ASSEMBLE_ONLY", os.path.join(ROOT, "tests", "cpp", "test_parquet_snappy_assemble.cpp"),
                           os.path.join(ROOT, "bow_amd", "csrc", "parquet_write.cpp"), "-o", exe])
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    path = str(out_dir / "assembled.parquet")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.listdir(str(out_dir)) == ["assembled.parquet"]   # no temporary, neither of the finished nor of the declined writer
    totals = dict(zip(p.stdout.split()[0::2], map(int, p.stdout.split()[1::2])))

    valid = [[], []]
    for g, plist in enumerate(GROUP_PAGES):
        r0 = sum(sum(q) for q in GROUP_PAGES[:g])
        for col in range(2):
            r = r0
            for pg, n in enumerate(plist):
                valid[col] += [_valid(col, g, pg, r + k) for k in range(n)]
                r += n
    rows = len(valid[0])
    valid = [np.array(v, dtype=bool) for v in valid]
    want = [1000 * np.arange(rows, dtype=np.int64) - 5, np.full(rows, 2.5)]

    f = pq.ParquetFile(path)
    md = f.metadata
    assert md.num_rows == rows == 192 and md.num_row_groups == 2 and md.num_columns == 2
    assert [md.row_group(g).num_rows for g in range(2)] == [168, 24]
    table = f.read()
    for i in range(2):
        col = table.column(i).combine_chunks()
        assert np.array_equal(np.asarray(col.is_valid()), valid[i])
        got = col.to_numpy(zero_copy_only=False)
        assert np.array_equal(np.asarray(got[valid[i]], dtype=want[i].dtype).view(np.uint64), want[i][valid[i]].view(np.uint64))
    a = level_bytes = comp_values = chunk_end = 0
    kinds = set()
    for g in range(2):
        b = a + md.row_group(g).num_rows
        raw_group = 0
        for i in range(2):
            ch = md.row_group(g).column(i)
            assert ch.physical_type == ("INT64", "DOUBLE")[i] and ch.compression == "SNAPPY" and "PLAIN" in ch.encodings
            assert ch.num_values == b - a
            st, ok = ch.statistics, valid[i][a:b]
            assert st.null_count == int((~ok).sum())
            assert st.has_min_max and st.min == want[i][a:b][ok].min() and st.max == want[i][a:b][ok].max()
            # the chunks lie end to end from byte 4 on: total_compressed_size is the chunk's bytes in the file, and the walker checks
            # that the page headers and sections fill exactly that and that header + uncompressed sizes sum to total_uncompressed_size
            assert ch.data_page_offset == (chunk_end or 4)
            chunk_end = ch.data_page_offset + ch.total_compressed_size
            raw_group += ch.total_uncompressed_size
            pages = list(swalk.pages(path, ch))
            assert [pg[0] for pg in pages] == GROUP_PAGES[g]
            r = a
            for pg in pages:
                okp, v = valid[i][r:r + pg[0]], want[i][r:r + pg[0]]
                k = int(okp.sum())
                kinds.add("all" if k == pg[0] else "none" if k == 0 else "mixed")
                assert pg[3] == v[okp].tobytes()
                vals = swalk.values_elements(pg[5], len(pg[2]))
                assert (len(vals) == 0) == (k == 0)          # a page without a valid row: the preamble and the levels literal alone
                if i == 0 and g == 1:
                    assert [(e[0], e[1]) for e in vals] == [(swalk.LITERAL, 96)]
                if i == 1 and k * 8 > 128:
                    assert len(vals) > 2 and {e[2] for e in vals if e[0] == swalk.COPY} == {8}
                level_bytes += 4 + len(pg[2])
                comp_values += sum(e[1] + e[4] if e[0] == swalk.LITERAL else e[4] for e in vals)
                r += pg[0]
        assert md.row_group(g).total_byte_size == raw_group
        a = b
    assert kinds == {"all", "none", "mixed"}
    with open(path, "rb") as fh:
        fh.seek(-8, os.SEEK_END)
        footer = int.from_bytes(fh.read(4), "little")
    assert chunk_end + footer + 8 == os.path.getsize(path)
    assert totals["file_bytes"] == os.path.getsize(path) and totals["rows"] == rows and totals["row_groups"] == 2 and totals["data_pages"] == 8
    assert totals["value_bytes"] == 8 * int(valid[0].sum() + valid[1].sum())     # the uncompressed section sizes
    assert totals["level_bytes"] == level_bytes
    assert totals["comp_bytes"] == comp_values
