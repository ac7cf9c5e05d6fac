"""bowgpu_parquet_write_bool without a GPU: the symbol in the header, the binding and the library, every decline with its code
before any device is touched (and nothing left in the directory), and the file assembly with a BOOLEAN column
(bow_amd/csrc/parquet_write.cpp, PqWriter) driven from host-made page bodies by a stand-alone C++ program built with
AddressSanitizer + UBSan, whose two files - stored and SNAPPY - pyarrow reads back."""
import os
import re
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_bool_pages as pb
import parquet_page_walk as walk
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_hold_the_symbol():
    src = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bowgpu_parquet_write_bool\s*\(", src)
    assert "bowgpu_parquet_write_bool" in capi.SYMBOLS
    assert hasattr(capi.lib(), "bowgpu_parquet_write_bool")
    assert re.search(r"#define BOWGPU_ABI_VERSION 14\b", src) and capi.lib().bowgpu_abi_version() == 14


def _col(n=100, typ=capi.INT64):
    if typ in (capi.INT64, capi.FLOAT64):
        return capi.Column(np.arange(n, dtype=np.int64 if typ == capi.INT64 else np.float64))
    return capi.Column(np.zeros(max(n, 8), np.uint8), None, typ, 0, n)


def _flag(n=100):
    return _col(n, capi.BOOLEAN)


UNSUPPORTED, ARG, NO_DEVICE = -9, -10, -11
DECLINES = [
    ("boolean rle", UNSUPPORTED, lambda: dict(cols=[_col(), _flag()], names=["a", "b"], encodings=[0, 3])),
    ("boolean delta", UNSUPPORTED, lambda: dict(cols=[_col(), _flag()], names=["a", "b"], encodings=[5, 5])),
    ("boolean dictionary", UNSUPPORTED, lambda: dict(cols=[_flag(), _col()], names=["b", "a"], encodings=[8, 8])),
    ("boolean negative encoding", UNSUPPORTED, lambda: dict(cols=[_flag()], names=["b"], encodings=[-1])),
    ("string column", UNSUPPORTED, lambda: dict(cols=[_flag(), _col(typ=capi.STRING)], names=["b", "s"])),
    ("codec 2", UNSUPPORTED, lambda: dict(cols=[_col(), _flag()], names=["a", "b"], codec=2)),
    ("unequal lengths", ARG, lambda: dict(cols=[_flag(100), _col(99)], names=["b", "a"])),
    ("boolean shorter", ARG, lambda: dict(cols=[_col(100), _flag(99)], names=["a", "b"])),
    ("null name", ARG, lambda: dict(cols=[_flag()], names=[None])),
    ("empty name", ARG, lambda: dict(cols=[_col(), _flag()], names=["a", ""])),
    ("name twice", ARG, lambda: dict(cols=[_flag(), _col(), _flag()], names=["b", "a", "b"])),
    ("page_rows no multiple of 64", ARG, lambda: dict(cols=[_flag()], names=["b"], page_rows=100)),
    ("page_rows too large", ARG, lambda: dict(cols=[_flag()], names=["b"], page_rows=(1 << 20) + 64)),
    ("row group no multiple of the page", ARG, lambda: dict(cols=[_flag()], names=["b"], page_rows=128, row_group_rows=192)),
    ("row group below the default page", ARG, lambda: dict(cols=[_flag()], names=["b"], row_group_rows=128)),
    ("row group too large", ARG, lambda: dict(cols=[_flag()], names=["b"], page_rows=1 << 20, row_group_rows=(1 << 27) + (1 << 20))),
    ("reserved", ARG, lambda: dict(cols=[_col(), _flag()], names=["a", "b"], reserved=1)),
]


@pytest.mark.parametrize("what,code,make", DECLINES, ids=[d[0] for d in DECLINES])
def test_declines_come_back_before_any_device_and_leave_nothing(tmp_path, what, code, make):
    path = str(tmp_path / "declined.parquet")
    with pytest.raises(capi.BowGpuError) as e:
        capi.write_parquet(path, booleans=True, **make())
    assert e.value.code == code, (what, e.value)
    if what.startswith("boolean ") and code == UNSUPPORTED:
        assert "'b'" in e.value.message, e.value.message   # the column is named
    assert os.listdir(str(tmp_path)) == []


def test_well_formed_call_without_a_gpu_is_no_device(tmp_path):
    try:
        n = capi.device_count()
    except capi.BowGpuError:
        n = 0
    if n > 0:
        return   # (tests/test_gpu_parquet_bool_write.py is this box's half)
    for rows in (0, 100):
        for codec in (0, 1):
            with pytest.raises(capi.BowGpuError) as e:
                capi.write_parquet(str(tmp_path / "x.parquet"), [_col(rows), _flag(rows)], ["a", "b"], page_rows=64, row_group_rows=128,
                                   encodings=[5, 0], metadata={"k": "v"}, codec=codec, booleans=True)
            assert e.value.code == NO_DEVICE
            assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------- the file assembly, sanitized, from host-made page bodies
GROUP_PAGES = [[64, 64, 40], [24]]   # tests/cpp/test_parquet_bool_assemble.cpp


def _valid(group, page, r):
    if group == 1:
        return r % 2 == 0
    return True if page == 0 else False if page == 1 else r % 3 != 0


def test_sanitized_assembly_program_writes_what_pyarrow_reads(tmp_path):
    exe = str(tmp_path / "test_parquet_bool_assemble")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DBOWGPU_PARQUET_ASSEMBLE_ONLY", os.path.join(ROOT, "tests", "cpp", "test_parquet_bool_assemble.cpp"),
                           os.path.join(ROOT, "bow_amd", "csrc", "parquet_write.cpp"), "-o", exe])
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    p = subprocess.run([exe, str(out_dir)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(str(out_dir))) == ["snappy.parquet", "stored.parquet"]   # no temporary, neither of a finished nor of the abandoned writer
    lines = p.stdout.splitlines()
    assert len(lines) == 2

    valid = []
    r = 0
    for g, plist in enumerate(GROUP_PAGES):
        for pg, n in enumerate(plist):
            valid += [_valid(g, pg, r + k) for k in range(n)]
            r += n
    rows = len(valid)
    valid = np.array(valid, dtype=bool)
    flags = (7 * np.arange(rows)) % 5 < 2
    ts = 1000 * np.arange(rows, dtype=np.int64) - 5
    ks = [[64, 0, 27], [12]]   # valid rows per page: all, none, k % 8 != 0 twice
    bounds = [(0, 168), (168, 192)]

    # pyarrow's own statistics for the same rows, one reference file per row group
    want_stats = []
    for a, b in bounds:
        ref = str(tmp_path / ("ref%d.parquet" % a))
        pq.write_table(pa.table({"flag": pa.array(flags[a:b], mask=~valid[a:b])}), ref, use_dictionary=False, compression="none")
        want_stats.append(pq.read_metadata(ref).row_group(0).column(0).statistics)

    for line, name, compression in zip(lines, ("stored.parquet", "snappy.parquet"), ("UNCOMPRESSED", "SNAPPY")):
        path = str(out_dir / name)
        totals = dict(zip(line.split()[0::2], map(int, line.split()[1::2])))
        f = pq.ParquetFile(path)
        md = f.metadata
        assert md.num_rows == rows == 192 and md.num_row_groups == 2 and md.num_columns == 2
        assert [md.schema.column(i).name for i in range(2)] == ["t", "flag"]
        assert [md.schema.column(i).physical_type for i in range(2)] == ["INT64", "BOOLEAN"]
        assert all(md.schema.column(i).max_definition_level == 1 and md.schema.column(i).max_repetition_level == 0 for i in range(2))
        assert f.schema_arrow.field(1).type == pa.bool_() and f.schema_arrow.field(1).nullable
        table = f.read()
        assert np.array_equal(np.asarray(table.column("t").combine_chunks()), ts) and table.column("t").null_count == 0
        gv, gm = pb.read_back(path, "flag")
        assert np.array_equal(gm, valid) and np.array_equal(gv, flags & valid)
        footer = open(path, "rb").read()
        for g, (a, b) in enumerate(bounds):
            ch = md.row_group(g).column(1)
            assert ch.physical_type == "BOOLEAN" and ch.compression == compression and set(ch.encodings) == {"PLAIN", "RLE"}
            assert ch.num_values == b - a
            st, want = ch.statistics, want_stats[g]
            assert st.null_count == want.null_count == int((~valid[a:b]).sum())
            assert st.has_min_max and want.has_min_max and (st.min, st.max) == (want.min, want.max) == (False, True)
            if compression == "UNCOMPRESSED":
                pages = list(walk.pages(path, ch))
                assert [pg[0] for pg in pages] == GROUP_PAGES[g] and all(pg[1] == pb.PLAIN for pg in pages)
                r0 = a
                for pg, n, k in zip(pages, GROUP_PAGES[g], ks[g]):
                    ok = valid[r0:r0 + n]
                    assert int(ok.sum()) == k and pg[3] == pb.plain_bits(flags[r0:r0 + n][ok]) and len(pg[3]) == (k + 7) // 8
                    r0 += n
        # Statistics of a BOOLEAN chunk in the footer's Thrift: null_count, then max_value (field 5) and min_value (field 6) as
        # binaries of ONE byte, then the struct's stop byte
        assert footer.count(bytes([0x28, 1, 1, 0x18, 1, 0, 0])) == 2
        assert totals["file_bytes"] == os.path.getsize(path) and totals["rows"] == rows and totals["row_groups"] == 2 and totals["data_pages"] == 8
        assert totals["value_bytes"] == 8 * rows + sum((k + 7) // 8 for g in ks for k in g)
