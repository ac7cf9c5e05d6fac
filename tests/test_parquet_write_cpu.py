"""bowgpu_parquet_write without a GPU: the page-walk helper against files whose page bodies are known, the symbol in the header
and the binding, every decline with its code before any device is touched (and nothing left in the directory), and the file
assembly (bow_amd/csrc/parquet_write.cpp, PqWriter) driven from host-made page bodies by a stand-alone C++ program built with
AddressSanitizer + UBSan, whose file pyarrow reads back."""
import os
import re
import subprocess

import numpy as np
import pyarrow.parquet as pq
import pytest

import parquet_page_walk as walk
import parquet_pages as pp
from bow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_page_walk_returns_the_bodies_that_went_in(tmp_path):
    rng = np.random.default_rng(1)
    ts = np.cumsum(rng.integers(1, 20, 700)).astype(np.int64)
    for optional in (False, True):
        def v(n):
            return (rng.random(n) >= 0.3) if optional else None
        pages = [(pp.PLAIN, ts[:100], v(100)), (pp.DELTA_BINARY_PACKED, ts[100:500], v(400), {"block_size": 128, "miniblocks": 4}),
                 (pp.PLAIN, ts[500:501], v(1)), (pp.DELTA_BINARY_PACKED, ts[501:], v(199))]
        path = str(tmp_path / ("walk%d.parquet" % optional))
        pp.write_file(path, pages, optional=optional)
        chunk = pq.read_metadata(path).row_group(0).column(0)
        got = list(walk.pages(path, chunk, optional=optional))
        assert len(got) == len(pages)
        for (num, enc, lv, body), pg in zip(got, pages):
            valid = np.ones(len(pg[1]), dtype=bool) if pg[2] is None else pg[2]
            assert (num, enc) == (len(pg[1]), pg[0])
            assert lv == (pp._levels(valid)[4:] if optional else b"")
            assert body == pp.ENCODERS[pg[0]](pg[1][valid], **(pg[3] if len(pg) > 3 else {}))


def test_header_and_binding_hold_the_symbol():
    src = open(os.path.join(ROOT, "include", "bowgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+bowgpu_parquet_write\s*\(", src)
    assert "bowgpu_parquet_write_options" in src and "bowgpu_parquet_write_info" in src
    assert "bowgpu_parquet_write" in capi.SYMBOLS
    assert hasattr(capi.lib(), "bowgpu_parquet_write")
    assert re.search(r"#define BOWGPU_ABI_VERSION 14\b", src)


def _col(n=100, typ=capi.INT64):
    if typ in (capi.INT64, capi.FLOAT64):
        return capi.Column(np.arange(n, dtype=np.int64 if typ == capi.INT64 else np.float64))
    return capi.Column(np.zeros(max(n, 8), np.uint8), None, typ, 0, n)


UNSUPPORTED, ARG, NO_DEVICE = -9, -10, -11
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
def test_declines_come_back_before_any_device_and_leave_nothing(tmp_path, what, code, make):
    path = str(tmp_path / "declined.parquet")
    with pytest.raises(capi.BowGpuError) as e:
        capi.write_parquet(path, **make())
    assert e.value.code == code, (what, e.value)
    assert os.listdir(str(tmp_path)) == []


def test_well_formed_call_without_a_gpu_is_no_device(tmp_path):
    try:
        n = capi.device_count()
    except capi.BowGpuError:
        n = 0
    if n > 0:
        return   # (tests/test_gpu_parquet_write.py is this box's half)
    for rows in (0, 100):
        with pytest.raises(capi.BowGpuError) as e:
            capi.write_parquet(str(tmp_path / "x.parquet"), [_col(rows), _col(rows, capi.FLOAT64)], ["a", "b"], page_rows=64, row_group_rows=128,
                               encodings=[5, 0], metadata={"k": "v"})
        assert e.value.code == NO_DEVICE
        assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------- the file assembly, sanitized, from host-made page bodies
GROUP_PAGES = [[64, 64, 40], [24]]   # tests/cpp/test_parquet_assemble.cpp


def _valid(col, group, page, r):
    if group == 1:
        return r % 2 == 0 if col == 0 else True
    if col == 0:
        return True if page == 0 else False if page == 1 else r % 3 != 0
    return r % 5 != 1 if page == 0 else page == 1


def test_sanitized_assembly_program_writes_what_pyarrow_reads(tmp_path):
    exe = str(tmp_path / "test_parquet_assemble")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-DBOWGPU_PARQUET_ASSEMBLE_ONLY", os.path.join(ROOT, "tests", "cpp", "test_parquet_assemble.cpp"),
                           os.path.join(ROOT, "bow_amd", "csrc", "parquet_write.cpp"), "-o", exe])
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    path = str(out_dir / "assembled.parquet")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert os.listdir(str(out_dir)) == ["assembled.parquet"]   # no temporary, neither of the finished nor of the abandoned writer
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
    want = [1000 * np.arange(rows, dtype=np.int64) - 5, 0.5 * np.arange(rows, dtype=np.float64) - 10.0]

    f = pq.ParquetFile(path)
    md = f.metadata
    assert md.num_rows == rows == 192 and md.num_row_groups == 2 and md.num_columns == 2
    assert [md.row_group(g).num_rows for g in range(2)] == [168, 24]
    assert md.metadata[b"origin"] == b"assemble" and md.metadata[b"empty"] == b""
    assert md.created_by.startswith("bowgpu")
    assert [md.schema.column(i).name for i in range(2)] == ["t", "v"]
    assert [md.schema.column(i).physical_type for i in range(2)] == ["INT64", "DOUBLE"]
    assert all(md.schema.column(i).max_definition_level == 1 and md.schema.column(i).max_repetition_level == 0 for i in range(2))   # OPTIONAL, flat
    assert all(f.schema_arrow.field(i).nullable for i in range(2))
    table = f.read()
    for i in range(2):
        col = table.column(i).combine_chunks()
        assert np.array_equal(np.asarray(col.is_valid()), valid[i])
        got = col.to_numpy(zero_copy_only=False)
        assert np.array_equal(np.asarray(got[valid[i]], dtype=want[i].dtype).view(np.uint64), want[i][valid[i]].view(np.uint64))
    a = 0
    for g in range(2):
        b = a + md.row_group(g).num_rows
        for i in range(2):
            ch = md.row_group(g).column(i)
            assert ch.physical_type == ("INT64", "DOUBLE")[i] and ch.compression == "UNCOMPRESSED" and "PLAIN" in ch.encodings
            assert ch.num_values == b - a
            st, ok = ch.statistics, valid[i][a:b]
            assert st.null_count == int((~ok).sum())
            assert st.has_min_max and st.min == want[i][a:b][ok].min() and st.max == want[i][a:b][ok].max()
            pages = list(walk.pages(path, ch))
            assert [pg[0] for pg in pages] == GROUP_PAGES[g]
        a = b
    assert totals["file_bytes"] == os.path.getsize(path) and totals["rows"] == rows and totals["row_groups"] == 2 and totals["data_pages"] == 8
    assert totals["value_bytes"] == 8 * int(valid[0].sum() + valid[1].sum())
