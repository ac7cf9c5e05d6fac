"""RLE_DICTIONARY through bowgpu_parquet_write / bowgpu_parquet_write_codec on the device.  Every comparison is exact.  Per file
written, verify() checks four things: pyarrow's reading bit for bit (through uint64 views, validity included); the walk of
tests/parquet_dict_walk.py from each chunk's dictionary page on - the dictionary equals expected_dictionary, every values section
equals expected_section (the contract of include/bowgpu.h restated; PLAIN where the contract falls back, the DELTA bytes of
tests/parquet_pages.py beside it); the library's own loader; and ParquetFile.check_column's mask."""
import os

import numpy as np
import pyarrow.parquet as pq
import pytest

import parquet_dict_walk as dwalk
import parquet_pages as pp
from bow_amd import capi
from test_gpu_parquet_write import Frame, write, want_levels, delta_shapes, RES, I64_MIN, I64_MAX
from test_parquet_loader import expect

pytestmark = pytest.mark.gpu

PLAIN, DELTA, DICT = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_RLE_DICTIONARY
SNAPPY = capi.PARQUET_CODEC_SNAPPY
CAP = capi.PARQUET_DICT_MAX
MASK = {PLAIN: capi.PARQUET_ENC_PLAIN, DELTA: capi.PARQUET_ENC_DELTA_BINARY_PACKED, DICT: capi.PARQUET_ENC_RLE_DICTIONARY}


def chunk_plan(values, valid, enc):
    """(the encoding the chunk comes out as, its dictionary or None) by the contract"""
    if enc != DICT:
        return enc, None
    dense = values[valid]
    if len(dense) == 0:
        return PLAIN, None
    d = dwalk.expected_dictionary(dense)
    return (PLAIN, None) if len(d) > CAP else (DICT, d)


def verify(path, data, names, page_rows, rg_rows, encodings, codec=0, info=None):
    """data: [(values, valid)] per column.  Returns the encodings each column's chunks came out as, row group by row group."""
    ncols, n = len(data), len(data[0][0])
    assert os.listdir(os.path.dirname(path)).count(os.path.basename(path) + ".tmp") == 0
    f = pq.ParquetFile(path)
    md = f.metadata
    groups = [(a, min(a + rg_rows, n)) for a in range(0, n, rg_rows)]
    assert md.num_rows == n and md.num_columns == ncols and md.num_row_groups == len(groups)
    table = f.read()
    npages = level_bytes = value_bytes = 0
    came_out = []
    for i, (values, valid) in enumerate(data):
        # 1. pyarrow, bit for bit
        gv, gm = expect(table, names[i])
        assert np.array_equal(gm, valid), (names[i], np.flatnonzero(gm != valid)[:10])
        assert np.array_equal(np.asarray(gv).view(np.uint64)[valid], values.view(np.uint64)[valid]), names[i]
        # 2. the bytes
        mask, encs = 0, []
        for g, (a, b) in enumerate(groups):
            ch = md.row_group(g).column(i)
            enc, want_dict = chunk_plan(values[a:b], valid[a:b], encodings[i])
            encs.append(enc)
            mask |= MASK[enc]
            assert ch.num_values == b - a and ch.compression == ("SNAPPY" if codec else "UNCOMPRESSED")
            assert ch.statistics.null_count == int((~valid[a:b]).sum())
            want_names = {PLAIN: ("PLAIN", "RLE"), DELTA: ("DELTA_BINARY_PACKED", "RLE"), DICT: ("RLE_DICTIONARY", "PLAIN", "RLE")}[enc]
            assert ch.encodings == want_names, (names[i], g, ch.encodings)
            assert ch.has_dictionary_page == (enc == DICT)
            dictionary, pages = dwalk.chunk_pages(path, ch)   # (both totals, and where the dictionary page lies)
            if enc == DICT:
                assert np.array_equal(dictionary, want_dict), (names[i], g)
                value_bytes += 8 * len(dictionary)
            else:
                assert dictionary is None
            assert [pg[0] for pg in pages] == [min(page_rows, b - r) for r in range(a, b, page_rows)]
            for pg, r in zip(pages, range(a, b, page_rows)):
                ok, v = valid[r:min(r + page_rows, b)], values[r:min(r + page_rows, b)]
                assert pg[1] == enc
                assert pg[2] == want_levels(ok), (names[i], g, r)
                want = dwalk.expected_section(v[ok], want_dict) if enc == DICT else pp.encode_delta(v[ok], 128, 4) if enc == DELTA else pp.encode_plain(v[ok])
                assert pg[3] == want, (names[i], g, r, int(ok.sum()))
                level_bytes += 4 + len(pg[2])
                value_bytes += len(pg[3])
            npages += len(pages)
        came_out.append((mask, encs))
    if info is not None:
        assert (info.rows, info.row_groups, info.data_pages, info.file_bytes) == (n, len(groups), npages, os.path.getsize(path))
        assert (info.level_bytes, info.value_bytes) == (level_bytes, value_bytes)
    # 3. the library's own loader, 4. its mask
    lf = capi.ParquetFile(path)
    assert lf.num_rows == n and [c[0] for c in lf.columns] == list(names)
    for i, (values, valid) in enumerate(data):
        if n:
            assert lf.check_column(i) == came_out[i][0], (names[i], lf.check_column(i), came_out[i])
        out = lf.read_column(i)
        assert out.length == n and out.null_count == int((~valid).sum())
        assert np.array_equal(out.valid_mask(), valid)
        assert np.array_equal(out.host_arrays()[0].view(np.uint64)[valid], values.view(np.uint64)[valid]), names[i]
    lf.close()
    return [e for _, e in came_out]


def pool_of(entries, rng, dt):
    """`entries` distinct 64-bit patterns with the type's special ones first"""
    if dt == np.int64:
        sp = np.array([I64_MIN, I64_MAX, 0, -1], dtype=np.int64).view(np.uint64)
    else:   # -0.0 / +0.0, two NaN payloads, the infinities
        sp = np.array([0x8000000000000000, 0, 0x7ff8000000000000, 0xfff8dead0000beef, 0x7ff0000000000000, 0xfff0000000000000], dtype=np.uint64)
    pool = sp[:entries]
    while len(pool) < entries:
        more = rng.integers(0, 2 ** 63, 2 * entries, dtype=np.uint64) * np.uint64(2) + np.uint64(rng.integers(0, 2))
        pool = np.concatenate([pool, more])
        _, first = np.unique(pool, return_index=True)
        pool = pool[np.sort(first)][:entries]
    return pool.view(dt)


def drawn(pool, n, rng, at=0):
    """n values from the pool, every entry present from row `at` on (n - at >= len(pool))"""
    v = pool[rng.integers(0, len(pool), n)]
    v[at:at + len(pool)] = pool
    return v


# ------------------------------------------------------------------ 1. the width steps, both types, with and without a bitmap
@pytest.mark.parametrize("codec", [0, SNAPPY], ids=["uncompressed", "snappy"])
@pytest.mark.parametrize("entries", [1, 2, 3, 4, 5, 255, 256, 257])
def test_width_steps(tmp_path, entries, codec):
    rng = np.random.default_rng(200 + entries)
    n, page, rg = 512 + 200, 64, 512
    fr = Frame()
    for k, dt in enumerate((np.int64, np.float64)):
        pool = pool_of(entries, rng, dt)
        v = drawn(pool, n, rng)
        valid = rng.random(n) >= 0.3
        valid[:entries] = True
        fr.add("nulls_%d" % k, v, valid, offset=3 + 10 * k, res=RES[(entries + k) % 3])
        fr.add("dense_%d" % k, v.copy(), None, offset=5 * k, res=RES[(entries + k + 1) % 3])
    enc = [DICT] * 4
    path = str(tmp_path / "width.parquet")
    info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, codec=codec)
    out = verify(path, fr.data, fr.names, page, rg, enc, codec, info)
    assert all(e == [DICT, DICT] for e in out)
    md = pq.read_metadata(path)
    for i in range(4):   # the first row group holds every entry of the pool
        d, pages = dwalk.chunk_pages(path, md.row_group(0).column(i))
        assert len(d) == entries and all(pg[3][0] == dwalk.width_of(entries) for pg in pages)


# ------------------------------------------------------------------ 2. at the cap
@pytest.fixture(scope="module")
def cap_pool():
    rng = np.random.default_rng(300)
    return pool_of(CAP + 1, rng, np.int64), pool_of(CAP + 1, rng, np.float64)


@pytest.mark.parametrize("entries", [CAP - 1, CAP, CAP + 1])
def test_entry_counts_at_the_cap(tmp_path, cap_pool, entries):
    rng = np.random.default_rng(entries)
    page = 1024
    n = rg = 65 * page   # 66560: just above the cap + 1
    codec = SNAPPY if entries == CAP else 0
    fr = Frame()
    fr.add("i", drawn(cap_pool[0][:entries], n, rng), None, res=capi.DEVICE)
    valid = np.ones(n, bool)
    valid[rng.choice(np.arange(entries, n), 500, replace=False)] = False   # (nulls behind the rows that hold every entry)
    fr.add("f", drawn(cap_pool[1][:entries], n, rng), valid, offset=7, res=capi.HOST)
    enc = [DICT, DICT]
    path = str(tmp_path / "cap.parquet")
    info = capi.write_parquet(path, fr.cols, fr.names, page_rows=page, row_group_rows=rg, encodings=enc, codec=codec)
    out = verify(path, fr.data, fr.names, page, rg, enc, codec, info)
    assert out == [[PLAIN if entries > CAP else DICT]] * 2
    if entries > CAP:   # byte for byte what encoding 0 gives
        path0 = str(tmp_path / "cap_plain.parquet")
        capi.write_parquet(path0, fr.cols, fr.names, page_rows=page, row_group_rows=rg, encodings=[PLAIN, PLAIN], codec=codec)
        assert open(path, "rb").read() == open(path0, "rb").read()


# ------------------------------------------------------------------ 3. the decision is per chunk
@pytest.mark.parametrize("rg", [128, 256])
def test_dictionaries_differ_per_row_group(tmp_path, rg):
    rng = np.random.default_rng(400 + rg)
    n = 1000
    v = (np.arange(n, dtype=np.int64) // 100) * 1000 - 3000 + rng.integers(0, 3, n)   # the values drift: every row group has its own few
    f = np.round(rng.standard_normal(n), 1) + np.arange(n) // rg
    fr = Frame().add("i", v, rng.random(n) >= 0.2, offset=9, res=capi.DEVICE).add("f", f, None, res=capi.HOST_PINNED)
    enc = [DICT, DICT]
    for codec in (0, SNAPPY):
        path = str(tmp_path / ("groups%d.parquet" % codec))
        info = capi.write_parquet(path, fr.cols, fr.names, page_rows=64, row_group_rows=rg, encodings=enc, codec=codec)
        verify(path, fr.data, fr.names, 64, rg, enc, codec, info)
        md = pq.read_metadata(path)
        dicts = [dwalk.chunk_pages(path, md.row_group(g).column(0))[0].tobytes() for g in range(md.num_row_groups)]
        assert len(set(dicts)) > 1
    fr.release()


def test_a_row_group_that_overflows_beside_one_that_does_not(tmp_path, cap_pool):
    rng = np.random.default_rng(500)
    page, rg = 64, 1025 * 64   # 65600 >= the cap + 1
    n = rg + 300
    v = np.concatenate([drawn(cap_pool[0], rg, rng), drawn(cap_pool[0][:17], 300, rng)])
    f = np.concatenate([drawn(cap_pool[1][:1000], rg, rng), cap_pool[1][rng.integers(0, CAP + 1, 300)]])   # 300 rows never overflow
    valid = rng.random(n) >= 0.1
    valid[:CAP + 1] = True
    fr = Frame().add("i", v, valid, offset=1, res=capi.DEVICE).add("f", f, None, res=capi.DEVICE)
    enc = [DICT, DICT]
    path = str(tmp_path / "beside.parquet")
    info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, codec=SNAPPY)
    out = verify(path, fr.data, fr.names, page, rg, enc, SNAPPY, info)
    assert out == [[PLAIN, DICT], [DICT, DICT]]
    lf = capi.ParquetFile(path)
    assert lf.check_column(0) == capi.PARQUET_ENC_PLAIN | capi.PARQUET_ENC_RLE_DICTIONARY
    lf.close()


# ------------------------------------------------------------------ 4. counts of values in a page
@pytest.mark.parametrize("codec", [0, SNAPPY], ids=["uncompressed", "snappy"])
def test_page_counts_and_a_page_without_a_valid_row(tmp_path, codec):
    rng = np.random.default_rng(600)
    page = 64
    counts = [5, 0, 1, 7, 8, 9, 0, 63, 64, 3]
    n = page * len(counts) - 20   # a short last page
    valid = np.zeros(n, bool)
    for p, k in enumerate(counts):
        rows = min(page, n - p * page)
        valid[p * page + np.sort(rng.choice(rows, k, replace=False))] = True
    fr = Frame()
    for k, dt in enumerate((np.int64, np.float64)):
        v = pool_of(300, rng, dt)[rng.integers(0, 300, n)]   # (what lies under a null is no entry)
        fr.add("c%d" % k, v, valid, offset=k * 11, res=RES[k])
    fr.add("allnull", pool_of(5, rng, np.float64)[rng.integers(0, 5, n)], np.zeros(n, bool), offset=2, res=capi.DEVICE)
    enc = [DICT, DICT, DICT]
    for rg in (page * 4, page * 16):
        path = str(tmp_path / ("counts%d.parquet" % rg))
        info = capi.write_parquet(path, fr.cols, fr.names, page_rows=page, row_group_rows=rg, encodings=enc, codec=codec)
        out = verify(path, fr.data, fr.names, page, rg, enc, codec, info)
        assert set(out[0]) == {DICT} and set(out[2]) == {PLAIN}   # a chunk without a valid row falls back
    md = pq.read_metadata(path)
    d, pages = dwalk.chunk_pages(path, md.row_group(0).column(0))
    w = dwalk.width_of(len(d))
    assert w >= 6 and [len(pg[3]) for pg in pages[:3]] == [2 + w, 1, 2 + w]   # the width byte alone between two pages with values
    fr.release()


# ------------------------------------------------------------------ 5. special values, residencies, offsets
@pytest.mark.parametrize("offset", [0, 3, 13])
def test_special_patterns_in_unsigned_order(tmp_path, offset):
    rng = np.random.default_rng(700 + offset)
    n = 700
    fr = Frame()
    for res in RES:
        fr.add("i%d" % res, drawn(pool_of(4, rng, np.int64), n, rng), rng.random(n) >= 0.3 if res != capi.HOST else None, offset=offset, res=res)
        fv = drawn(pool_of(6, rng, np.float64), n, rng)
        ok = rng.random(n) >= 0.3
        ok[:6] = True
        fr.add("f%d" % res, fv, ok, offset=offset + 1, res=res)
    enc = [DICT] * 6
    path = str(tmp_path / "special.parquet")
    info = write(path, fr, page_rows=128, row_group_rows=1024, encodings=enc)
    verify(path, fr.data, fr.names, 128, 1024, enc, 0, info)
    md = pq.read_metadata(path)
    d = dwalk.chunk_pages(path, md.row_group(0).column(1))[0]
    assert d.tolist() == [0, 0x7ff0000000000000, 0x7ff8000000000000, 0x8000000000000000, 0xfff0000000000000, 0xfff8dead0000beef]
    d = dwalk.chunk_pages(path, md.row_group(0).column(0))[0]
    assert d.view(np.int64).tolist() == [0, I64_MAX, I64_MIN, -1]   # negatives last


# ------------------------------------------------------------------ 6. beside DELTA and PLAIN
@pytest.mark.parametrize("codec", [0, SNAPPY], ids=["uncompressed", "snappy"])
def test_dictionary_next_to_delta_and_plain(tmp_path, codec):
    rng = np.random.default_rng(800)
    n = 3000
    fr = Frame()
    fr.add("ts", delta_shapes(n, rng)["timestamps"], None, res=capi.DEVICE)
    fr.add("state", rng.integers(0, 6, n).astype(np.int64), rng.random(n) >= 0.2, offset=3, res=capi.DEVICE)
    fr.add("v", rng.standard_normal(n), rng.random(n) >= 0.3, offset=9, res=capi.HOST)
    fr.add("q", np.round(rng.standard_normal(n), 2), rng.random(n) >= 0.05, offset=4, res=capi.HOST_PINNED)
    enc = [DELTA, DICT, PLAIN, DICT]
    path = str(tmp_path / "mixed.parquet")
    info = write(path, fr, page_rows=512, row_group_rows=1024, encodings=enc, codec=codec)
    out = verify(path, fr.data, fr.names, 512, 1024, enc, codec, info)
    assert out == [[DELTA] * 3, [DICT] * 3, [PLAIN] * 3, [DICT] * 3]


# ------------------------------------------------------------------ 7. the chain
def test_chain_boolean_to_int64_flag_to_a_dictionary_snappy_file(tmp_path):
    rng = np.random.default_rng(900)
    n, page, rg = 3000, 1024, 2048
    flags, valid = rng.random(n) < 0.2, rng.random(n) >= 0.1
    col = capi.Column(np.packbits(flags, bitorder="little"), np.packbits(valid, bitorder="little"), capi.BOOLEAN, 0, n, -1).to_device()
    as_int = capi.convert([col], [capi.INT64], out_residency=capi.DEVICE)[0]
    cols, names = [capi.out_as_column(as_int)], ["flag"]
    assert as_int.type == capi.INT64 and cols[0].residency == capi.DEVICE
    path = str(tmp_path / "chain.parquet")
    info = capi.write_parquet(path, cols, names, page_rows=page, row_group_rows=rg, encodings=[DICT], codec=SNAPPY)
    data = [(flags.astype(np.int64), valid)]
    assert verify(path, data, names, page, rg, [DICT], SNAPPY, info) == [[DICT, DICT]]
    # by the contract: per row group a dictionary of two entries, per page the width byte, a run header of 2 bytes, one bit a value
    want = 0
    for a in range(0, n, rg):
        want += 16
        for r in range(a, min(a + rg, n), page):
            k = int(valid[r:min(r + page, a + rg, n)].sum())
            assert k >= 512   # (64 groups of 8 and more: the run header takes 2 bytes)
            want += 1 + 2 + (k + 7) // 8
    assert info.value_bytes == want


# ------------------------------------------------------------------ 8. fuzz
def fuzz_frame(seed):
    rng = np.random.default_rng(5000 + seed)
    ncols = int(rng.integers(1, 4))
    page = int(rng.choice([64, 128, 1024]))
    big = seed % 4 == 3   # a cardinality above the cap needs the rows for it
    n = int(rng.integers(CAP + 2, CAP + 3000)) if big else int(rng.integers(1, 6000))
    rg = page * int(rng.integers(1, 9)) if not big else page * (-(-(CAP + 1) // page))
    fr, enc = Frame(), []
    for i in range(ncols):
        dt = (np.int64, np.float64)[int(rng.integers(0, 2))]
        card = CAP + 1 if big and i == 0 else int(rng.choice([2, 17, 1000]))
        pool = pool_of(card, rng, dt)
        values = drawn(pool, n, rng) if n >= card else pool[rng.integers(0, card, n)]
        density = [0.0, 0.3, "page"][int(rng.integers(0, 3))]
        if density == 0.0:
            valid = None if rng.random() < 0.5 else np.ones(n, bool)
        else:
            valid = rng.random(n) >= 0.3 if density == 0.3 else np.ones(n, bool)
            if density == "page" and n > page:
                p = int(rng.integers(0, n // page))
                valid[p * page:(p + 1) * page] = False
        if card > CAP and valid is not None:
            valid[:card] = True
        enc.append(DICT if i == 0 or rng.random() < 0.7 else PLAIN if dt == np.float64 else DELTA)
        fr.add("c%d" % i, values, valid, offset=int(rng.integers(0, 70)), res=RES[int(rng.integers(0, 3))], known=bool(rng.integers(0, 2)))
    return fr, enc, page, rg


def test_fuzz_against_pyarrow_the_contract_and_the_loader(tmp_path):
    seen = set()
    for seed in range(16):
        fr, enc, page, rg = fuzz_frame(seed)
        codec = SNAPPY if seed % 2 else 0
        path = str(tmp_path / ("fuzz%d.parquet" % seed))
        info = write(path, fr, page_rows=page, row_group_rows=rg, encodings=enc, statistics=bool(seed % 3), codec=codec)
        out = verify(path, fr.data, fr.names, page, rg, enc, codec, info)
        seen |= {(e, x) for e, col in zip(enc, out) for x in col}
        os.remove(path)
    assert {(DICT, DICT), (DICT, PLAIN)} <= seen


# ------------------------------------------------------------------ 9. determinism
def test_the_same_call_twice_gives_identical_files(tmp_path):
    rng = np.random.default_rng(1000)
    n = 20000
    fr = Frame()
    fr.add("i", drawn(pool_of(5000, rng, np.int64), n, rng), rng.random(n) >= 0.2, offset=3, res=capi.DEVICE)
    fr.add("f", np.round(rng.standard_normal(n), 1), None, res=capi.DEVICE)
    files = []
    for k in range(3):
        path = str(tmp_path / ("twice%d.parquet" % k))
        capi.write_parquet(path, fr.cols, fr.names, page_rows=1024, row_group_rows=8192, encodings=[DICT, DICT], codec=SNAPPY)
        files.append(open(path, "rb").read())
    assert files[0] == files[1] == files[2]
    verify(path, fr.data, fr.names, 1024, 8192, [DICT, DICT], SNAPPY)
