"""bowgpu_parquet_read_bool_column on the device: a Parquet BOOLEAN column into the bit-packed Boolean layout of bowgpu_convert and the
Boolean reducers.  The expectation is always pyarrow.parquet.read_table of the same file (for the hand-built shapes pyarrow cannot be
asked to write: what their builder meant, which tests/test_parquet_bool_cpu.py proves against pyarrow).  Every comparison is bit for
bit - value bits, validity bits, value bits of null rows 0, the padding bits of both last bytes 0, the null count - for HOST and
DEVICE outputs."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_bool_pages as pb
from bow_amd import capi

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001]   # the word and trip (2048 rows) edges
MODES = ["plain_v1", "rle_v1", "rle_v2"]
MASK = {"plain_v1": capi.PARQUET_ENC_PLAIN, "rle_v1": capi.PARQUET_ENC_RLE, "rle_v2": capi.PARQUET_ENC_RLE}
MID_WORD = dict(write_batch_size=100, data_page_size=16, row_group_size=330)   # pages of 200 / 130 rows, row groups of 330


def assert_column(label, got, vals, valid):
    """got: the OutColumn of read_bool_column; vals / valid: per row"""
    n = len(valid)
    nb = (n + 7) // 8
    assert got.type == capi.BOOLEAN and got.length == n, (label, got.type, got.length)
    assert got.null_count == int((~valid).sum()), (label, got.null_count, int((~valid).sum()))
    gv, gb = got.host_arrays()
    want_valid = np.packbits(valid, bitorder="little")          # (packbits pads the last byte with zeros: the padding is compared too)
    want_bits = np.packbits(vals & valid, bitorder="little")    # (null rows: 0)
    bad = np.flatnonzero(np.asarray(gb[:nb]) != want_valid)
    assert bad.size == 0, (label, "validity bytes", bad[:8])
    bad = np.flatnonzero(np.asarray(gv[:nb]) != want_bits)
    assert bad.size == 0, (label, "value bytes", bad[:8], np.asarray(gv[:nb])[bad[:4]], want_bits[bad[:4]])


GUARD = 64   # bytes of poison behind the ceil(n / 8) bytes of each buffer of a device output


class GuardedOut(capi.OutColumn):
    """a device output of n slots whose two buffers hold ceil(n / 8) bytes and GUARD bytes behind them, all poisoned: a HOST output
    is poisoned by OutColumn itself, this makes the DEVICE half as strong (what lies behind the column's bytes must keep its poison,
    and the padding bits of the last byte are zeros the library wrote, not zeros it found)"""

    def __init__(self, n):
        self.slots, self.residency, self.type, self.null_count, self.length = n, capi.DEVICE, 0, -1, n
        self.nb = (n + 7) // 8
        self.values = capi.DeviceBuffer.from_numpy(np.full(self.nb + GUARD, 0x5A, np.uint8))
        self.validity = capi.DeviceBuffer.from_numpy(np.full(self.nb + GUARD, 0xA5, np.uint8))

    def host_arrays(self):   # (OutColumn's reads 8 bytes a slot before it looks at the type: these buffers hold bits only)
        nb = (self.length + 7) // 8
        return self.values.to_numpy(np.uint8, nb), self.validity.to_numpy(np.uint8, nb)

    def guard_intact(self):
        v = self.values.to_numpy(np.uint8, self.nb + GUARD)
        b = self.validity.to_numpy(np.uint8, self.nb + GUARD)
        return bool((v[self.nb:] == 0x5A).all() and (b[self.nb:] == 0xA5).all())


def read_and_compare(label, path, column, vals, valid, residencies=(capi.HOST, capi.DEVICE)):
    f = capi.ParquetFile(path)
    for res in residencies:
        if res == capi.DEVICE:
            got = GuardedOut(f.num_rows)
            o = got.c()
            capi.check(capi.lib().bowgpu_parquet_read_bool_column(f.h, column, C.byref(o)))
            got.absorb(o)
            assert got.guard_intact(), (label, "written behind the column's bytes")
        else:
            got = f.read_bool_column(column, out_residency=res)
        assert_column("%s residency %d" % (label, res), got, vals, valid)
    f.close()


def against_pyarrow(label, path, column=0, name="flag", **kw):
    vals, valid = pb.read_back(path, name)
    read_and_compare(label, path, column, vals, valid, **kw)
    return vals, valid


@pytest.mark.parametrize("nulls", ["0", "0.3", "1.0", "required"])
@pytest.mark.parametrize("mode", MODES)
def test_row_counts_at_the_word_and_trip_edges(tmp_path, mode, nulls):
    rng = np.random.default_rng(41)
    for n in SIZES:
        vals = rng.random(n) < 0.5
        valid = None if nulls == "required" else rng.random(n) >= float(nulls)
        path = str(tmp_path / ("n%d.parquet" % n))
        pb.write_pyarrow(path, vals, valid, mode)
        f = capi.ParquetFile(path)
        assert f.check_bool_column(0) == MASK[mode]
        f.close()
        against_pyarrow("%s nulls %s n %d" % (mode, nulls, n), path)


@pytest.mark.parametrize("compression", ["none", "snappy"])
@pytest.mark.parametrize("mode", MODES)
def test_pages_and_row_groups_that_start_mid_word(tmp_path, mode, compression):
    rng = np.random.default_rng(42)
    n = 4097
    path = str(tmp_path / "midword.parquet")
    for valid in (rng.random(n) >= 0.3, None):
        pb.write_pyarrow(path, rng.random(n) < 0.5, valid, mode, compression=compression, **MID_WORD)
        md = pq.ParquetFile(path).metadata
        assert md.num_row_groups == 13 and md.row_group(0).num_rows == 330
        against_pyarrow("%s %s required %s" % (mode, compression, valid is None), path)


def _shapes(rng):
    n = 9000
    out = {"random": rng.random(n) < 0.5, "all_true": np.ones(n, bool), "all_false": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0,
           "long_runs": np.concatenate([np.ones(5000, bool), np.zeros(3000, bool), np.ones(77, bool)]),   # three RLE runs, two longer than a trip
           "runs_of_8": (np.arange(n) // 8) % 2 == 0, "runs_of_7": (np.arange(n) // 7) % 2 == 0,
           "sparse_true": rng.random(n) < 0.01}
    return out


@pytest.mark.parametrize("shape", ["random", "all_true", "all_false", "alternating", "long_runs", "runs_of_8", "runs_of_7", "sparse_true"])
def test_value_shapes(tmp_path, shape):
    rng = np.random.default_rng(43)
    vals = _shapes(rng)[shape]
    n = len(vals)
    long_nulls = np.ones(n, bool)
    long_nulls[300:300 + 2500] = False   # nulls in runs longer than a trip of 2048 rows
    long_nulls[n - 2100:n - 10] = False
    path = str(tmp_path / "shape.parquet")
    for mode in MODES:
        for label, valid in (("no nulls", np.ones(n, bool)), ("nulls 0.3", rng.random(n) >= 0.3), ("null runs", long_nulls)):
            pb.write_pyarrow(path, vals, valid, mode)
            against_pyarrow("%s %s %s" % (shape, mode, label), path)


def test_hand_built_pages(tmp_path):
    files = pb.well_formed(np.random.default_rng(11))
    for name, (pages, optional, codec, vals, valid) in files.items():
        path = str(tmp_path / (name + ".parquet"))
        pb.write_file(path, pages, optional, codec)
        read_and_compare(name, path, 0, vals & valid, valid)
        if name not in pb.NO_PYARROW:
            against_pyarrow(name + " (pyarrow)", path, residencies=(capi.HOST,))


def test_damaged_pages_come_back_as_argument_errors(tmp_path):
    """each file of parquet_bool_pages.damaged is short of something it promises (what pyarrow does with them:
    tests/test_parquet_bool_cpu.py); a good file is read between them, so a raised status bit does not outlive its call"""
    rng = np.random.default_rng(12)
    good = str(tmp_path / "good.parquet")
    gv, gm = rng.random(500) < 0.5, rng.random(500) >= 0.3
    pb.write_pyarrow(good, gv, gm, "rle_v1")
    files = pb.damaged(rng)
    assert len(files) == 11
    for name, (pages, optional, codec) in files.items():
        path = str(tmp_path / (name + ".parquet"))
        pb.write_file(path, pages, optional, codec)
        f = capi.ParquetFile(path)
        for res in (capi.HOST, capi.DEVICE):
            with pytest.raises(capi.BowGpuError) as e:
                f.read_bool_column(0, out_residency=res)
            assert e.value.code == -10 and "'flag'" in e.value.message, (name, e.value.message)
        f.close()
        read_and_compare("good after " + name, good, 0, gv & gm, gm, residencies=(capi.HOST,))


def test_residencies_the_empty_file_and_the_declines(tmp_path):
    rng = np.random.default_rng(44)
    n = 3001
    path = str(tmp_path / "res.parquet")
    pb.write_pyarrow(path, rng.random(n) < 0.5, rng.random(n) >= 0.3, "plain_v1", extra={"t": pa.array(np.arange(n, dtype=np.int64))})
    against_pyarrow("three residencies", path, column=1, residencies=(capi.HOST, capi.HOST_PINNED, capi.DEVICE))
    f = capi.ParquetFile(path)
    with pytest.raises(capi.BowGpuError) as e:
        f.read_bool_column(0)
    assert e.value.code == -9 and "'t'" in e.value.message and "bowgpu_parquet_read_column" in e.value.message
    with pytest.raises(capi.BowGpuError) as e:
        f.read_column(1)
    assert e.value.code == -9 and "INT64 / DOUBLE" in e.value.message
    f.close()
    empty = str(tmp_path / "empty.parquet")
    pb.write_pyarrow(empty, np.zeros(0, bool), np.zeros(0, bool))
    f = capi.ParquetFile(empty)
    for res in (capi.HOST, capi.DEVICE):
        got = f.read_bool_column(0, out_residency=res)
        assert got.type == capi.BOOLEAN and got.length == 0 and got.null_count == 0
    f.close()


def test_flag_column_to_the_boolean_reducers_without_leaving_the_device(tmp_path):
    """an Int64 time column through read_column and a BOOLEAN flag through read_bool_column, both into HBM, aggregated there by the
    Boolean reducers; the expectation is the oracle over pyarrow's decode of the same file"""
    from bool_agg_common import compare_exact
    from oracle import pyoracle as orc
    rng = np.random.default_rng(45)
    n = 50_000
    path = str(tmp_path / "chain.parquet")
    pb.write_pyarrow(path, rng.random(n) < 0.4, rng.random(n) >= 0.3, "rle_v2", compression="snappy",
                     extra={"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64))})
    f = capi.ParquetFile(path)
    assert [c[1] for c in f.columns] == [capi.INT64, capi.BOOLEAN]
    ts = f.read_column(0, out_residency=capi.DEVICE)
    flag = f.read_bool_column(1, out_residency=capi.DEVICE)
    f.close()
    assert ts.null_count == 0 and flag.type == capi.BOOLEAN
    cols = [capi.Column(ts.values, None, capi.INT64, 0, n, 0), capi.Column(flag.values, flag.validity, capi.BOOLEAN, 0, n, flag.null_count)]
    aggs = [("WindowStart", 0), ("Count", 1), ("ArithmeticMean", 1), ("Last", 1), ("Mode", 1)]
    got, _ = capi.rolling_aggregate(cols, 0, 50, aggs, out_residency=capi.DEVICE)
    tv = np.asarray(pq.read_table(path).column("ts")).astype(np.int64)
    vals, valid = pb.read_back(path, "flag")
    ocols = [orc.Column(tv, None, orc.INT64),
             orc.Column(np.packbits(vals, bitorder="little"), np.packbits(valid, bitorder="little"), orc.BOOLEAN, 0, n)]
    want, _ = orc.aggregate(ocols, 0, 50, aggs)
    for (k, _c), g, w in zip(aggs, got, want):
        compare_exact("flag chain %s" % k, g, w)


def test_the_references_own_file(tmp_path):
    """tests/golden/bow1-100-rows.parquet, written by the reference through parquet-go (SNAPPY, PLAIN, data page v1): its Boolean column"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bow1-100-rows.parquet")
    f = capi.ParquetFile(path)
    i = [c[0] for c in f.columns].index("Boolean_bow1")
    assert f.columns[i][1] == capi.BOOLEAN and f.check_bool_column(i) == capi.PARQUET_ENC_PLAIN
    f.close()
    vals, valid = against_pyarrow("bow1-100-rows", path, column=i, name="Boolean_bow1")
    assert 0 < valid.sum() <= 100
