"""Bow.Convert on the device (bowgpu_convert, bow_amd/csrc/convert.hip) against the numpy model of tests/convert_model.py, exactly:
every (source, target) pair of Int64, Float64 and Boolean at the lengths where convert_kernel takes another path (a lane's pair, a
64-row word, a chunk of 128 rows, a trip of 512, a workgroup of 2048), at Arrow offsets that are and are not multiples of 8, with the
validity absent, all null or 30 % null and the null count given or left to the library, null slots holding NaN, 1 or set bits, from
and to every residency.  Checked: values, validity, null_count, type, zeroed null slots, clear padding bits, and that nothing is
written behind 8 n bytes (ceil(n / 8) for bits) of a buffer - poison on the host, a guard region on the device."""
import os
import subprocess

import numpy as np
import pyarrow.parquet as pq
import pytest

import convert_model as cm
from bool_agg_common import bool_cols
from bow_amd import capi
from convert_model import B, F, I

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 63, 64, 65, 2047, 2048, 2049, 4097)
NULLS = ("absent", "all", "all_counted", "given", "counted")
SPARE = 19          # slots of capacity beyond the column's length: what lies behind the rows must keep its poison
GUARD = 64          # bytes behind a device output
PAIR_IDS = ["%s-%s" % (cm.NAMES[a], cm.NAMES[b]) for a, b in cm.PAIRS]


def grid_columns(from_t, to_t, seed):
    """one CaseColumn per (length, offset, validity mode): special values salted in, null slots filled with NaN / 1 / set bits in turn"""
    rng = np.random.default_rng(seed)
    cols = []
    for n in LENGTHS:
        for offset in cm.OFFSETS:
            for nulls in NULLS:
                slots = cm.random_slots(rng, from_t, n)
                valid = None if nulls == "absent" else np.zeros(n, bool) if nulls.startswith("all") else rng.random(n) >= 0.3
                keep = [] if nulls.startswith("all") else cm.salt(rng, from_t, slots, valid)
                if valid is not None:
                    held = np.zeros(n, bool)
                    held[keep] = True
                    slots[~valid & ~held] = cm.null_fill(from_t, ("nan", "one")[len(cols) % 2])
                cols.append(cm.CaseColumn(from_t, to_t, slots, valid, offset, -1 if nulls.endswith("counted") else 1, capi.HOST, keep))
    return cols


class GuardedOut(capi.OutColumn):
    """a device output whose buffers are followed by SPARE slots and GUARD bytes of poison"""

    def __init__(self, n, to_t):
        self.slots, self.residency, self.type, self.null_count, self.length = n + SPARE, capi.DEVICE, 0, -1, n + SPARE
        self.value_bytes = (n + 7) // 8 if to_t == B else 8 * n
        self.bitmap_bytes = (n + 7) // 8
        self.values = capi.DeviceBuffer.from_numpy(np.full(8 * (n + SPARE) + GUARD, 0x5A, np.uint8))
        self.validity = capi.DeviceBuffer.from_numpy(np.full((n + SPARE + 7) // 8 + GUARD, 0xA5, np.uint8))

    def guard_intact(self):
        v = self.values.to_numpy(np.uint8, self.values.nbytes)
        b = self.validity.to_numpy(np.uint8, self.validity.nbytes)
        return (v[self.value_bytes:] == 0x5A).all() and (b[self.bitmap_bytes:] == 0xA5).all()


def host_poison_intact(out, n, to_t):
    v = out.values.view(np.uint8)
    return (v[(n + 7) // 8 if to_t == B else 8 * n:] == 0x5A).all() and (out.validity[(n + 7) // 8:] == 0xA5).all()


def run_columns(case_cols, in_res, out_res):
    cols = [cm.place(c.column(), in_res) for c in case_cols]
    try:
        if out_res == capi.DEVICE:
            outs = [GuardedOut(len(c.slots), c.to_t) for c in case_cols]
        else:
            outs = [capi.OutColumn(len(c.slots) + SPARE, out_res) for c in case_cols]
        capi.convert(cols, [c.to_t for c in case_cols], outs=outs)
    finally:
        for c in cols:
            c.unpin()
    assert capi.last_kernel_name() == "convert_kernel"
    for k, (c, o) in enumerate(zip(case_cols, outs)):
        name = (cm.NAMES[c.from_t], cm.NAMES[c.to_t], len(c.slots), c.offset, "no bitmap" if c.valid is None else int(c.valid.sum()), c.null_count, k)
        cm.compare(name, o, c.expected())
        assert o.guard_intact() if out_res == capi.DEVICE else host_poison_intact(o, len(c.slots), c.to_t), (name, "written behind the rows")
    return outs


@pytest.mark.parametrize("in_res,out_res", [(capi.HOST, capi.HOST), (capi.DEVICE, capi.DEVICE), (capi.HOST_PINNED, capi.HOST)],
                         ids=["host-host", "device-device", "pinned-host"])
@pytest.mark.parametrize("from_t,to_t", cm.PAIRS, ids=PAIR_IDS)
def test_every_pair_length_offset_and_validity(from_t, to_t, in_res, out_res):
    cols = grid_columns(from_t, to_t, 100 * from_t + to_t)
    if in_res != capi.HOST:   # (every length and validity mode; the offsets in turn, all of them at the longest)
        per_len = len(cm.OFFSETS) * len(NULLS)
        cols = [c for k, c in enumerate(cols) if c.offset == cm.OFFSETS[(k // per_len) % len(cm.OFFSETS)] or len(c.slots) == 4097]
    run_columns(cols, in_res, out_res)


def test_host_inputs_to_device_and_pinned_outputs():
    cols = [c for a, b in cm.PAIRS for c in grid_columns(a, b, 7)[5::23]]
    run_columns(cols, capi.HOST, capi.DEVICE)
    run_columns(cols, capi.DEVICE, capi.HOST_PINNED)


def nine_columns(seed, n=3001):
    rng = np.random.default_rng(seed)
    cols = []
    for k, (a, b) in enumerate(cm.PAIRS):
        slots = cm.random_slots(rng, a, n - 37 * k)   # lengths differ: Convert has no frame rule
        valid = rng.random(len(slots)) >= 0.3
        cm.salt(rng, a, slots, valid)
        cols.append(cm.CaseColumn(a, b, slots, valid, cm.OFFSETS[k % 6], -1, capi.HOST))
    return cols


def bytes_of(outs):
    return [tuple(np.asarray(x).tobytes() for x in o.host_arrays()) + (o.type, o.length, o.null_count) for o in outs]


def test_nine_pairs_in_one_call_equal_nine_single_calls():
    cols = nine_columns(3)
    together = bytes_of(run_columns(cols, capi.HOST, capi.HOST))
    single = [bytes_of(capi.convert([c.column()], [c.to_t]))[0] for c in cols]
    assert together == single


def test_the_same_call_twice_gives_the_same_bytes():
    cols = nine_columns(4, 70_001)
    dev = [c.column().to_device() for c in cols]
    types = [c.to_t for c in cols]
    first = bytes_of(capi.convert(dev, types, out_residency=capi.DEVICE))
    assert first == bytes_of(capi.convert(dev, types, out_residency=capi.DEVICE))
    assert first == bytes_of(capi.convert([c.column() for c in cols], types))
    for c, got in zip(cols, first):
        e = c.expected()
        assert got[0] == e.values.tobytes() and got[1] == e.validity.tobytes()


def test_cpp_mirror_converts():
    exe = os.path.join(ROOT, "tests", "cpp", "test_convert")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bow_amd", "host")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failures" in p.stdout


AGGS = [("WindowStart", 0), ("Count", 1), ("ArithmeticMean", 1), ("Last", 1), ("Mode", 1)]


def flag_frame(n=5000, seed=11):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(1, 9, n)).astype(np.int64)
    flags = (rng.random(n) < 0.4).astype(np.int64)
    valid = rng.random(n) >= 0.3
    return ts, flags, valid


def test_chain_flag_column_to_boolean_to_rolling_aggregate():
    """an Int64 0 / 1 flag column with nulls becomes the bit-packed column the Boolean reducers want, and never leaves the device"""
    ts, flags, valid = flag_frame()
    slots = flags.copy()
    slots[~valid] = 1   # (what a null slot holds does not matter)
    flag_col = cm.make_column(I, slots, valid, offset=13).to_device()
    as_bool = capi.convert([flag_col], [B], out_residency=capi.DEVICE)[0]
    assert (as_bool.type, as_bool.length, as_bool.null_count) == (B, len(ts), int((~valid).sum()))
    ts_col = capi.Column(ts, None, I).to_device()
    got, _ = capi.rolling_aggregate([ts_col, capi.out_as_column(as_bool)], 0, 40, AGGS, out_residency=capi.DEVICE)
    packed, _ = bool_cols(ts, flags != 0, valid)   # the same column packed on the host
    want, _ = capi.rolling_aggregate(packed, 0, 40, AGGS)
    assert bytes_of(got) == bytes_of(want)
    assert [o.type for o in got] == [I, I, F, B, B]


def test_chain_boolean_last_to_int64_to_parquet(tmp_path):
    """a Boolean Last result becomes an Int64 column that the Parquet writer takes, without leaving the device"""
    ts, flags, valid = flag_frame(seed=12)
    packed, _ = bool_cols(ts, flags != 0, valid)
    res, _ = capi.rolling_aggregate([c.to_device() for c in packed], 0, 40, [("WindowStart", 0), ("Last", 1)], out_residency=capi.DEVICE)
    assert res[1].type == B and 0 < res[1].null_count < res[1].length
    as_int = capi.convert([capi.out_as_column(res[1])], [I], out_residency=capi.DEVICE)[0]
    path = str(tmp_path / "last.parquet")
    capi.write_parquet(path, [capi.out_as_column(res[0]), capi.out_as_column(as_int)], ["time", "last"])
    table = pq.read_table(path)
    want_last = res[1].to_list()
    assert table.column("time").to_pylist() == res[0].to_list()
    assert table.column("last").to_pylist() == [None if x is None else int(x) for x in want_last]
    assert str(table.schema.field("last").type) == "int64"
