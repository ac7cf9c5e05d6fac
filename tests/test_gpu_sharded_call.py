"""ONE Rolling.Aggregate over a frame the CALLER holds as row-range shards, one per device (bowgpu_rolling_aggregate_sharded,
bow_amd/csrc/sharded_call.cpp).  On a one-GPU box the same device id is listed k times: k library threads, k contexts and streams, the
records exchanged in host memory, every rank writing its own output buffers.  The owned slots, concatenated in rank order, are checked
against the oracle, against the one-device call of the whole frame (bit for bit wherever no window took an order-free form) and against
the shard protocol driven by hand over the same per-rank columns (sharded.run_local)."""
import os
import threading

import numpy as np
import pytest

from bow_amd import capi, sharded
from oracle import pyoracle as orc
from test_gpu_aggregate import ORDER_SENSITIVE, compare
from test_gpu_fuzz import aggregate_cases
from test_gpu_multi import PLAIN, TW, frame, same_bits
from tolerance import order_free_bounds

pytestmark = pytest.mark.gpu


class Owned:
    """output i of a sharded call: slots [0, windows_owned) of every rank, concatenated in rank order (what compare() / same_bits() read)"""

    def __init__(self, outs, decisions, i):
        vals, valid = [], []
        self.null_count, self.type = 0, outs[0][i].type
        for o, d in zip(outs, decisions):
            n = max(d.windows_owned, 0)
            assert o[i].length == n, (o[i].length, n)
            if n:
                v, _ = o[i].host_arrays()
                vals.append(v.view(np.uint64)[:n].copy())
                valid.append(o[i].valid_mask()[:n])
            self.null_count += o[i].null_count
            if n and o[i].type:
                assert o[i].type == self.type
        self.vals = np.concatenate(vals) if vals else np.zeros(0, np.uint64)
        self.valid = np.concatenate(valid) if valid else np.zeros(0, bool)
        self.length = len(self.vals)

    def host_arrays(self):
        dt = np.int64 if self.type == capi.INT64 else np.float64
        return self.vals.view(dt), np.packbits(self.valid, bitorder="little")

    def valid_mask(self):
        return self.valid


def views(ccols, bounds):
    """per-rank column views of the frame's columns (same residency, same buffers): rows [bounds[r], bounds[r + 1])"""
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        out.append([capi.Column(c.values, c.validity, c.type, c.offset + a, b - a, -1 if c.validity is not None else 0) for c in ccols])
    return out


def check_against_oracle_and_one_device(outs, ds, info, ocols, ccols, interval, aggs, offset, inclusive, label, strict=False):
    exp, nic = orc.aggregate(ocols, 0, interval, aggs, offset=offset, inclusive=inclusive)
    one, info1 = capi.rolling_aggregate(ccols, 0, interval, aggs, offset=offset, inclusive=inclusive, strict_order=strict)
    assert (info.s0, info.num_windows, info.new_interval_col, info.inclusive) == \
        (info1.s0, info1.num_windows, info1.new_interval_col, info1.inclusive), label
    assert info.new_interval_col == nic, label
    assert sum(max(d.windows_owned, 0) for d in ds) == info.num_windows, label
    bounds = None
    if info.long_windows:
        bounds = order_free_bounds(ocols, 0, interval, aggs, offset=offset, inclusive=inclusive, ref=exp)
    for i, (a, w) in enumerate(zip(aggs, exp)):
        g = Owned(outs, ds, i)
        exact = info.long_windows == 0 or a[0] not in ORDER_SENSITIVE
        compare("%s %s" % (label, a[0]), g, w, exact=exact, bound=None if exact else bounds[i])
        if info.long_windows == 0 and info1.long_windows == 0:
            same_bits("%s %s vs one device" % (label, a[0]), g, one[i])


class Provider(sharded.GpuProvider):
    """sharded.GpuProvider with Options.inclusive as the call has it"""

    def __init__(self, cols, interval, aggs, offset, inclusive, strict):
        super().__init__(cols, 0, interval, aggs, offset=offset, strict_order=strict)
        self._opts.inclusive = int(bool(inclusive))


def check_against_run_local(vs, outs, ds, interval, aggs, offset, inclusive, label):
    provs = [Provider(v, interval, aggs, offset, inclusive, False) for v in vs]
    hand = sharded.run_local(provs)
    F = [f for f, _ in capi.ShardDecision._fields_]
    for r, (d, h) in enumerate(zip(ds, hand)):
        assert [getattr(d, f) for f in F] == [getattr(h, f) for f in F], (label, r)
        n = max(d.windows_owned, 0)
        for i in range(len(aggs)):
            gv, _ = outs[r][i].host_arrays()
            hv, _ = provs[r].outs[i].host_arrays()
            assert np.array_equal(gv.view(np.uint64)[:n], hv.view(np.uint64)[:n]), (label, r, i)
            assert np.array_equal(outs[r][i].valid_mask()[:n], provs[r].outs[i].valid_mask()[:n]), (label, r, i)


def random_bounds(rng, n, k):
    """k contiguous row ranges: empty ranks, one-row ranks, cuts inside windows, and (clustered cuts) windows over three or more ranks"""
    if rng.random() < 0.3 and n > 0:
        c = int(rng.integers(0, n + 1))
        cuts = np.clip(c + rng.integers(-3, 4, k - 1), 0, n)
    else:
        cuts = rng.integers(0, n + 1, k - 1)
    cuts = sorted(int(x) for x in cuts)
    if k > 2 and n > 2 and rng.random() < 0.3:
        cuts[0] = max(0, cuts[1] - 1)      # a one-row (or empty) rank
    return [0] + cuts + [n]


@pytest.mark.parametrize("seed", range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")) // 4))
def test_fuzz_cases_as_one_sharded_call(seed):
    """test_fuzz_aggregate's seeded cases cut into k in {1, 2, 3, 4, 8} ranks at random (the test's own rng), each rank a view of
    the case's columns in the case's residency"""
    rng = np.random.default_rng(17000 + seed)
    served = 0
    for ccols, ocols, n, interval, aggs, offset, inclusive, label in aggregate_cases(seed):
        k = int([1, 2, 3, 4, 8][int(rng.integers(0, 5))])
        bounds = random_bounds(rng, n, k)
        vs = views(ccols, bounds)
        label = "%s k=%d bounds=%s" % (label, k, bounds)
        out_res = capi.DEVICE if ccols[0].residency == capi.DEVICE else capi.HOST
        has_mode = any(a[0] == "Mode" for a in aggs)
        if has_mode or len(aggs) > 16:
            with pytest.raises(capi.BowGpuError) as e:
                capi.rolling_aggregate_sharded(vs, 0, interval, aggs, [0] * k, offset=offset, inclusive=inclusive, out_residency=out_res)
            assert e.value.code == -9, (label, e.value)
            continue
        outs, ds, info = capi.rolling_aggregate_sharded(vs, 0, interval, aggs, [0] * k, offset=offset, inclusive=inclusive, out_residency=out_res)
        check_against_oracle_and_one_device(outs, ds, info, ocols, ccols, interval, aggs, offset, inclusive, label)
        check_against_run_local(vs, outs, ds, interval, aggs, offset, inclusive, label)
        served += n >= 2
        if rng.random() < 0.3:   # strict_order: row order across every boundary, or declined with the stated reasons
            try:
                outs, ds, info = capi.rolling_aggregate_sharded(vs, 0, interval, aggs, [0] * k, offset=offset, inclusive=inclusive,
                                                                strict_order=True, out_residency=out_res)
            except capi.BowGpuError as e:
                assert e.code == -9 and ("three or more" in e.message or "2^20" in e.message), (label, e.message)
                continue
            assert info.long_windows == 0, label
            check_against_oracle_and_one_device(outs, ds, info, ocols, ccols, interval, aggs, offset, inclusive, label + " strict", strict=True)
    assert served >= 10, served


def rank_columns(ts, vals, valid, bounds, residency):
    """per-rank columns, each rank in allocations of its own"""
    typ = capi.INT64 if vals.dtype == np.int64 else capi.FLOAT64
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        t, v = np.ascontiguousarray(ts[a:b]), np.ascontiguousarray(vals[a:b])
        bm = None if valid is None else np.packbits(valid[a:b], bitorder="little")
        if residency == capi.HOST_PINNED:
            tp = capi.page_aligned(len(t), np.int64); tp[:] = t
            vp = capi.page_aligned(len(v), v.dtype); vp[:] = v
            bp = None
            if bm is not None:
                bp = capi.page_aligned(len(bm), np.uint8); bp[:] = bm
            cols = [capi.Column(tp, None, capi.INT64, 0, b - a, 0), capi.Column(vp, bp, typ, 0, b - a, -1)]
            if b > a:
                cols = [c.pin() for c in cols]
        else:
            cols = [capi.Column(t, None, capi.INT64, 0, b - a, 0), capi.Column(v, bm, typ, 0, b - a, -1 if bm is not None else 0)]
            if residency == capi.DEVICE:
                cols = [c.to_device() for c in cols]
        out.append(cols)
    return out


@pytest.mark.parametrize("residency", [capi.HOST, capi.HOST_PINNED, capi.DEVICE], ids=["host", "pinned", "device"])
@pytest.mark.parametrize("mode", ["dense", "irregular", "negative", "gappy"])
def test_residencies_and_timestamp_shapes(mode, residency):
    """150 000 rows x {dense, irregular, negative (the second round of the protocol), gappy} x plain exclusive / time-weighted
    inclusive / plain inclusive x four intervals x world 4 and 8; outputs DEVICE and HOST"""
    n = 150_000
    ts, vals, valid = frame(n, mode, 11)
    bm = np.packbits(valid, bitorder="little")
    ccols = [capi.Column(ts, None, capi.INT64), capi.Column(vals, bm, capi.FLOAT64, 0, n, -1)]
    ocols = [orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)]
    rng = np.random.default_rng(23)
    for k in (4, 8):
        bounds = [0] + sorted(int(x) for x in rng.integers(1, n, k - 1)) + [n]
        rcols = rank_columns(ts, vals, valid, bounds, residency)
        try:
            j = 0
            for aggs, inclusive in [(PLAIN, False), (TW, True), (PLAIN, True)]:
                for interval, offset in [(7, 0), (100, 13), (3_000, -5), (90_000, 1)]:
                    out_res = (capi.DEVICE, capi.HOST)[j % 2]
                    j += 1
                    label = "%s I=%d k=%d out=%d" % (mode, interval, k, out_res)
                    outs, ds, info = capi.rolling_aggregate_sharded(rcols, 0, interval, aggs, [0] * k, offset=offset, inclusive=inclusive,
                                                                    out_residency=out_res)
                    check_against_oracle_and_one_device(outs, ds, info, ocols, ccols, interval, aggs, offset, inclusive, label)
        finally:
            for cols in rcols:
                for c in cols:
                    c.unpin()


def poisoned_outs(ds, naggs, residency):
    outs = [[capi.OutColumn(max(d.windows_local, 0), residency) for _ in range(naggs)] for d in ds]
    if residency == capi.DEVICE:
        for row in outs:
            for o in row:
                capi.check(capi.lib().bowgpu_memset(capi.C.c_void_p(o.values.ptr), 0xA5, capi.C.c_int64(o.values.nbytes)))
                capi.check(capi.lib().bowgpu_memset(capi.C.c_void_p(o.validity.ptr), 0xA5, capi.C.c_int64(o.validity.nbytes)))
    return outs


def check_tails(cols_by_rank, interval, aggs, offset, label, residency):
    layout = capi.sharded_layout(cols_by_rank, 0, interval, aggs, [0] * len(cols_by_rank), offset=offset)
    outs = poisoned_outs(layout, len(aggs), residency)
    outs, ds, info = capi.rolling_aggregate_sharded(cols_by_rank, 0, interval, aggs, [0] * len(cols_by_rank), offset=offset, outs_by_rank=outs)
    F = [f for f, _ in capi.ShardDecision._fields_]
    for r, (a, d) in enumerate(zip(layout, ds)):
        assert [getattr(a, f) for f in F] == [getattr(d, f) for f in F], (label, r)
    for r, d in enumerate(ds):
        wrote = (max(d.windows_local, 0) + 7) // 8
        for i, o in enumerate(outs[r]):
            n = o.length
            assert n == max(d.windows_owned, 0), (label, r, i)
            if residency == capi.DEVICE:
                bm = o.validity.to_numpy(np.uint8, wrote)
                vals = o.values.to_numpy(np.uint64, max(d.windows_local, 0))
            else:
                bm, vals = o.validity[:wrote], o.values[:max(d.windows_local, 0)]
            bits = np.unpackbits(bm, bitorder="little") if wrote else np.zeros(0, np.uint8)
            assert not bits[n:].any(), (label, r, i, "bits at or past length")
            assert o.null_count == int((bits[:n] == 0).sum()), (label, r, i, o.null_count)
            if d.drops_last:
                assert vals[n] == 0, (label, r, i, "the dropped slot's value")
    # a capacity one short of windows_local
    for r, d in enumerate(layout):
        if d.windows_local >= 1:
            short = [[capi.OutColumn(max(q.windows_local, 0) - (1 if q_r == r else 0), residency) for _ in aggs] for q_r, q in enumerate(layout)]
            with pytest.raises(capi.BowGpuError) as e:
                capi.rolling_aggregate_sharded(cols_by_rank, 0, interval, aggs, [0] * len(cols_by_rank), offset=offset, outs_by_rank=short)
            assert e.value.code == -10 and str(d.windows_local) in e.value.message, (label, r, e.value)
            break
    return outs, ds, info


def host_rank(ts, vals=None, valid=None):
    ts = np.asarray(ts, np.int64)
    if vals is None:
        vals = np.arange(len(ts), dtype=np.float64) * 0.5 - 3
    bm = None if valid is None else np.packbits(valid, bitorder="little")
    return [capi.Column(ts, None, capi.INT64, 0, len(ts), 0), capi.Column(np.asarray(vals), bm, capi.FLOAT64, 0, len(ts), -1 if bm is not None else 0)]


@pytest.mark.parametrize("residency", [capi.DEVICE, capi.HOST], ids=["device", "host"])
def test_tails_layout_and_capacity(residency):
    aggs = PLAIN
    rng = np.random.default_rng(4)
    # a gap of many empty windows between two ranks
    a, b = np.arange(0, 1000, 3), np.arange(50_000, 51_000, 3)
    cols = [host_rank(a, valid=rng.random(len(a)) > 0.3), host_rank(b, valid=rng.random(len(b)) > 0.3)]
    _, ds, _ = check_tails(cols, 10, aggs, 0, "gap", residency)
    assert ds[1].lead_empty_windows > 1000
    # a rank whose rows all fall in one window shared with both neighbours (offset 3: windows [103, 113), ...)
    t = np.arange(0, 300)
    cols = [host_rank(t[:105], valid=rng.random(105) > 0.5), host_rank(t[105:109], valid=np.array([0, 1, 0, 0], bool)),
            host_rank(t[109:], valid=rng.random(191) > 0.5)]
    outs, ds, _ = check_tails(cols, 10, aggs, 3, "middle", residency)
    assert ds[1].first_window_id == ds[1].last_window_id and ds[1].windows_owned == 0 and ds[1].drops_last and ds[2].seed_first_rank == 0
    assert ds[0].drops_last
    # ... the same against the oracle and the one-device call
    vals = np.concatenate([c[1].values for c in cols])
    valid = np.concatenate([np.unpackbits(c[1].validity, bitorder="little")[:c[1].length] for c in cols]).astype(bool)
    bm = np.packbits(valid, bitorder="little")
    whole = [capi.Column(t.astype(np.int64), None, capi.INT64), capi.Column(vals, bm, capi.FLOAT64, 0, 300, -1)]
    owhole = [orc.Column(t.astype(np.int64), None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)]
    outs, ds, info = capi.rolling_aggregate_sharded(cols, 0, 10, aggs, [0] * 3, offset=3, out_residency=residency)
    check_against_oracle_and_one_device(outs, ds, info, owhole, whole, 10, aggs, 3, False, "middle")
    # every rank empty
    empty = [host_rank(np.zeros(0, np.int64)) for _ in range(3)]
    outs, ds, info = check_tails(empty, 10, aggs, 0, "empty", residency)
    assert info.num_windows == 0 and all(o.length == 0 for row in outs for o in row)
    # world 1 is the one-device call
    n = 5000
    ts, v, valid = frame(n, "irregular", 2)
    cols = [host_rank(ts, v, valid)]
    outs, ds, info = check_tails(cols, 25, aggs, 4, "world 1", residency)
    one, _ = capi.rolling_aggregate(cols[0], 0, 25, aggs, offset=4)
    for i, a in enumerate(aggs):
        same_bits("world 1 " + a[0], Owned(outs, ds, i), one[i])


def test_errors():
    n = 40_000
    ts, vals, valid = frame(n, "irregular", 9)
    bounds = [0, 10_000, 25_000, n]
    cols = rank_columns(ts, vals, valid, bounds, capi.HOST)
    call = lambda cs, ids=None, aggs=PLAIN: capi.rolling_aggregate_sharded(cs, 0, 10, aggs, ids or [0] * len(cs), out_residency=capi.HOST)
    # two ranks swapped
    with pytest.raises(capi.BowGpuError) as e:
        call([cols[0], cols[2], cols[1]])
    assert e.value.code == -14
    # not ascending inside a rank (found by that rank's pass)
    bad = ts.copy()
    bad[12_345] = bad[12_344] - 50
    with pytest.raises(capi.BowGpuError) as e:
        call(rank_columns(bad, vals, valid, bounds, capi.HOST))
    assert e.value.code == -14
    # a null in one rank's interval column
    tv = np.ones(15_000, bool)
    tv[77] = False
    nts = [capi.Column(np.ascontiguousarray(ts[10_000:25_000]), np.packbits(tv, bitorder="little"), capi.INT64, 0, 15_000, -1), cols[1][1]]
    with pytest.raises(capi.BowGpuError) as e:
        call([cols[0], nts, cols[2]])
    assert e.value.code == -13
    # a device id past the last device
    with pytest.raises(capi.BowGpuError) as e:
        call(cols, [0, capi.device_count(), 0])
    assert e.value.code == -11
    # a rank whose value column has another type: BOWGPU_ERR_ARG (include/bowgpu.h: every rank has the same schema)
    other = [cols[1][0], capi.Column(np.ascontiguousarray(vals[10_000:25_000]).astype(np.int64), None, capi.INT64)]
    with pytest.raises(capi.BowGpuError) as e:
        call([cols[0], other, cols[2]])
    assert e.value.code == -10 and "rank 1" in e.value.message
    # a DEVICE buffer of a rank that does not live on that rank's device: only checkable with a second device
    if capi.device_count() > 1:
        dcols = rank_columns(ts, vals, valid, bounds, capi.DEVICE)
        with pytest.raises(capi.BowGpuError) as e:
            call(dcols, [0, 1, 0])
        assert e.value.code == -10 and "rank 1" in e.value.message
    # Mode
    with pytest.raises(capi.BowGpuError) as e:
        call(cols, aggs=PLAIN + [("Mode", 1)])
    assert e.value.code == -9


def test_independent_of_the_device_list_and_thread_safe():
    n = 200_000
    ts, vals, valid = frame(n, "irregular", 21)
    bounds = [0, 50_000, 120_000, 160_000, n]
    rcols = rank_columns(ts, vals, valid, bounds, capi.DEVICE)
    ref, dref, iref = capi.rolling_aggregate_sharded(rcols, 0, 25, PLAIN, [0] * 4)
    counts, ranks = capi.fanout_counts(), capi.last_call_ranks()
    with capi.devices([0, 0], min_rows=1000):
        got, dgot, igot = capi.rolling_aggregate_sharded(rcols, 0, 25, PLAIN, [0] * 4)
        assert capi.get_devices() == [0, 0]
    assert capi.fanout_counts() == counts and capi.last_call_ranks() == ranks
    for i, a in enumerate(PLAIN):
        same_bits("with a device list " + a[0], Owned(got, dgot, i), Owned(ref, dref, i))
    # two threads, each with its own frame, at the same time
    frames = []
    for t in range(2):
        ts_t, v_t, valid_t = frame(150_000, ["gappy", "dense"][t], 30 + t)
        bm = np.packbits(valid_t, bitorder="little")
        exp, _ = orc.aggregate([orc.Column(ts_t, None, orc.INT64), orc.Column(v_t, bm, orc.FLOAT64)], 0, 40, PLAIN)
        frames.append((rank_columns(ts_t, v_t, valid_t, [0, 30_000, 90_000, 150_000], [capi.DEVICE, capi.HOST][t]), exp))
    errors = []

    def work(t):
        try:
            cols, exp = frames[t]
            for _ in range(5):
                outs, ds, info = capi.rolling_aggregate_sharded(cols, 0, 40, PLAIN, [0] * 3, out_residency=[capi.DEVICE, capi.HOST][t])
                for i, (a, w) in enumerate(zip(PLAIN, exp)):
                    compare("thread %d %s" % (t, a[0]), Owned(outs, ds, i), w)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[0]
