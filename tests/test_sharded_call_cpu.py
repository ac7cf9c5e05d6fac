"""bowgpu_rolling_aggregate_sharded on the CPU side: the layout query on host-resident interval columns is host arithmetic (no GPU
needed) and answers what bowgpu_shard_plan decides from the ranks' row counts and first / last timestamps; bad arguments are
BOWGPU_ERR_ARG; the full call has no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from bow_amd import capi

AGGS = [("WindowStart", 0), ("Sum", 1), ("ArithmeticMean", 1)]


def shards(ts, cuts, with_values=True):
    """per-rank host columns of the frame ts cut at `cuts`"""
    bounds = [0] + list(cuts) + [len(ts)]
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        t = np.ascontiguousarray(ts[a:b])
        v = np.arange(a, b, dtype=np.float64)
        out.append([capi.Column(t, None, capi.INT64), capi.Column(v, None, capi.FLOAT64)] if with_values else [capi.Column(t, None, capi.INT64)])
    return out


def plan_by_hand(cols_by_rank, interval, offset):
    """bowgpu_shard_plan over records made of each rank's row count and first / last timestamp.  The records say 'built with s0
    known' (flags bit 0): the decisions of the settled protocol, which is what the layout query answers (retry_with_s0 = 0)."""
    world = len(cols_by_rank)
    recs = (capi.ShardRecord * world)()
    for r, cols in enumerate(cols_by_rank):
        t = cols[0]
        recs[r].nrows = t.length
        recs[r].naggs = len(AGGS)
        recs[r].flags = 1
        if t.length:
            recs[r].first_ts = int(t.values[t.offset])
            recs[r].last_ts = int(t.values[t.offset + t.length - 1])
    out = []
    for r in range(world):
        d = capi.ShardDecision()
        capi.check(capi.lib().bowgpu_shard_plan(recs, world, r, C.c_int64(interval), C.c_int64(offset), C.byref(d)))
        out.append(d)
    return out


def fields(d):
    return tuple(getattr(d, f) for f, _ in capi.ShardDecision._fields_)


def test_layout_query_is_the_shard_plan_of_the_ranks_first_and_last_timestamps():
    rng = np.random.default_rng(5)
    checked = 0
    for case in range(300):
        n = int(rng.integers(0, 400))
        ts = np.cumsum(rng.integers(0, 9, n)).astype(np.int64)
        if rng.random() < 0.4:
            ts -= int(rng.integers(0, 3 * max(n, 1)))           # negative timestamps: rows below the first window start
        if n and rng.random() < 0.3:
            ts[n // 2:] += int(rng.integers(100, 5000))          # a gap of empty windows
        interval = int([1, 3, 7, 10, 64, 1000][int(rng.integers(0, 6))])
        offset = int(rng.integers(-3 * interval, 3 * interval + 1))
        world = int([1, 2, 3, 4, 8][int(rng.integers(0, 5))])
        cuts = np.sort(rng.integers(0, n + 1, world - 1))          # empty ranks and one-row ranks come with it
        cols_by_rank = shards(ts, cuts)
        got = capi.sharded_layout(cols_by_rank, 0, interval, AGGS, [0] * world, offset=offset)
        want = plan_by_hand(cols_by_rank, interval, offset)
        label = "case=%d n=%d I=%d off=%d cuts=%s" % (case, n, interval, offset, list(cuts))
        assert [fields(d) for d in got] == [fields(d) for d in want], label
        assert all(d.retry_with_s0 == 0 for d in got), label
        owned = sum(max(d.windows_owned, 0) for d in got)
        assert owned == got[0].num_windows, label
        checked += 1
    assert checked == 300


def test_layout_query_reports_what_the_call_would_decline():
    ts = np.arange(100, dtype=np.int64)
    cols = shards(ts, [40, 70])
    # two ranks swapped: not ascending across ranks
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout([cols[1], cols[0], cols[2]], 0, 10, AGGS, [0, 0, 0])
    assert e.value.code == -14
    # a null in one rank's interval column
    bm = np.packbits(np.arange(30) != 7, bitorder="little")
    bad = [capi.Column(np.ascontiguousarray(ts[40:70]), bm, capi.INT64, 0, 30, -1), cols[1][1]]
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout([cols[0], bad, cols[2]], 0, 10, AGGS, [0, 0, 0])
    assert e.value.code == -13
    # Mode
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout(cols, 0, 10, AGGS + [("Mode", 1)], [0, 0, 0])
    assert e.value.code == -9
    # the one-device call's validation errors
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout(cols, 0, 0, AGGS, [0, 0, 0])
    assert e.value.code == -1
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout(cols, 0, 10, [("Sum", 1)], [0, 0, 0])
    assert e.value.code == -5
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout(cols, 0, 10, [], [0, 0, 0])
    assert e.value.code == -4
    # a rank whose value column has another type
    other = [cols[1][0], capi.Column(np.arange(30, dtype=np.int64), None, capi.INT64)]
    with pytest.raises(capi.BowGpuError) as e:
        capi.sharded_layout([cols[0], other, cols[2]], 0, 10, AGGS, [0, 0, 0])
    assert e.value.code == -10


def test_bad_arguments():
    ts = np.arange(50, dtype=np.int64)
    cols = shards(ts, [25])
    world, ncols, carrs, cptrs, ids, aarr = capi._sharded_args(cols, [0, 0], AGGS)
    dec = (capi.ShardDecision * 64)()
    info = capi.AggInfo()
    opts = capi.Options(0, 0, 0)
    L = capi.lib()
    call = lambda cp, ip, w, nc, d: L.bowgpu_rolling_aggregate_sharded(cp, ip, w, nc, 0, C.c_int64(10), C.byref(opts), aarr, len(AGGS),
                                                                          None, d, C.byref(info))
    assert call(cptrs, ids, 2, ncols, dec) == 0
    assert call(None, ids, 2, ncols, dec) == -10
    assert call(cptrs, None, 2, ncols, dec) == -10
    assert call(cptrs, ids, 2, ncols, None) == -10
    assert call(cptrs, ids, 0, ncols, dec) == -10
    assert call(cptrs, ids, -1, ncols, dec) == -10
    assert call(cptrs, ids, 2, 0, dec) == -10
    assert call(cptrs, ids, 2, -3, dec) == -10
    big = [cols[0]] + shards(np.zeros(0, np.int64), []) * 64   # (one rank of rows, the rest empty)
    _, _, _, bptrs, bids, _ = capi._sharded_args(big, [0] * 65, AGGS)
    assert call(bptrs, bids, 65, ncols, dec) == -10
    assert call(bptrs, bids, 64, ncols, dec) == 0   # (64 ranks is the limit, and fine)
    assert dec[0].windows_owned == 3 and all(dec[r].windows_local == 0 for r in range(1, 64))


def test_full_call_has_no_cpu_fallback():
    ts = np.arange(50, dtype=np.int64)
    cols = shards(ts, [20])
    try:
        n = capi.device_count()
    except capi.BowGpuError:
        n = 0
    ids = [0, 0] if n == 0 else [0, n]   # without a GPU every id fails; with one, an id past the last device does
    with pytest.raises(capi.BowGpuError) as e:
        capi.rolling_aggregate_sharded(cols, 0, 10, AGGS, ids, out_residency=capi.HOST,
                                       outs_by_rank=[[capi.OutColumn(8) for _ in AGGS] for _ in cols])
    assert e.value.code == -11, e.value
