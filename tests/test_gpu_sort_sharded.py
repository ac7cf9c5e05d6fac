"""bowgpu_sort_by_col_sharded on the GPU (bow_amd/csrc/sort_shard_api.cpp, sort_shard.hip), all ranks on ONE device unless a case says
otherwise (device_ids = [0] * world: the path a one-GPU box runs).  Every case is compared bit for bit with capi.sort_by_col of the
concatenated frame on device 0 - values as raw 64-bit payloads, validity byte for byte with clear padding bits, null_count per rank -
and its key with numpy's stable argsort of the key image.  A row-number column rides along in every case: stability is equality of
that column."""
import numpy as np
import pytest

from bow_amd import capi
from test_gpu_sort import col_of, image, place, stable_perm

pytestmark = pytest.mark.gpu

T = capi.MERGE_TILE_ROWS          # output rows per workgroup of merge_runs_kernel
RNG = np.random.default_rng(20251018)
POISON = 0x5A5A5A5A5A5A5A5A


def shard(key, extra=(), offset=0):
    """one rank's logical columns: the key, its rows' numbers within the rank (filled in by build), extra (values, valid | None) pairs"""
    return {"key": np.ascontiguousarray(key), "extra": list(extra), "offset": offset}


def with_values(key, offset=0, ncols=2, density=0.3):
    """a shard with ncols value columns, alternately Float64 / Int64, nulls at `density`; the last one without a bitmap"""
    n = len(key)
    extra = []
    for i in range(ncols):
        vals = RNG.standard_normal(n) if i % 2 == 0 else RNG.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)
        valid = None if i == ncols - 1 else RNG.random(n) >= density
        extra.append((vals, valid))
    return shard(key, extra, offset)


def build(shards):
    """-> (ranks of host Columns, logical columns of the concatenated frame as (values, valid | None) pairs)"""
    ranks, logical, row0 = [], None, 0
    for s in shards:
        n, off = len(s["key"]), s["offset"]
        cols = [(s["key"], None), (np.arange(row0, row0 + n, dtype=np.int64), None)] + s["extra"]
        if logical is None:
            logical = [{"vals": [], "mask": [], "bitmap": False} for _ in cols]
        rank = []
        for i, (vals, valid) in enumerate(cols):
            vals = np.ascontiguousarray(vals)
            buf = np.concatenate([np.full(off, 77, vals.dtype), vals])           # rows in front of the Arrow offset
            vbuf = None if valid is None else np.concatenate([RNG.random(off) < 0.5, valid])
            typ = capi.INT64 if vals.dtype == np.int64 else capi.FLOAT64
            rank.append(col_of(buf, vbuf, typ, off, n))
            logical[i]["vals"].append(vals)
            logical[i]["mask"].append(np.ones(n, bool) if valid is None else valid)
            logical[i]["bitmap"] |= valid is not None
        ranks.append(rank)
        row0 += n
    frame = [(np.concatenate(c["vals"]), np.concatenate(c["mask"]) if c["bitmap"] else None) for c in logical]
    return ranks, frame


def one_device(frame):
    """capi.sort_by_col of the concatenated frame on device 0 -> (per column (raw uint64 values, valid mask, type), unchanged)"""
    cols = [col_of(v, m, capi.INT64 if v.dtype == np.int64 else capi.FLOAT64).to_device() for v, m in frame]
    outs, unchanged = capi.sort_by_col(cols, 0, out_residency=capi.DEVICE)
    if unchanged:
        return None, True
    return [(o.host_arrays()[0].view(np.uint64), o.valid_mask(), o.type) for o in outs], False


def run(shards, residency=capi.DEVICE, out_residency=capi.DEVICE, ids=None):
    ranks, frame = build(shards)
    placed = [[place(c, residency) for c in rank] for rank in ranks]
    ids = [0] * len(shards) if ids is None else ids
    try:
        outs, unchanged = capi.sort_by_col_sharded(placed, 0, ids, out_residency=out_residency)
    finally:
        if residency == capi.HOST_PINNED:
            for rank in placed:
                for c in rank:
                    c.unpin()
    return frame, outs, unchanged


def raw_bytes(outs):
    return [(o.host_arrays()[0].view(np.uint64).copy(), o.host_arrays()[1].copy(), o.length, o.null_count, o.type) for rank in outs for o in rank]


def check(shards, name="", **kw):
    frame, outs, unchanged = run(shards, **kw)
    key = frame[0][0]
    n = len(key)
    perm = stable_perm(key) if n else np.zeros(0, np.int64)
    img = image(key) if n else np.zeros(0, np.uint64)
    in_order = not (img[1:] < img[:-1]).any()
    want, ref_unchanged = (None, True) if n < 2 else one_device(frame)
    assert unchanged == ref_unchanged == in_order, (name, unchanged, ref_unchanged, in_order)
    if unchanged:
        return outs
    at = 0
    for r, s in enumerate(shards):
        nr = len(s["key"])
        for i, o in enumerate(outs[r]):
            wbits, wmask, wtype = want[i]
            assert o.length == nr and o.type == wtype, (name, r, i, o.length, o.type)
            gv, gb = o.host_arrays()
            gbits = gv.view(np.uint64)
            bad = np.flatnonzero(gbits != wbits[at:at + nr])
            assert bad.size == 0, (name, r, i, bad[:10])                         # raw payloads, null slots (0) included
            wb = np.packbits(wmask[at:at + nr], bitorder="little") if nr else np.zeros(0, np.uint8)
            assert np.array_equal(gb, wb), (name, r, i)                          # validity byte for byte: the padding bits are clear
            assert o.null_count == int((~wmask[at:at + nr]).sum()), (name, r, i, o.null_count)
        # the key and the row numbers against numpy's stable order
        assert np.array_equal(outs[r][0].host_arrays()[0].view(np.uint64), key.view(np.uint64)[perm[at:at + nr]]), (name, r)
        assert np.array_equal(outs[r][1].host_arrays()[0], perm[at:at + nr]), (name, r)
        at += nr
    return outs


def keys_for(lengths, lo, hi):
    return [RNG.integers(lo, hi, n, dtype=np.int64) for n in lengths]


# ------------------------------------------------------------------ world and rank lengths
@pytest.mark.parametrize("lengths", [[10007], [4097, 63], [0, 4096, 65], [1, 64, 0, 4095, 10001], [65, 1, 0], [0, 0, 0], [0, 2, 0]],
                         ids=lambda v: "x".join(map(str, v)))
def test_world_and_rank_lengths(lengths):
    check([with_values(k) for k in keys_for(lengths, -1000, 1000)], "narrow")     # many ties
    check([shard(k) for k in keys_for(lengths, -2 ** 62, 2 ** 62)], "wide")


# ------------------------------------------------------------------ splitters and ties
def test_tie_groups_larger_than_a_rank():
    lengths = [63, 4097, 1, 4096, 65]
    check([with_values(k) for k in keys_for(lengths, 0, 4)], "keys 0..3")          # a cut inside a tie at every boundary
    check([shard(k) for k in keys_for([64, 64, 64], 0, 2)], "keys 0..1")


def test_all_keys_equal_is_unchanged_and_nothing_is_written():
    shards = [shard(np.full(n, 5, np.int64)) for n in (65, 0, 4097, 63)]
    frame, outs, unchanged = run(shards, out_residency=capi.HOST)
    assert unchanged
    for rank in outs:
        for o in rank:
            assert o.null_count == -1 and o.type == 0 and o.length == o.slots
            assert (o.values == POISON).all() and (o.validity == 0xA5).all()
    check(shards, "all equal")


def test_all_equal_but_one_smaller_key_on_the_last_rank():
    keys = [np.full(n, 5, np.int64) for n in (65, 4097, 63)]
    keys[-1][40] = 1
    check([with_values(k) for k in keys], "one smaller")


def test_one_rank_holds_every_small_key():
    """rank 1's keys all lie below everybody else's: destinations that receive nothing from some sources (empty pieces)"""
    keys = [RNG.integers(1000, 2000, 4096, dtype=np.int64), RNG.integers(0, 100, 9000, dtype=np.int64), RNG.integers(1000, 2000, 65, dtype=np.int64)]
    check([with_values(k) for k in keys], "small keys on rank 1")


# ------------------------------------------------------------------ the merge kernels
def sorted_over(n, lo=0, hi=1 << 20):
    return np.sort(RNG.integers(lo, hi, n, dtype=np.int64))


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1])
def test_two_overlapping_sorted_ranks(n):
    check([shard(sorted_over(n // 2)), shard(sorted_over(n - n // 2))], "total %d" % n)      # the frame has n rows
    check([with_values(sorted_over(n)), with_values(sorted_over(n))], "each %d" % n)       # every destination merges n rows


def test_run_of_one_against_two_tiles():
    left = np.arange(0, 2 * (2 * T + 1), 2, dtype=np.int64)
    check([shard(left), shard(np.array([2 * T + 1], np.int64))], "1 against 2T")
    check([shard(np.array([2 * T + 1], np.int64)), shard(left)], "2T against 1")


@pytest.mark.parametrize("world", [3, 5])
def test_interleaving_runs_with_a_carried_one(world):
    check([with_values(sorted_over(3000 + 100 * r)) for r in range(world)], "%d runs" % world)
    info = capi.sort_by_col_sharded_info()
    assert info.merged_ranks == world and info.merge_rounds == {3: 2, 5: 3}[world]      # every destination merges one run of every rank
    assert 1 <= info.splitter_rounds <= 65 and info.sort_passes == 0                    # (the ranks were in order: no radix pass)


def test_equal_keys_across_tiles_in_both_runs_left_wins():
    """destination 0 merges [3T fives of rank 0] with [10 ones + 3T fives of rank 1]: every diagonal of the merge path lies inside the
    tie, and rank 0's fives come first"""
    k0 = np.concatenate([np.full(3 * T, 5, np.int64), np.full(3 * T + 10, 9, np.int64)])
    k1 = np.concatenate([np.full(10, 1, np.int64), np.full(3 * T, 5, np.int64)])
    check([with_values(k0), with_values(k1)], "ties across tiles")


# ------------------------------------------------------------------ routes without a merge
def test_ranged_shuffled_shards():
    keys = [RNG.permutation(np.arange(r * 10000, r * 10000 + n, dtype=np.int64)) for r, n in enumerate([4097, 63, 5000])]
    check([with_values(k) for k in keys], "ranged")
    info = capi.sort_by_col_sharded_info()
    assert info.merge_rounds == 0 and info.merged_ranks == 0 and info.sort_passes > 0   # one piece per destination: the append alone


def test_sorted_shards_in_reverse_rank_order():
    for lengths in ([3000, 3000, 3000], [4097, 63, 3000]):
        keys = [np.arange(n, dtype=np.int64) + 100000 * (len(lengths) - r) for r, n in enumerate(lengths)]
        check([with_values(k) for k in keys], "reverse %s" % lengths)
        info = capi.sort_by_col_sharded_info()
        if len(set(lengths)) == 1:
            assert info.merge_rounds == 0 and info.merged_ranks == 0                    # destination d receives exactly rank (world - 1 - d)


def test_a_frame_in_order_is_unchanged_and_untouched():
    keys = [np.arange(0, 100, dtype=np.int64), np.zeros(0, np.int64), np.arange(99, 4200, dtype=np.int64), np.full(65, 4199, np.int64)]
    frame, outs, unchanged = run([with_values(k) for k in keys], out_residency=capi.HOST)
    assert unchanged
    for rank in outs:
        for o in rank:
            assert o.null_count == -1 and o.type == 0 and o.length == o.slots
            assert (o.values == POISON).all() and (o.validity == 0xA5).all()
    info = capi.sort_by_col_sharded_info()
    assert info.splitter_rounds == 0 and info.merge_rounds == 0                         # the call ended behind the local reads of the keys
    # ... and one row out of place across a rank boundary is not
    keys[2] = keys[2].copy()
    keys[2][0] = 98
    check([with_values(k) for k in keys], "one row early")


# ------------------------------------------------------------------ keys
def test_float_keys_with_signed_zeros_and_negatives():
    ks = []
    for n in (4097, 63, 3000):
        k = RNG.standard_normal(n) * 3
        k[RNG.random(n) < 0.2] = 0.0
        k[RNG.random(n) < 0.2] = -0.0
        ks.append(k)
    check([with_values(k) for k in ks], "float")          # -0.0 / +0.0 tie across ranks: each keeps its bits (raw payloads compared)


def test_int_keys_using_all_eight_bytes():
    ks = [RNG.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True) for n in (4097, 65, 1000)]
    ks[0][:2] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    check([with_values(k) for k in ks], "all eight bytes")


def test_nan_on_the_last_rank_only():
    ks = [RNG.standard_normal(n) for n in (100, 65, 300)]
    ks[-1][7] = np.nan
    with pytest.raises(capi.BowGpuError) as e:
        run([shard(k) for k in ks])
    assert e.value.code == -9 and "NaN" in e.value.message


def test_null_key_on_one_rank():
    ranks, _ = build([shard(k) for k in keys_for([100, 65, 300], 0, 1000)])
    valid = np.ones(65, bool)
    valid[[3, 40]] = False
    ranks[1][0] = col_of(ranks[1][0].values, valid, capi.INT64, 0, 65)
    placed = [[c.to_device() for c in rank] for rank in ranks]           # (the count is not known before the device has counted)
    with pytest.raises(capi.BowGpuError) as e:
        capi.sort_by_col_sharded(placed, 0, [0, 0, 0], out_residency=capi.DEVICE)
    assert e.value.code == -16 and e.value.message == "column to sort by has 2 nil values"


# ------------------------------------------------------------------ value columns
@pytest.mark.parametrize("offsets", [(0, 0, 0), (3, 13, 0), (13, 3, 13)])
def test_value_columns_with_nulls_at_arrow_offsets(offsets):
    """pieces meet inside validity bytes at the destination; five columns are two gather groups"""
    lengths = [4097, 63, 1001]
    check([with_values(k, offset=off, ncols=3) for k, off in zip(keys_for(lengths, 0, 500), offsets)], "offsets %s" % (offsets,))
    check([with_values(np.sort(k), offset=off, ncols=3) for k, off in zip(keys_for(lengths, 0, 500), offsets)], "sorted ranks, offsets %s" % (offsets,))


# ------------------------------------------------------------------ residency, determinism
@pytest.mark.parametrize("residency", [capi.DEVICE, capi.HOST_PINNED, capi.HOST], ids=["device", "registered", "pageable"])
def test_residencies(residency):
    keys = keys_for([4097, 63, 1001], 0, 500)
    keys[1] = np.sort(keys[1])                                           # one rank in order: its input is pulled from where it lies
    check([with_values(k, offset=3) for k in keys], "residency", residency=residency, out_residency=residency)


def test_the_same_call_twice_gives_the_same_bytes():
    shards = [with_values(k, ncols=3) for k in keys_for([4097, 4096, 65], 0, 50)]
    _, a, _ = run(shards)
    _, b, _ = run(shards)
    for x, y in zip(raw_bytes(a), raw_bytes(b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:]


# ------------------------------------------------------------------ what the sort is for
def test_sorted_shards_feed_the_sharded_rolling_call():
    aggs = [("WindowStart", 0), ("Sum", 2), ("Count", 2), ("Max", 2)]
    ts = [RNG.integers(0, 20000, n, dtype=np.int64) for n in (3000, 65, 2000)]
    shards = [with_values(k, ncols=1) for k in ts]
    for s in shards:                                                     # (a value column with nulls: with_values' last column has no bitmap)
        s["extra"] = [(s["extra"][0][0], RNG.random(len(s["key"])) >= 0.3)]
    frame, outs, unchanged = run(shards)
    assert not unchanged
    by_rank = [[capi.out_as_column(o) for o in rank] for rank in outs]
    got, decisions, _ = capi.rolling_aggregate_sharded(by_rank, 0, 10, aggs, [0, 0, 0])
    cols = [col_of(v, m, capi.INT64 if v.dtype == np.int64 else capi.FLOAT64).to_device() for v, m in frame]
    sorted_one, _ = capi.sort_by_col(cols, 0, out_residency=capi.DEVICE)
    want, _ = capi.rolling_aggregate([capi.out_as_column(o) for o in sorted_one], 0, 10, aggs, out_residency=capi.DEVICE)
    for i, w in enumerate(want):
        gv = np.concatenate([got[r][i].host_arrays()[0].view(np.uint64)[:decisions[r].windows_owned] for r in range(3)])
        gm = np.concatenate([got[r][i].valid_mask()[:decisions[r].windows_owned] for r in range(3)])
        wm = w.valid_mask()
        assert len(gv) == w.length and np.array_equal(gm, wm), aggs[i]
        assert np.array_equal(gv[gm], w.host_arrays()[0].view(np.uint64)[wm]), aggs[i]


# ------------------------------------------------------------------ two devices
def test_two_distinct_devices():
    if capi.device_count() < 2:
        pytest.skip("fewer than two devices")
    ranks, frame = build([with_values(k, offset=3) for k in keys_for([4097, 3000], 0, 500)])
    placed, outs = [], []
    for d, rank in enumerate(ranks):
        capi.set_device(d)
        placed.append([c.to_device() for c in rank])
        outs.append([capi.OutColumn(c.length, capi.DEVICE) for c in rank])
    try:
        _, unchanged = capi.sort_by_col_sharded(placed, 0, [0, 1], outs=outs)
        assert not unchanged
        got = []
        for d in range(2):
            capi.set_device(d)
            got.append([(o.host_arrays()[0].view(np.uint64).copy(), o.host_arrays()[1].copy(), o.null_count) for o in outs[d]])
    finally:
        capi.set_device(0)
    want, _ = one_device(frame)
    at = 0
    for d, rank in enumerate(ranks):
        nr = rank[0].length
        for i, (gbits, gb, nulls) in enumerate(got[d]):
            wbits, wmask, _ = want[i]
            assert np.array_equal(gbits, wbits[at:at + nr]), (d, i)
            assert np.array_equal(gb, np.packbits(wmask[at:at + nr], bitorder="little")), (d, i)
            assert nulls == int((~wmask[at:at + nr]).sum()), (d, i)
        at += nr
