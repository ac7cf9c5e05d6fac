"""configs[4] at its size through ONE call: 8 ranks x 1e9 dense rows, each rank in HBM allocations of its own, aggregated by
bowgpu_rolling_aggregate_sharded (bow_amd/csrc/sharded_call.cpp) with every rank listed on device 0 - the same rows, the same protocol as
tests/test_gpu_fullsize.py's config-4 test drives by hand, behind one C ABI call."""
import ctypes as C

import numpy as np
import pytest

from bow_amd import capi, sharded
from test_gpu_fullsize import _gpu_free_gb, _oracle_windows

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(1800)
def test_config4_eight_ranks_of_1e9_rows_as_one_sharded_call():
    capi.trim(True)
    if _gpu_free_gb() < 200:
        pytest.skip("needs 200 GB of free HBM (an MI355X has 288 GB), found %.0f GB" % _gpu_free_gb())
    world, R = 8, 1_000_000_000
    N = world * R
    interval, offset = 10, 3        # a window straddles every rank boundary
    aggs = [("WindowStart", 0), ("ArithmeticMean", 1)]
    bufs, cols_by_rank = [], []
    for r in range(world):
        tsb, vb = capi.DeviceBuffer(R * 8), capi.DeviceBuffer(R * 8)
        capi.check(capi.lib().bowgpu_gen_dense(C.c_int64(r * R), C.c_int64(R), C.c_uint64(42), C.c_void_p(tsb.ptr), C.c_void_p(vb.ptr)))
        bufs.append((tsb, vb))
        cols_by_rank.append([capi.Column(tsb, None, capi.INT64, 0, R, 0), capi.Column(vb, None, capi.FLOAT64, 0, R, 0)])
    s0 = sharded.first_window_start(0, interval, offset)
    W = (N - 1 - s0) // interval + 1
    outs, ds, info = capi.rolling_aggregate_sharded(cols_by_rank, 0, interval, aggs, [0] * world, offset=offset, out_residency=capi.DEVICE)
    assert info.s0 == s0 and info.num_windows == W and info.long_windows == 0

    # ownership is contiguous and covers W; WindowStart is the arithmetic progression on every rank
    covered = 0
    for r, d in enumerate(ds):
        assert d.s0 == s0 and d.num_windows == W
        assert d.first_slot_window_id == covered, (r, d.first_slot_window_id, covered)
        assert d.drops_last == (1 if r + 1 < world else 0)
        assert outs[r][0].length == d.windows_owned and outs[r][0].null_count == 0 and outs[r][1].null_count == 0
        ws = outs[r][0].values.to_numpy(np.int64, d.windows_owned)
        assert ws[0] == s0 + interval * d.first_slot_window_id and (np.diff(ws) == interval).all(), r
        del ws
        covered += d.windows_owned
    assert covered == W

    # checksum of checksums over the owned slots == the same over the shard protocol driven by hand on the same buffers
    provs = [sharded.GpuProvider(cols_by_rank[r], 0, interval, aggs, offset=offset) for r in range(world)]
    hand = sharded.run_local(provs)
    for i, k in enumerate(["WindowStart", "ArithmeticMean"]):
        mine, theirs = [0, 0], [0, 0]
        for r in range(world):
            assert hand[r].first_slot_window_id == ds[r].first_slot_window_id and hand[r].windows_owned == ds[r].windows_owned
            fs, nw = ds[r].first_slot_window_id, ds[r].windows_owned
            for acc, buf in ((mine, outs[r][i].values), (theirs, provs[r].outs[i].values)):
                x, sm = capi.checksum64(buf, nw, index_base=fs)
                acc[0] ^= x
                acc[1] = (acc[1] + sm) & 0xFFFFFFFFFFFFFFFF
        assert mine == theirs, k
    del provs

    # 2e6-row ranges around every boundary against the oracle, bit for bit, from the owning rank's buffer
    half = 1_000_000
    for r in range(1, world):
        g0, want = _oracle_windows(r * R - half, 2 * half, interval, offset, aggs, s0)
        nw = want[0].length
        lo, hi = g0 + 1, g0 + nw - 1            # (the range's edge windows are cut)
        for q in (r - 1, r):
            fs, n_own = ds[q].first_slot_window_id, ds[q].windows_owned
            a, b = max(lo, fs), min(hi, fs + n_own)
            assert a < b
            for i in range(2):
                gv = outs[q][i].values.to_numpy(np.uint64, b - a, first=a - fs)
                assert np.array_equal(gv, want[i].values[:nw].view(np.uint64)[a - g0:b - g0]), (r, q, i)
