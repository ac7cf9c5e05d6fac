"""Wall time per call of bowgpu_rolling_aggregate_sharded against the one-device bowgpu_rolling_aggregate (profiles/r07_*).

1e8 dense rows, interval 10, WindowStart + ArithmeticMean, device-resident columns and outputs.  First line: the one-device call over
the frame (the only line when the library has no bowgpu_rolling_aggregate_sharded, so the script runs on older commits too).  Then the
sharded call over the same rows as world = 2, 4, 8 per-rank allocations on device 0, and 8 ranks of 1e8 rows each next to the one-device
call over 8e8 rows.  Best of REPS calls after WARM warm-up calls; every timed call returns with its outputs complete (both entry points
synchronise before they return), measured by the host clock around the C call with its arguments built beforehand.
BOW_ROOT=<tree>: import bow_amd (binding + library) from another tree - an older commit's build, for the A/B in one session.
COMMIT: the sha printed in the first line."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.environ.get("BOW_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bow_amd import capi  # noqa: E402

N = int(os.environ.get("ROWS", "100000000"))
REPS, WARM = int(os.environ.get("REPS", "30")), 5
INTERVAL = 10
AGGS = [("WindowStart", 0), ("ArithmeticMean", 1)]


def best(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), sorted(t)[len(t) // 2]


def one_device(n):
    ts, val = capi.gen_dense(0, n)
    capi.synchronize()
    W = (n - 1) // INTERVAL + 1
    outs = [capi.OutColumn(W, capi.DEVICE) for _ in AGGS]
    oarr = (capi.Out * len(AGGS))()
    carr, aarr = capi._cols([ts, val]), capi._aggs(AGGS)
    opts, info = capi.Options(0, 0, 0), capi.AggInfo()
    L = capi.lib()

    def call():
        for i, o in enumerate(outs):
            oarr[i] = o.c()
        capi.check(L.bowgpu_rolling_aggregate(carr, 2, 0, C.c_int64(INTERVAL), C.byref(opts), aarr, len(AGGS), oarr, C.byref(info)))
    ms = best(call)
    del ts, val, outs
    return ms


def sharded(world, rows_per_rank):
    cols_by_rank, keep = [], []
    for r in range(world):
        ts, val = capi.gen_dense(r * rows_per_rank, rows_per_rank)
        keep.append((ts, val))
        cols_by_rank.append([ts, val])
    capi.synchronize()
    ds = capi.sharded_layout(cols_by_rank, 0, INTERVAL, AGGS, [0] * world)
    outs = [[capi.OutColumn(d.windows_local, capi.DEVICE) for _ in AGGS] for d in ds]
    world_, ncols, carrs, cptrs, ids, aarr = capi._sharded_args(cols_by_rank, [0] * world, AGGS)
    oarrs = [(capi.Out * len(AGGS))() for _ in range(world)]
    optrs = (C.POINTER(capi.Out) * world)(*[C.cast(a, C.POINTER(capi.Out)) for a in oarrs])
    dec = (capi.ShardDecision * world)()
    opts, info = capi.Options(0, 0, 0), capi.AggInfo()
    L = capi.lib()

    def call():
        for r in range(world):
            for i, o in enumerate(outs[r]):
                oarrs[r][i] = o.c()
        capi.check(L.bowgpu_rolling_aggregate_sharded(cptrs, ids, world, ncols, 0, C.c_int64(INTERVAL), C.byref(opts), aarr, len(AGGS),
                                                      optrs, dec, C.byref(info)))
    ms = best(call)
    del keep, outs
    return ms


def main():
    print("commit %s" % os.environ.get("COMMIT", "?"))
    b, m = one_device(N)
    print("one-device %d rows: best %.3f ms, median %.3f ms" % (N, b, m), flush=True)
    if not hasattr(capi.lib(), "bowgpu_rolling_aggregate_sharded"):
        return
    for world in (2, 4, 8):
        sb, sm = sharded(world, N // world)
        print("sharded world=%d x %d rows: best %.3f ms, median %.3f ms, best/one-device best %.3f" % (world, N // world, sb, sm, sb / b), flush=True)
    b8, m8 = one_device(8 * N)
    print("one-device %d rows: best %.3f ms, median %.3f ms" % (8 * N, b8, m8), flush=True)
    sb, sm = sharded(8, N)
    print("sharded world=8 x %d rows: best %.3f ms, median %.3f ms, best/one-device best %.3f" % (N, sb, sm, sb / b8), flush=True)


if __name__ == "__main__":
    main()
