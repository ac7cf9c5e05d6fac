"""Wall time of SMALL Rolling.Aggregate calls, where the host side of a call - staging the caller's buffers, preparing and handing
back the outputs (bow_amd/csrc/dev_cols.cpp) - dominates:
  host     1e5 rows, pageable columns and outputs (BOWGPU_HOST), one Float64 column with a bitmap, WindowStart + ArithmeticMean
  device   the same call with device-resident columns and outputs
  boolean  (a) of scratch/bool_agg_wall.py at 1e5 rows: Count + ArithmeticMean + Last over a device-resident Boolean column
One process measures one library (BOWGPU_LIB=<path> picks another build); comparing two builds is a matter of running it for
each, alternating, in one session on one machine:
    timeout -k 10 300 python scratch/staging_wall.py <label> <output file>
Per case: WARM calls, then REPS timed calls, each followed by a synchronise; median, minimum, 10th and 90th percentile in microseconds."""
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

label = sys.argv[1] if len(sys.argv) > 1 else "this build"
dst = sys.argv[2] if len(sys.argv) > 2 else None
N, INTERVAL, WARM, REPS = 100_000, 10, 50, 1000

rng = np.random.default_rng(42)
ts = np.arange(N, dtype=np.int64)
valid = rng.random(N) >= 0.3
bm = np.packbits(valid, bitorder="little")
nulls = int(N - valid.sum())
h_cols = [capi.Column(ts, None, capi.INT64), capi.Column(rng.standard_normal(N), bm, capi.FLOAT64, 0, N, nulls)]
d_cols = [c.to_device() for c in h_cols]
b_cols = [d_cols[0], capi.Column(np.packbits(rng.random(N) < 0.5, bitorder="little"), bm, capi.BOOLEAN, 0, N, nulls).to_device()]
W = capi.plan_windows(h_cols[0], INTERVAL)[1]
MEAN = [("WindowStart", 0), ("ArithmeticMean", 1)]
BOOL = [("WindowStart", 0), ("Count", 1), ("ArithmeticMean", 1), ("Last", 1)]
cases = [("host", h_cols, MEAN, capi.HOST), ("device", d_cols, MEAN, capi.DEVICE), ("boolean", b_cols, BOOL, capi.DEVICE)]

lines = ["scratch/staging_wall.py [%s] on %s: %d rows, interval %d (%d windows), 30 %% nulls; wall of one bowgpu_rolling_aggregate call + synchronise,"
         % (label, capi.device_name(), N, INTERVAL, W), "%d calls after %d warm-up calls, microseconds" % (REPS, WARM)]
for name, cols, aggs, residency in cases:
    outs = [capi.OutColumn(W, residency) for _ in aggs]       # allocated once, outside the timed region

    def call():
        capi.rolling_aggregate(cols, 0, INTERVAL, aggs, outs=outs)
        capi.synchronize()

    for _ in range(WARM):
        call()
    t = np.empty(REPS)
    for i in range(REPS):
        t0 = time.perf_counter()
        call()
        t[i] = (time.perf_counter() - t0) * 1e6
    lines.append("%-8s median %8.1f  min %8.1f  p10 %8.1f  p90 %8.1f" % (name, np.median(t), t.min(), np.percentile(t, 10), np.percentile(t, 90)))
print("\n".join(lines), flush=True)
if dst:
    with open(dst, "w") as f:
        f.write("\n".join(lines) + "\n")
