"""Wall time of Rolling.Aggregate over a BOOLEAN value column at 1e8 rows (device-resident, interval 10: 1e7 windows of 10 rows,
30 % nulls, outputs allocated ONCE outside the timed region), next to the same reducers over a Float64 column holding the same
0.0 / 1.0 values and the same validity - the path the data had before the device took Boolean columns:
  (a) Count + ArithmeticMean + Last            (bool_windows_kernel against the Float64 tile kernel)
  (b) WeightedAverageStep                      (the Boolean column widened to Float64 first: the difference is the widening)
One process; run it under a time limit:
    timeout -k 10 600 python scratch/bool_agg_wall.py [rows] [output file] [trace]
Warm-up call, then REPS timed calls: median (min .. max).  With `trace` only run (a) over the Boolean column is made and nothing is
written: the process a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python scratch/bool_agg_wall.py 1e8 - trace)."""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
dst = sys.argv[2] if len(sys.argv) > 2 else "profiles/bool_agg_wall_1e8.txt"
TRACE = len(sys.argv) > 3 and sys.argv[3] == "trace"
REPS = 5
INTERVAL = 10

try:
    commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
except Exception:
    commit = open("scratch/HEAD_COMMIT").read().strip() if os.path.exists("scratch/HEAD_COMMIT") else "(snapshot without .git)"
lines = ["commit %s + the working tree of the commit that adds this file" % commit,
         "scratch/bool_agg_wall.py %d rows on %s; ts[i] = i, interval %d (%d windows), value column 30 %% nulls, device-resident inputs and outputs;"
         % (n, capi.device_name(), INTERVAL, (n + INTERVAL - 1) // INTERVAL),
         "wall = one bowgpu_rolling_aggregate call + synchronise, median of %d after a warm-up (min .. max); kernel = bowgpu_agg_info.kernel_ms, median" % REPS, ""]


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(fn):
    fn(); capi.synchronize()
    wall, kern = [], []
    for _ in range(REPS):
        t0 = time.perf_counter(); info = fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3); kern.append(info.kernel_ms)
    wall.sort(); kern.sort()
    return wall[REPS // 2], wall[0], wall[-1], kern[REPS // 2]


rng = np.random.default_rng(42)
ts, _ = capi.gen_dense(0, n, seed=42)          # ts[i] = i
vals = rng.random(n) < 0.5
valid = rng.random(n) >= 0.3
bm = np.packbits(valid, bitorder="little")
bcol = capi.Column(np.packbits(vals, bitorder="little"), bm, capi.BOOLEAN, 0, n, int(n - valid.sum())).to_device()
fcol = capi.Column(vals.astype(np.float64), bm, capi.FLOAT64, 0, n, int(n - valid.sum())).to_device()
del vals, valid
W = capi.plan_windows(ts, INTERVAL)[1]

runs = [("(a) Count + ArithmeticMean + Last", [("WindowStart", 0), ("Count", 1), ("ArithmeticMean", 1), ("Last", 1)]),
        ("(b) WeightedAverageStep", [("WindowStart", 0), ("WeightedAverageStep", 1)])]
for label, aggs in runs[:1] if TRACE else runs:
    outs = [capi.OutColumn(W, capi.DEVICE) for _ in aggs]
    res = {}
    for name, col in (("Boolean", bcol), ("Float64", fcol))[:1 if TRACE else 2]:
        res[name] = timeit(lambda: capi.rolling_aggregate([ts, col], 0, INTERVAL, aggs, outs=outs)[1])
        kernel = capi.last_kernel_instance()
        say("%s over the %s column: wall median %.3f ms (min %.3f .. max %.3f), kernel median %.3f ms   [%s]"
            % ((label, name) + res[name] + (kernel,)))
    if TRACE:
        sys.exit(0)
    b, f = res["Boolean"], res["Float64"]
    overlap = b[1] <= f[2] and f[1] <= b[2]
    say("    Boolean / Float64 wall medians: %.2f   (%s)" % (b[0] / f[0], "the two runs' min .. max ranges overlap" if overlap else
                                                             "Boolean is FASTER beyond the spread" if b[0] < f[0] else "Boolean is SLOWER beyond the spread"))
    say("")
with open(dst, "w") as f:
    f.write("\n".join(lines) + "\n")
