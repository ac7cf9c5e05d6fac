"""Wall time of bowgpu_parquet_write_codec with RLE_DICTIONARY at 1e8 rows: the frame of scratch/parquet_snappy_wall.py in HBM (an
ascending Int64 timestamp, a Float64 with 30 % nulls, an Int64 0 / 1 flag) written to tmpfs, the timestamp DELTA_BINARY_PACKED
throughout, and ONE column varied over the four ways it can be written:
  flag   the 0 / 1 flag:                                PLAIN, PLAIN + SNAPPY, dictionary, dictionary + SNAPPY   (v stays PLAIN)
  q      v rounded to 1000 distinct values (30 % nulls): PLAIN, PLAIN + SNAPPY, dictionary, dictionary + SNAPPY   (in v's place; flag PLAIN)
PLAIN and PLAIN + SNAPPY are what the parent commit writes: the comparators, taken in the same run.  One process; run it under a
time limit:
    timeout -k 10 1100 python scratch/parquet_dict_wall.py [rows] [output file]
Set-up outside the clock; a warm-up call, then REPS timed calls: median (min .. max).  value_bytes / row of the varied column comes
from a one-column file written outside the clock."""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
dst = sys.argv[2] if len(sys.argv) > 2 else "profiles/parquet_dict_wall_1e8.txt"
REPS = 5
TMP = "/dev/shm/bowgpu_dict_wall_%d" % os.getpid()
PLAIN, DELTA, DICT, SNAPPY = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_RLE_DICTIONARY, capi.PARQUET_CODEC_SNAPPY

try:
    commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
except Exception:
    commit = open("scratch/HEAD_COMMIT").read().strip() if os.path.exists("scratch/HEAD_COMMIT") else "(snapshot without .git)"
lines = ["commit %s + the working tree of the commit that adds this file" % commit,
         "scratch/parquet_dict_wall.py %d rows on %s, %d host cores; device-resident frame: ts ascending Int64 (DELTA_BINARY_PACKED throughout),"
         % (n, capi.device_name(), len(os.sched_getaffinity(0))),
         "v uniform random Float64 with 30 % nulls | q = v rounded to 1000 distinct values, flag Int64 0 / 1; default page and row-group sizes; files on tmpfs;",
         "wall = one call for the three-column frame, median of %d after a warm-up (min .. max); value B/row = info.value_bytes / rows of the varied column alone" % REPS, ""]


def say(s):
    print(s, flush=True)
    lines.append(s)


def timeit(fn, reps=REPS):
    fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    return wall[len(wall) // 2], wall[0], wall[-1]


rng = np.random.default_rng(42)
ts = (1_600_000_000_000 + np.cumsum(rng.integers(1, 2000, n))).astype(np.int64)
v = rng.random(n)
valid = rng.random(n) >= 0.3
flag = rng.integers(0, 2, n).astype(np.int64)
q = np.floor(v * 1000) / 1000
bm = np.packbits(valid, bitorder="little")
nulls = int(n - valid.sum())
c_ts, c_flag = capi.Column(ts).to_device(), capi.Column(flag).to_device()
c_v, c_q = capi.Column(v, bm, capi.FLOAT64, 0, n, nulls).to_device(), capi.Column(q, bm, capi.FLOAT64, 0, n, nulls).to_device()
del ts, v, flag, q
os.makedirs(TMP, exist_ok=True)
path = os.path.join(TMP, "frame.parquet")

try:
    for what, cols, names, at in (("flag", [c_ts, c_v, c_flag], ["ts", "v", "flag"], 2), ("q", [c_ts, c_q, c_flag], ["ts", "q", "flag"], 1)):
        say("%s varied; frame %s" % (what, " / ".join(names)))
        res = {}
        for label, enc, codec in (("PLAIN", PLAIN, 0), ("PLAIN + SNAPPY", PLAIN, SNAPPY), ("dictionary", DICT, 0), ("dictionary + SNAPPY", DICT, SNAPPY)):
            one = capi.write_parquet(path, cols[at:at + 1], names[at:at + 1], encodings=[enc], codec=codec)
            one_file = os.path.getsize(path)
            encs = [DELTA, PLAIN, PLAIN]
            encs[at] = enc
            t = timeit(lambda: capi.write_parquet(path, cols, names, encodings=encs, codec=codec))
            size = os.path.getsize(path)
            res[label] = t
            say("  %-20s wall %8.1f ms (%8.1f .. %8.1f)   file %6.3f GB = %5.2f B/row   %s alone: value %6.4f B/row, file %6.4f B/row"
                % (label, t[0], t[1], t[2], size / 1e9, size / n, what, one.value_bytes / n, one_file / n))
        for a, b in (("dictionary", "PLAIN"), ("dictionary + SNAPPY", "PLAIN + SNAPPY")):
            x, y = res[a], res[b]
            say("  %s against %s: %.2fx the wall time (medians); spreads %s" % (a, b, x[0] / y[0], "overlap" if x[1] <= y[2] and y[1] <= x[2] else "do not overlap"))
        say("")
    if dst != "-":
        with open(dst, "w") as fh:
            fh.write("\n".join(lines) + "\n")
finally:
    if os.path.exists(path):
        os.remove(path)
    os.rmdir(TMP)
