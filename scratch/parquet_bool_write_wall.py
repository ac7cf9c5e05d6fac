"""Wall time of bowgpu_parquet_write_bool at 1e8 rows: one flag column in HBM (random flags, 30 % nulls) written to tmpfs three ways,
each under both codecs:
  boolean      the bit-packed Boolean column through bowgpu_parquet_write_bool: a Parquet BOOLEAN column
  dictionary   the same flags as an Int64 0 / 1 column with encodings = 8 (bowgpu_parquet_write_codec): the route that stood before,
               and the comparator of the expectation "the Boolean column is not slower than the Int64 dictionary route"
  plain        the same Int64 column PLAIN
One process; run it under a time limit:
    timeout -k 10 900 python scratch/parquet_bool_write_wall.py [rows] [output file]
Set-up outside the clock, the removal of the previous variant's file included; a warm-up round, then REPS timed rounds, the six
variants alternating inside every round: median (min .. max) per variant."""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
dst = sys.argv[2] if len(sys.argv) > 2 else "profiles/parquet_bool_write_wall_1e8.txt"
REPS = 5
TMP = "/dev/shm/bowgpu_bool_write_wall_%d" % os.getpid()
PLAIN, DICT, SNAPPY = capi.PARQUET_PLAIN, capi.PARQUET_RLE_DICTIONARY, capi.PARQUET_CODEC_SNAPPY

try:
    commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
except Exception:
    commit = open("scratch/HEAD_COMMIT").read().strip() if os.path.exists("scratch/HEAD_COMMIT") else "(snapshot without .git)"
lines = ["commit %s + the working tree of the commit that adds this file" % commit,
         "scratch/parquet_bool_write_wall.py %d rows on %s, %d host cores; one device-resident flag column, random flags, 30 %% nulls;"
         % (n, capi.device_name(), len(os.sched_getaffinity(0))),
         "default page and row-group sizes, statistics on; files on tmpfs; wall = one call, median of %d rounds after a warm-up round (min .. max)," % REPS,
         "the six variants alternating inside every round", ""]


def say(s):
    print(s, flush=True)
    lines.append(s)


rng = np.random.default_rng(42)
flags = rng.random(n) < 0.5
valid = rng.random(n) >= 0.3
bm = np.packbits(valid, bitorder="little")
nulls = int(n - valid.sum())
c_bool = capi.Column(np.packbits(flags, bitorder="little"), bm, capi.BOOLEAN, 0, n, nulls).to_device()
c_int = capi.Column(flags.astype(np.int64), bm, capi.INT64, 0, n, nulls).to_device()
del flags, valid
os.makedirs(TMP, exist_ok=True)
path = os.path.join(TMP, "flag.parquet")

VARIANTS = [("boolean", c_bool, PLAIN, 0, True), ("boolean + SNAPPY", c_bool, PLAIN, SNAPPY, True),
            ("dictionary", c_int, DICT, 0, False), ("dictionary + SNAPPY", c_int, DICT, SNAPPY, False),
            ("plain", c_int, PLAIN, 0, False), ("plain + SNAPPY", c_int, PLAIN, SNAPPY, False)]

try:
    wall = {v[0]: [] for v in VARIANTS}
    size, value = {}, {}
    for rnd in range(REPS + 1):
        for label, col, enc, codec, booleans in VARIANTS:
            if os.path.exists(path):   # outside the clock: else the rename inside the call frees the previous variant's file, up to 0.57 GB of tmpfs
                os.remove(path)
            t0 = time.perf_counter()
            info = capi.write_parquet(path, [col], ["flag"], encodings=[enc], codec=codec, booleans=booleans)
            t = (time.perf_counter() - t0) * 1e3
            if rnd:
                wall[label].append(t)
            size[label], value[label] = os.path.getsize(path), info.value_bytes
    res = {}
    for label, *_ in VARIANTS:
        w = sorted(wall[label])
        res[label] = (w[len(w) // 2], w[0], w[-1])
        say("  %-20s wall %8.1f ms (%8.1f .. %8.1f)   file %7.4f GB = %6.3f B/row   value %6.4f B/row"
            % (label, res[label][0], w[0], w[-1], size[label] / 1e9, size[label] / n, value[label] / n))
    say("")
    for a, b in (("boolean", "dictionary"), ("boolean + SNAPPY", "dictionary + SNAPPY"), ("boolean", "plain"), ("boolean + SNAPPY", "plain + SNAPPY")):
        x, y = res[a], res[b]
        verdict = ""
        if b.startswith("dictionary"):
            verdict = "   expectation 'not slower than the Int64 dictionary route': %s" % ("MET" if x[0] <= y[0] else "MISSED")
        say("  %s against %s: %.2fx the wall time (medians); spreads %s%s"
            % (a, b, x[0] / y[0], "overlap" if x[1] <= y[2] and y[1] <= x[2] else "do not overlap", verdict))
    if dst != "-":
        with open(dst, "w") as fh:
            fh.write("\n".join(lines) + "\n")
finally:
    if os.path.exists(path):
        os.remove(path)
    os.rmdir(TMP)
