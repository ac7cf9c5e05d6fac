"""Wall time of bowgpu_parquet_write_codec at 1e8 rows: a frame in HBM (an ascending Int64 timestamp, a Float64 of uniform random
doubles with 30 % nulls, an Int64 0 / 1 flag) written to tmpfs
  (a) with codec 1 (SNAPPY), every column PLAIN
  (b) with codec 1, the timestamp DELTA_BINARY_PACKED
  (c) with codec 0 through the same entry point, every column PLAIN (the path of bowgpu_parquet_write)
  (d) with codec 0, the timestamp DELTA_BINARY_PACKED
  (e) by pyarrow.parquet.write_table(compression='snappy', use_dictionary=False) of host copies, the device-to-host copies counted.
One process; run it under a time limit:
    timeout -k 10 1100 python scratch/parquet_snappy_wall.py [rows] [output file] [trace]
Set-up outside the clock; a warm-up call, then REPS timed calls: median (min .. max).  With `trace` only run (a) is made and nothing
is written: the process a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python scratch/parquet_snappy_wall.py 1e8 - trace)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
dst = sys.argv[2] if len(sys.argv) > 2 else "profiles/parquet_snappy_wall_1e8.txt"
TRACE = len(sys.argv) > 3 and sys.argv[3] == "trace"
REPS = 5
TMP = "/dev/shm/bowgpu_snappy_wall_%d" % os.getpid()
PLAIN, DELTA, SNAPPY = capi.PARQUET_PLAIN, capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_CODEC_SNAPPY
L = capi.lib()

try:
    commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
except Exception:
    commit = open("scratch/HEAD_COMMIT").read().strip() if os.path.exists("scratch/HEAD_COMMIT") else "(snapshot without .git)"
lines = ["commit %s + the working tree of the commit that adds this file" % commit,
         "scratch/parquet_snappy_wall.py %d rows on %s, %d host cores; device-resident frame: ts ascending Int64, v uniform random Float64 with 30 %% nulls,"
         % (n, capi.device_name(), len(os.sched_getaffinity(0))),
         "flag Int64 0 / 1; default page and row-group sizes; files on tmpfs; wall = one call, median of %d after a warm-up (min .. max)" % REPS, ""]


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
bm = np.packbits(valid, bitorder="little")
cols = [capi.Column(ts).to_device(), capi.Column(v, bm, capi.FLOAT64, 0, n, int(n - valid.sum())).to_device(), capi.Column(flag).to_device()]
names = ["ts", "v", "flag"]
del ts, v, flag
os.makedirs(TMP, exist_ok=True)
path = os.path.join(TMP, "frame.parquet")


def writer(codec, enc):
    def run():
        return capi.write_parquet(path, cols, names, encodings=enc, codec=codec)
    return run


def write_codec0_through_new_entry(enc):
    o = capi.ParquetWriteOptions()
    o.statistics = 1
    e = (C.c_int32 * 3)(*enc)
    o.encodings = C.cast(e, C.POINTER(C.c_int32))
    cn = (C.c_char_p * 3)(*[s.encode() for s in names])

    def run():
        info = capi.ParquetWriteInfo()
        capi.check(L.bowgpu_parquet_write_codec(os.fsencode(path), capi._cols(cols), cn, 3, C.byref(o), C.c_int32(0), C.byref(info)))
        return info
    return run


try:
    if TRACE:
        run = writer(SNAPPY, [PLAIN] * 3)
        run(); run()
        sys.exit(0)
    # what each column's chunk brings over the link: one-column files, outside the clock
    say("per column, one-column files (file bytes / row; the file is the pages, their headers and the footer):")
    for i, nm in enumerate(names):
        row = []
        for codec, enc in ((0, PLAIN), (SNAPPY, PLAIN)) + (((0, DELTA), (SNAPPY, DELTA)) if i == 0 else ()):
            info = capi.write_parquet(path, cols[i:i + 1], names[i:i + 1], encodings=[enc], codec=codec)
            row.append("%s %s %.3f B/row" % ("SNAPPY" if codec else "UNCOMPRESSED", "DELTA" if enc == DELTA else "PLAIN", info.file_bytes / n))
        say("  %-5s %s" % (nm, "   ".join(row)))
    say("")
    results = {}
    for label, fn in (("(a) codec 1 SNAPPY, PLAIN", writer(SNAPPY, [PLAIN] * 3)),
                      ("(b) codec 1 SNAPPY, ts DELTA", writer(SNAPPY, [DELTA, PLAIN, PLAIN])),
                      ("(c) codec 0 (new entry point), PLAIN", write_codec0_through_new_entry([PLAIN] * 3)),
                      ("(d) codec 0 (new entry point), ts DELTA", write_codec0_through_new_entry([DELTA, PLAIN, PLAIN]))):
        t = timeit(fn)
        size = os.path.getsize(path)
        results[label] = t
        say("%-42s wall %9.1f ms (%9.1f .. %9.1f)   file %7.3f GB = %6.2f B/row   %5.2f GB/s of the frame's %.1f GB"
            % (label, t[0], t[1], t[2], size / 1e9, size / n, 24 * n / (t[0] * 1e-3) / 1e9, 24 * n / 1e9))
    host = [np.empty(n, np.int64), np.empty(n, np.float64), np.empty(n, np.int64)]
    mask = ~np.unpackbits(bm, bitorder="little")[:n].astype(bool)

    def arrow():
        for c, h in zip(cols, host):
            capi.check(L.bowgpu_memcpy_d2h(h.ctypes.data_as(C.c_void_p), C.c_void_p(c.values.ptr), C.c_int64(n * 8)))
        tab = pa.table({"ts": pa.array(host[0]), "v": pa.array(host[1], mask=mask), "flag": pa.array(host[2])})
        pq.write_table(tab, path, compression="snappy", use_dictionary=False)

    t = timeit(arrow, 3)
    size = os.path.getsize(path)
    say("%-42s wall %9.1f ms (%9.1f .. %9.1f)   file %7.3f GB = %6.2f B/row   (median of 3)" % ("(e) d2h copies + pyarrow write_table snappy", t[0], t[1], t[2], size / 1e9, size / n))
    a, c = results["(a) codec 1 SNAPPY, PLAIN"], results["(c) codec 0 (new entry point), PLAIN"]
    say("")
    say("(a) against (c): %.2fx the wall time (medians); spreads %s" % (a[0] / c[0], "overlap" if a[1] <= c[2] and c[1] <= a[2] else "do not overlap"))
    if dst != "-":
        with open(dst, "w") as fh:
            fh.write("\n".join(lines) + "\n")
finally:
    if os.path.exists(path):
        os.remove(path)
    os.rmdir(TMP)
