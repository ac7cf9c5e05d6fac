"""Wall time of bowgpu_parquet_write for a device-resident frame: `rows` rows in HBM, an ascending Int64 timestamp column plus a
Float64 column with 30 % nulls, written to a tmpfs path, once PLAIN / PLAIN and once DELTA_BINARY_PACKED / PLAIN.  Set-up (the
columns, their host twins for the comparators, the ctypes arguments) happens outside the clock.  Comparators, timed in the same run:
  (a) bowgpu_memcpy_d2h of the same two columns and the bitmap plus one write() of those bytes to the same directory: the only way
      out of HBM there was, with no encoding counted at all.  The call is expected not to be slower than this beyond the spread.
  (b) pyarrow.parquet.write_table(compression=None, use_dictionary=False) of the host copies, the device-to-host copies counted.
File bytes per row stand beside the times.  One process; run it under a time limit:
    timeout -k 10 900 python scratch/parquet_write_wall.py [rows [outfile [commit [dir]]]]
It prints what it measures and writes the same lines to outfile (default profiles/parquet_write_wall_<rows>.txt), headed by the
commit (the argument, else git rev-parse HEAD).  Per-kernel times come from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/parquet_write_wall.py 1e8 /dev/null
Warm-up call, then REPS timed calls: wall median with min .. max."""
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
OUTFILE = sys.argv[2] if len(sys.argv) > 2 else "profiles/parquet_write_wall_%s.txt" % ("%.0e" % n).replace("e+0", "e").replace("e+", "e")
DIR = sys.argv[4] if len(sys.argv) > 4 else "/dev/shm"
REPS = 5
L = capi.lib()
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def commit():
    if len(sys.argv) > 3:
        return sys.argv[3]
    p = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True)
    return p.stdout.strip() if p.returncode == 0 else "unknown (no git history next to this tree)"


def timeit(fn, reps=REPS):
    fn(); capi.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    return wall[len(wall) // 2], wall[0], wall[-1]


def show(label, t, extra=""):
    say("  %-66s median %10.3f ms   (min %.3f .. max %.3f)%s" % (label, t[0], t[1], t[2], extra))


say("commit: %s" % commit())
say("device: %s   rows: %d   directory: %s   host cores available: %d" % (capi.device_name(), n, DIR, len(os.sched_getaffinity(0))))

# ---- set-up, outside the clock
ts, val = capi.gen_dense(0, n, seed=42)                      # ts[i] = i: ascending
valid = np.random.default_rng(7).random(n) >= 0.3
bitmap = np.packbits(valid, bitorder="little")
nulls = int(n - valid.sum())
d_bitmap = capi.DeviceBuffer.from_numpy(np.concatenate([bitmap, np.zeros(8, np.uint8)]))
cols = [capi.Column(ts.values, None, capi.INT64, 0, n, 0), capi.Column(val.values, d_bitmap, capi.FLOAT64, 0, n, nulls)]
names = ["time", "value"]
path = os.path.join(DIR, "bowgpu_parquet_write_wall.parquet")
raw_path = os.path.join(DIR, "bowgpu_parquet_write_wall.raw")
h_ts, h_val, h_bm = np.empty(n, np.int64), np.empty(n, np.float64), np.empty(len(bitmap), np.uint8)
results = {}

try:
    for label, enc in (("PLAIN / PLAIN", [capi.PARQUET_PLAIN, capi.PARQUET_PLAIN]), ("DELTA_BINARY_PACKED / PLAIN", [capi.PARQUET_DELTA_BINARY_PACKED, capi.PARQUET_PLAIN])):
        info = [None]

        def call():
            info[0] = capi.write_parquet(path, cols, names, encodings=enc)

        t = timeit(call)
        md = pq.read_metadata(path)
        per_col = [sum(md.row_group(g).column(i).total_compressed_size for g in range(md.num_row_groups)) / n for i in range(2)]
        assert md.num_rows == n and info[0].file_bytes == os.path.getsize(path)
        show("bowgpu_parquet_write %s" % label, t, "   %.3f B/row in the file (time %.3f, value %.3f), %d pages, %d row groups"
             % (info[0].file_bytes / n, per_col[0], per_col[1], info[0].data_pages, info[0].row_groups))
        results[label] = t

    def raw_copy():   # (a)
        for harr, dptr in ((h_ts, ts.values.ptr), (h_val, val.values.ptr), (h_bm, d_bitmap.ptr)):
            capi.check(L.bowgpu_memcpy_d2h(harr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), C.c_int64(harr.nbytes)))
        fd = os.open(raw_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            for harr in (h_ts, h_val, h_bm):
                view, done = memoryview(harr).cast("B"), 0
                while done < len(view):
                    done += os.write(fd, view[done:])
        finally:
            os.close(fd)

    a = timeit(raw_copy)
    show("(a) bowgpu_memcpy_d2h of the columns + one write() of the bytes", a, "   %.3f B/row" % (os.path.getsize(raw_path) / n))

    def arrow():      # (b)
        for harr, dptr in ((h_ts, ts.values.ptr), (h_val, val.values.ptr), (h_bm, d_bitmap.ptr)):
            capi.check(L.bowgpu_memcpy_d2h(harr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), C.c_int64(harr.nbytes)))
        v = pa.Array.from_buffers(pa.float64(), n, [pa.py_buffer(h_bm), pa.py_buffer(h_val)], null_count=nulls)
        pq.write_table(pa.table({"time": pa.array(h_ts), "value": v}), path, compression=None, use_dictionary=False)

    b = timeit(arrow, 3)
    show("(b) the same copies + pyarrow.parquet.write_table, no codec", b, "   %.3f B/row" % (os.path.getsize(path) / n))
    for label, t in results.items():
        say("%s: wall median %.3f ms vs (a) %.3f ms: %s (%.2fx); vs (b) %.3f ms: %.2fx"
            % (label, t[0], a[0], "not slower than the raw copy" if t[0] <= a[2] else "SLOWER than the raw copy", a[0] / t[0], b[0], b[0] / t[0]))
finally:
    for p in (path, raw_path, path + ".tmp"):
        if os.path.exists(p):
            os.remove(p)

if OUTFILE != "/dev/null":
    with open(OUTFILE, "w") as fh:
        fh.write("\n".join(lines) + "\n")
