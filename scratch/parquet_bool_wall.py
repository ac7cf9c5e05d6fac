"""Wall time of the Parquet loader's BOOLEAN path (bowgpu_parquet_read_bool_column) at 1e8 rows, 30 % nulls, random flags: the
column written by pyarrow PLAIN and RLE, each with codec none and SNAPPY, file on tmpfs, output DEVICE (built ONCE outside the timed
region, like the ctypes arguments).  The comparator, in the same run and alternating with those reads, is the same flags stored as an
Int64 PLAIN column (codec none) through bowgpu_parquet_read_column.  What bytes moved lead one to expect: the Boolean file crosses
the host link at about 1/4 B per row (value bits + level bits), the Int64 file at 8 B per row, so the Boolean read is expected to be
NOT SLOWER than the Int64 read.  One process; run it under a time limit:
    timeout -k 10 900 python scratch/parquet_bool_wall.py [rows]
Warm-up read of every file, then REPS rounds over all files: wall median with the spread (min .. max)."""
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
REPS = 5
L = capi.lib()
print("device: %s   rows: %d   nulls: 30 %%   reps: %d   pyarrow %s" % (capi.device_name(), n, REPS, pa.__version__))

rng = np.random.default_rng(7)
flags = rng.random(n) < 0.5
nulls = rng.random(n) < 0.3
null_count = int(nulls.sum())
tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
files = []   # (label, path, entry point, column type, encoding bit the check must report)
try:
    barr = pa.array(flags, mask=nulls)
    for enc, kw, bit in (("PLAIN", {}, capi.PARQUET_ENC_PLAIN), ("RLE", {"column_encoding": {"flag": "RLE"}}, capi.PARQUET_ENC_RLE)):
        for codec in ("none", "snappy"):
            path = os.path.join(tmp, "bool_%s_%s.parquet" % (enc, codec))
            pq.write_table(pa.table({"flag": barr}), path, use_dictionary=False, compression=codec, **kw)
            files.append(("BOOLEAN %-5s %-6s" % (enc, codec), path, L.bowgpu_parquet_read_bool_column, capi.BOOLEAN, bit))
    del barr
    path = os.path.join(tmp, "int64_PLAIN_none.parquet")
    pq.write_table(pa.table({"flag": pa.array(flags.astype(np.int64), mask=nulls)}), path, use_dictionary=False, compression="none")
    files.append(("INT64   PLAIN none  ", path, L.bowgpu_parquet_read_column, capi.INT64, capi.PARQUET_ENC_PLAIN))
    del flags, nulls

    out = capi.OutColumn(n, capi.DEVICE)   # 8 n bytes of values: holds the Boolean output's n / 8 too
    handles, walls = [], [[] for _ in files]
    for label, path, fn, typ, bit in files:
        f = capi.ParquetFile(path)
        groups = pq.ParquetFile(path).metadata.num_row_groups
        got = f.check_bool_column(0) if typ == capi.BOOLEAN else f.check_column(0)
        assert got == bit, (label, got)
        handles.append(f)
        print("%s  %12d bytes   %d row groups" % (label, os.path.getsize(path), groups))

    def read(k):
        o = out.c()
        capi.check(files[k][2](handles[k].h, 0, C.byref(o)))
        capi.synchronize()
        assert (o.length, o.type, o.null_count) == (n, files[k][3], null_count), (files[k][0], o.length, o.type, o.null_count)

    for k in range(len(files)):   # warm-up: code objects, pools, the page cache
        read(k)
    for _ in range(REPS):         # the reads alternate: every round reads every file once
        for k in range(len(files)):
            t0 = time.perf_counter()
            read(k)
            walls[k].append((time.perf_counter() - t0) * 1e3)
    med = [sorted(w)[REPS // 2] for w in walls]
    ref = med[-1]
    print("\n%-22s %10s %24s %14s   %s" % ("file", "wall med", "(min .. max) ms", "rows/s", "expectation: not slower than the Int64 read"))
    missed = []
    for k, (label, path, fn, typ, bit) in enumerate(files):
        w = sorted(walls[k])
        verdict = "(the comparator)" if k == len(files) - 1 else "%.2f x the Int64 read: %s" % (med[k] / ref, "MET" if med[k] <= ref else "MISSED")
        if k < len(files) - 1 and med[k] > ref:
            missed.append(label.strip())
        print("%-22s %10.3f %24s %14.3e   %s" % (label, med[k], "(%.3f .. %.3f)" % (w[0], w[-1]), n / (med[k] * 1e-3), verdict))
    print("\nexpectations MISSED: %s" % (", ".join(missed) + " (kernel to look at: bool_pages_kernel, bow_amd/csrc/parquet_decode.hip)" if missed else "none"))
    for f in handles:
        f.close()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
