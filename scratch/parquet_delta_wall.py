"""Wall time of bowgpu_parquet_read_column on DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT columns, every comparator in the same run:
  columns   ts: ascending int64 timestamps (steps 1..19), REQUIRED          -> DELTA_BINARY_PACKED
            i:  int64 within +-1e9 with 30 % nulls                           -> DELTA_BINARY_PACKED
            d:  standard-normal doubles with 30 % nulls                      -> BYTE_STREAM_SPLIT
  files     "new":   the encodings above, written UNCOMPRESSED and with SNAPPY
            "plain": the same data PLAIN + SNAPPY without a dictionary - what the loader read before these encodings
            each at two page sizes: 8 KB (the reference's writer) and pyarrow's default of 1 MiB
  per column  bytes of its chunks in the file, data pages, wall time into a DEVICE output (warm-up call, then REPS timed calls that
              end in a device synchronise: median with min .. max), and pyarrow.parquet.read_table(columns=[name]) of the same file
One process; run it under a time limit:
    timeout -k 10 900 python scratch/parquet_delta_wall.py [rows [only [outfile [commit]]]]     # only: a column name, or all
It prints what it measures and writes the same lines to outfile (default profiles/parquet_delta_wall.txt), headed by the commit (the
argument, else git rev-parse HEAD).  The dominant kernel comes from a profiler run of one column in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/parquet_delta_wall.py 2e7 ts /dev/null"""
import mmap
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, '.')
from bow_amd import capi

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20_000_000
ONLY = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "all" else None
OUTFILE = sys.argv[3] if len(sys.argv) > 3 else "profiles/parquet_delta_wall.txt"
REPS = 5
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def commit():
    if len(sys.argv) > 4:
        return sys.argv[4]
    p = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True)
    return p.stdout.strip() if p.returncode == 0 else "unknown (no git history next to this tree)"


def timeit(fn, reps=REPS):
    fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    return wall[len(wall) // 2], wall[0], wall[-1]


# ---- counting a chunk's data pages: a Thrift compact reader that keeps PageHeader.type and .compressed_page_size and skips the rest
def _varint(b, p):
    r = sh = 0
    while True:
        c = b[p]
        p += 1
        r |= (c & 0x7f) << sh
        sh += 7
        if not c & 0x80:
            return r, p


def _skip(b, p, t):
    if t in (1, 2):
        return p
    if t == 3:
        return p + 1
    if t in (4, 5, 6):
        return _varint(b, p)[1]
    if t == 7:
        return p + 8
    if t == 8:
        ln, p = _varint(b, p)
        return p + ln
    if t in (9, 10):
        h = b[p]
        p += 1
        cnt = h >> 4
        if cnt == 15:
            cnt, p = _varint(b, p)
        for _ in range(cnt):
            p = p + 1 if (h & 15) <= 2 else _skip(b, p, h & 15)
        return p
    if t == 12:
        return _struct(b, p, None)
    raise ValueError("thrift type %d" % t)


def _struct(b, p, keep):
    fid = 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return p
        if h >> 4:
            fid += h >> 4
        else:
            z, p = _varint(b, p)
            fid = (z >> 1) ^ -(z & 1)
        if keep is not None and (h & 15) == 5 and fid in (1, 3):
            z, p = _varint(b, p)
            keep[fid] = (z >> 1) ^ -(z & 1)
        else:
            p = _skip(b, p, h & 15)


def chunk_stats(path, col):
    """(bytes of the column's chunks, data pages in them)"""
    md = pq.ParquetFile(path).metadata
    with open(path, "rb") as fh:
        blob = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)   # (indexing gives Python ints)
    nbytes = pages = 0
    for g in range(md.num_row_groups):
        cm = md.row_group(g).column(col)
        start = cm.dictionary_page_offset if cm.dictionary_page_offset else cm.data_page_offset
        nbytes += cm.total_compressed_size
        p, end = start, start + cm.total_compressed_size
        while p < end:
            keep = {}
            p = _struct(blob, p, keep)
            pages += keep.get(1) in (0, 3)
            p += keep[3]
    return nbytes, pages


rng = np.random.default_rng(1)
cols = {"ts": pa.array(np.cumsum(rng.integers(1, 20, n)).astype(np.int64)),
        "i": pa.array(rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64), mask=rng.random(n) < 0.3),
        "d": pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.3)}
table = pa.table(cols, schema=pa.schema([pa.field("ts", pa.int64(), nullable=False), pa.field("i", pa.int64()), pa.field("d", pa.float64())]))
NEW = {"ts": "DELTA_BINARY_PACKED", "i": "DELTA_BINARY_PACKED", "d": "BYTE_STREAM_SPLIT"}
VARIANTS = [("plain + snappy", dict(compression="snappy")),
            ("new, uncompressed", dict(compression="none", column_encoding=NEW)),
            ("new + snappy", dict(compression="snappy", column_encoding=NEW))]

say("commit %s" % commit())
say("scratch/parquet_delta_wall.py %d rows on %s; new = ts, i: DELTA_BINARY_PACKED, d: BYTE_STREAM_SPLIT; wall = read_column into a DEVICE output," % (n, capi.device_name()))
say("file in the page cache, median of %d after a warm-up (min .. max); pyarrow = read_table(columns=[name]) of the same file, same way" % REPS)
d = tempfile.mkdtemp()
results = {}
for page in (8192, 1 << 20):
    say()
    say("data_page_size %d B" % page)
    say("  %-18s %-4s %13s %8s   %-42s %s" % ("file", "col", "chunk bytes", "pages", "read_column -> device, ms", "pyarrow read_table, ms"))
    for tag, kw in VARIANTS:
        path = os.path.join(d, "f_%d_%s.parquet" % (page, tag.replace(" ", "").replace(",", "_").replace("+", "_")))
        pq.write_table(table, path, use_dictionary=False, data_page_size=page, data_page_version="2.0" if "new" in tag else "1.0", **kw)
        f = capi.ParquetFile(path)
        for ci, name in enumerate(table.schema.names):
            if ONLY and name != ONLY:
                continue
            nbytes, pages = chunk_stats(path, ci)

            def read():
                out = f.read_column(ci, out_residency=capi.DEVICE)
                capi.synchronize()
                return out
            t = timeit(read)
            ta = timeit(lambda: pq.read_table(path, columns=[name]), reps=3) if not ONLY else (float("nan"),) * 3
            results[(page, tag, name)] = t[0]
            say("  %-18s %-4s %13d %8d   %9.3f  (%8.3f .. %8.3f)             %9.3f  (%8.3f .. %8.3f)" % ((tag, name, nbytes, pages) + t + ta))
        f.close()
        os.remove(path)
say()
for page in (8192, 1 << 20):
    for name in table.schema.names:
        if (page, "plain + snappy", name) in results:
            p = results[(page, "plain + snappy", name)]
            say("page %7d B, %-2s: new uncompressed / plain + snappy = %.2f, new + snappy / plain + snappy = %.2f  (wall medians; below 1: the new encoding loads faster)"
                % (page, name, results[(page, "new, uncompressed", name)] / p, results[(page, "new + snappy", name)] / p))
if OUTFILE != "/dev/null":
    with open(OUTFILE, "w") as fh:
        fh.write("\n".join(lines) + "\n")
