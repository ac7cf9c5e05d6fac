"""The device's Snappy stream next to libsnappy's for six page contents at 65 536 rows in one PLAIN page without nulls: the bytes of
the page's values elements as tests/parquet_snappy_walk.py finds them in the file bowgpu_parquet_write_codec wrote, and
len(pyarrow.Codec('snappy').compress(...)) of the same 524 288 page bytes.  One process; run it under a time limit:
    timeout -k 10 120 python scratch/parquet_snappy_sizes.py [output file]"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import parquet_snappy_walk as swalk
from bow_amd import capi

dst = sys.argv[1] if len(sys.argv) > 1 else "profiles/parquet_snappy_sizes.txt"
N = 65536
try:
    commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
except Exception:
    commit = open("scratch/HEAD_COMMIT").read().strip() if os.path.exists("scratch/HEAD_COMMIT") else "(snapshot without .git)"
lines = ["commit %s + the working tree of the commit that adds this file" % commit,
         "scratch/parquet_snappy_sizes.py on %s: one PLAIN page of %d rows without nulls (%d bytes), codec SNAPPY;" % (capi.device_name(), N, 8 * N),
         "device = bytes of the page's values elements in the written file; libsnappy = pyarrow.Codec('snappy').compress of the page's bytes", "",
         "%-42s %10s %8s %10s %8s %8s %8s %9s" % ("page contents", "device B", "/ page", "libsnappy", "/ page", "dev/lib", "copies", "literals")]
rng = np.random.default_rng(42)
shapes = [("Int64 0 / 1 flags", rng.integers(0, 2, N).astype(np.int64)),
          ("small integers (0 .. 99)", rng.integers(0, 100, N).astype(np.int64)),
          ("a constant", np.full(N, 1013.25)),
          ("PLAIN ascending timestamps", (1_600_000_000_000 + np.cumsum(rng.integers(1, 2000, N))).astype(np.int64)),
          ("a measurement rounded to two decimals", np.round(20.0 + np.cumsum(0.1 * rng.standard_normal(N)), 2)),
          ("uniform random doubles", rng.random(N))]
codec = pa.Codec("snappy")
with tempfile.TemporaryDirectory() as d:
    for name, v in shapes:
        path = os.path.join(d, "p.parquet")
        capi.write_parquet(path, [capi.Column(v).to_device()], ["c"], page_rows=N, row_group_rows=N, codec=capi.PARQUET_CODEC_SNAPPY)
        (pg,) = list(swalk.pages(path, pq.read_metadata(path).row_group(0).column(0)))
        assert pg[3] == v.tobytes()
        els = swalk.values_elements(pg[5], len(pg[2]))
        dev = sum(e[4] + (e[1] if e[0] == swalk.LITERAL else 0) for e in els)
        lib = len(codec.compress(pg[3]))
        s = "%-42s %10d %8.3f %10d %8.3f %8.2f %8d %9d" % (name, dev, dev / (8 * N), lib, lib / (8 * N), dev / lib, sum(e[0] == swalk.COPY for e in els),
                                                         sum(e[0] == swalk.LITERAL for e in els))
        print(s, flush=True)
        lines.append(s)
with open(dst, "w") as fh:
    fh.write("\n".join(lines) + "\n")
