"""bench.py as its own launcher: `python bench.py --gpus N` with no WORLD_SIZE in the environment must start N rank
processes itself (before anything touches the GPU in the parent), forward only rank 0's stdout, and fail when a rank dies."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run_launcher(tmp_path, body, n=3, timeout=60):
    stub = tmp_path / "stub.py"
    stub.write_text(textwrap.dedent(body))
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "raise SystemExit(bench.launch_ranks(%d, ['--x', '1'], script=%r, timeout=%d))" % (ROOT, n, str(stub), timeout))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout + 30)


def test_launcher_forwards_rank0_only_and_sets_env(tmp_path):
    r = _run_launcher(tmp_path, """
        import json, os, sys
        print(json.dumps({k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
                         | {"argv": sys.argv[1:]}))
    """)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout           # rank 0's line is the only stdout line
    rec = json.loads(lines[0])
    assert rec["RANK"] == "0" and rec["LOCAL_RANK"] == "0" and rec["WORLD_SIZE"] == "3"
    assert rec["MASTER_ADDR"] == "127.0.0.1" and int(rec["MASTER_PORT"]) > 0
    assert rec["argv"] == ["--x", "1"]
    others = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{")]
    assert sorted(o["RANK"] for o in others) == ["1", "2"]
    assert {o["MASTER_PORT"] for o in others} == {rec["MASTER_PORT"]}


def test_launcher_dead_rank_fails_the_run(tmp_path):
    r = _run_launcher(tmp_path, """
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(7)
        time.sleep(30)      # the surviving ranks are stopped by the launcher, long before this ends
        print("{}")
    """, timeout=25)
    assert r.returncode == 7, (r.returncode, r.stderr)
    assert r.stdout.strip() == ""
    assert "rank 1 exited with code 7" in r.stderr


def test_bench_without_gpu_fails_loudly_for_n2():
    """No GPU in this container: both ranks must refuse (no CPU fallback), and the launcher must report it."""
    from bow_amd import capi
    try:
        n = capi.device_count()   # (not torch in this process: once libbowgpu is loaded, torch's own HIP runtime copy sees no device)
    except capi.BowGpuError:
        n = 0
    if n > 0:
        pytest.skip("GPU box: covered by test_bench_two_ranks_on_one_gpu")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "1e5", "--steps", "1",
                        "--warmup", "0", "--no-cpu"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert r.stdout.strip() == ""
    assert "needs a GPU" in r.stderr


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu():
    """The driver's `python bench.py --gpus 2` form on a 1-GPU box: both ranks on GPU 0, exchange over gloo."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(BOW_BENCH_SINGLE_DEVICE="1", BOW_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "1e7", "--steps", "3",
                        "--warmup", "1", "--no-cpu", "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    assert rec["config"]["parallelism"] == "rows range-partitioned x2"
    assert rec["value"] > 0 and rec["exchange_ms"] > 0 and rec["exchange_hidden_ms"] >= 0
    assert rec["exchange"]["exchanges_per_step"] == 1 and rec["exchange"]["record_bytes"] > 2000
    assert rec["parity_check"]["ok"] is True and rec["parity_check"]["checked_against_oracle"] > 100_000


@pytest.mark.gpu
def test_bench_line_contract_single_gpu():
    """`python bench.py --full` at N = 1 (a reduced row count, everything else as the default run): ONE JSON line on stdout with the keys of
    the bench contract - the metric of BASELINE.json, the roofline object (live kernel time on the library's stream, the in-run
    ceilings) and the cpu_baseline object - and values that hang together."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "2e7", "--steps", "4", "--warmup", "1",
                        "--cpu-sample", "2e6", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert rec["metric"] == "rows/sec rolling-mean on 1B-row float64" and rec["metric"] in base["metric"]
    assert rec["unit"] == "rows/s" and rec["n_gpus"] == 1 and rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["higher_is_better"] is True and rec["scaling"] == "weak" and rec["vs_baseline"] is None
    assert rec["dtype"] == "f64" and rec["data"] == "synthetic" and "workload" in rec["config"] and "model" not in rec["config"]
    assert abs(rec["value"] - 2e7 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-6
    roof = rec["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    assert abs(roof["achieved"] - 2e7 * 16 / (roof["kernel_ms"] * 1e-3) / 1e9) / roof["achieved"] < 1e-6
    assert roof["kernel"] == "rolling_simple_kernel" and 0 < roof["kernel_ms"] <= rec["ms_per_step"]
    assert roof["traffic"] is None          # (PMC traffic is committed for the 1e9-row launch only)
    assert roof["stream_read_ceiling"]["value"] > 0 and roof["stream_rw_probe"]["value"] > 0
    cpu = rec["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] == 1 and cpu["unit"] == "rows/s" and cpu["value"] > 0 and cpu["sample"]
    assert rec["host_pinned"]["value"] > 0 and rec["host_pinned"]["pageable_rows_per_s"] > 0
    par = rec["parity_check"]
    assert par["ok"] is True and par["progression_checked"] == 2_000_000 and par["checked_against_oracle"] >= 2_000_000 // 10 * 2 - 2


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_the_timed_outputs(tmp_path):
    """`python bench.py` without --full: the headline keys and none of what --full adds.  --dump-outputs DIR writes what the last timed
    step computed: a fixed sample of windows as float32 / float64 .npy files, at most 64 MB, equal to the oracle's outputs bit for bit
    and the same in a second run with the same arguments."""
    import numpy as np
    import bench
    from oracle import pyoracle as orc
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    rows, windows = 20_000_000, 2_000_000

    def run(d):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "2e7", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    rec, got = run(tmp_path / "a")
    assert rec["metric"] == "rows/sec rolling-mean on 1B-row float64" and rec["unit"] == "rows/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f64" and rec["steps"] == 3 and rec["warmup"] == 1
    assert abs(rec["value"] - rows / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-6
    assert rec["parity_check"] is None
    assert not {"cpu_baseline", "cpu_baseline_all_cores", "host_pinned", "host_pinned_multi"} & set(rec)
    assert not {"stream_read_ceiling", "stream_rw_probe"} & set(rec["roofline"])
    assert sorted(got) == ["mean", "mean_valid", "window_index", "window_start", "window_start_valid"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in got) <= 64 * 2 ** 20
    idx = got["window_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and idx[0] >= 0 and idx[-1] < windows and (np.diff(idx) > 0).all()
    ts, val = orc.gen_dense(0, rows, seed=42)
    want, _ = orc.aggregate([orc.Column(ts, None, orc.INT64), orc.Column(val, None, orc.FLOAT64)], 0, bench.INTERVAL,
                            [("WindowStart", 0), ("ArithmeticMean", 1)])
    assert want[0].length == windows
    for name, w in (("window_start", want[0]), ("mean", want[1])):
        assert np.array_equal(got[name], w.values[:windows][idx].astype(np.float64)), name
        assert np.array_equal(got[name + "_valid"], w.valid_mask()[idx].astype(np.float32)), name
    _, again = run(tmp_path / "b")
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)
