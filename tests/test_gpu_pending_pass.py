"""A pass that bowgpu_shard_pass_begin puts in flight and nobody collects (include/bowgpu.h, "the shard protocol"): every other
entry point of the thread settles and drops it before it touches the thread's scratch, and a thread that exits with one in flight
gives its device memory back all the same (bow_amd/csrc/runtime.cpp ThreadState, shard_api.cpp PendingPass)."""
import threading
import time

import numpy as np
import pytest

from bow_amd import capi, sharded
from oracle import pyoracle as orc
from test_gpu_aggregate import compare

pytestmark = pytest.mark.gpu

AGGS = [("WindowStart", 0), ("Sum", 1), ("Min", 1), ("Max", 1)]
INTERVAL = 10


def _frame(seed, n):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)
    vals = np.round(rng.standard_normal(n) * 100, 2)
    bm = np.packbits(rng.random(n) >= 0.2, bitorder="little")
    return ts, vals, bm


def _cols(ts, vals, bm, device):
    cols = [capi.Column(ts, None, capi.INT64), capi.Column(vals, bm, capi.FLOAT64, 0, len(vals), -1)]
    return [c.to_device() for c in cols] if device else cols


def _oracle(ts, vals, bm):
    return orc.aggregate([orc.Column(ts, None, orc.INT64), orc.Column(vals, bm, orc.FLOAT64)], 0, INTERVAL, AGGS)[0]


def _bits(provider):
    return [(o.host_arrays()[0].view(np.uint64).copy(), o.valid_mask().copy()) for o in provider.outs]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_pass_left_in_flight_is_dropped_by_the_next_call(device):
    shard, other = _frame(11, 200_000), _frame(12, 100_000)
    want_shard, want_other = _oracle(*shard), _oracle(*other)
    residency = None if device else capi.HOST

    def provider():
        return sharded.GpuProvider(_cols(*shard, device), 0, INTERVAL, AGGS, out_residency=residency)

    plain = provider()
    sharded.run_local([plain])                    # begin -> pass_begin -> plan -> finish, nothing in between
    for (k, _), g, w in zip(AGGS, plain.outs, want_shard):
        compare("uninterrupted %s" % k, g, w)

    p = provider()
    assert p.pass_begin(p.begin())                # in flight on this thread's stream, never collected
    outs, _ = capi.rolling_aggregate(_cols(*other, device), 0, INTERVAL, AGGS)   # ... another call of this thread: it reuses the scratch
    for (k, _), g, w in zip(AGGS, outs, want_other):
        compare("the call in between %s" % k, g, w)
    sharded.run_local([p])
    for (k, _), g, w in zip(AGGS, p.outs, want_shard):
        compare("after the interruption %s" % k, g, w)
    for (k, _), (gv, gm), (wv, wm) in zip(AGGS, _bits(p), _bits(plain)):
        assert np.array_equal(gm, wm) and np.array_equal(gv, wv), k


def test_a_thread_that_exits_with_a_pass_in_flight_gives_its_memory_back():
    """The shape of test_a_thread_that_exits_gives_its_device_memory_back (test_gpu_threads.py); here the worker's last act is a
    bowgpu_shard_pass_begin whose kernels, staged columns and scratch are still in use when its thread-local state is destroyed."""
    n = 8_000_000
    ts = np.arange(n, dtype=np.int64)
    vals = np.ones(n)
    small = _frame(13, 100_000)
    want = _oracle(*small)
    # host-resident columns and outputs: the pass stages 2 x 64 MB through the worker's scratch cache and owns every device byte of the call
    p = sharded.GpuProvider([capi.Column(ts, None, capi.INT64), capi.Column(vals, None, capi.FLOAT64)], 0, INTERVAL, AGGS, out_residency=capi.HOST)
    # the record is made HERE: range_state_kernel spills to private memory, and the ~0.8 GB the HIP runtime sets aside for that belong to
    # a hardware queue of the process, not to the thread whose stream happened to run the kernel first
    record = p.begin()
    capi.rolling_aggregate(_cols(*small, False), 0, INTERVAL, AGGS)
    capi.trim(True)
    free0, _ = capi.mem_info()
    seen = {}
    begun, leave = threading.Event(), threading.Event()

    def work():
        try:
            seen["in_flight"] = p.pass_begin(record)   # the worker's ONLY call into the library: any other after it would settle and drop the pass
        finally:
            begun.set()
        leave.wait(60)

    th = threading.Thread(target=work)
    th.start()
    assert begun.wait(120)
    seen["during"] = capi.mem_info()[0]               # (asked from THIS thread: the worker's pass stays in flight)
    leave.set()
    th.join()
    # (Thread.join returns when the Python side of the thread is done; the OS thread runs its thread-local destructors a moment later)
    deadline = time.monotonic() + 10.0
    while True:
        free1, _ = capi.mem_info()
        if free0 - free1 < 64 << 20 or time.monotonic() > deadline:
            break
        time.sleep(0.05)
    assert seen["in_flight"]
    assert free0 - seen["during"] > 100 << 20          # the worker did hold its staging blocks while it lived ...
    assert free0 - free1 < 64 << 20, (free0, free1)    # ... and they are gone with it
    outs, _ = capi.rolling_aggregate(_cols(*small, False), 0, INTERVAL, AGGS)
    for (k, _), g, w in zip(AGGS, outs, want):
        compare("main thread afterwards %s" % k, g, w)
