"""The two small blocks of a thread's context - the scratch block in device memory and the registered host block - are shared by every
entry point of the thread (bow_amd/csrc/ctx_blocks.h states their layouts and which regions may hold data at the same time).  What a call
leaves in them must not matter to the next one: one call of every family that uses the blocks, made on ONE thread in two different orders,
gives bit for bit what the same call gives as the first call of a fresh thread."""
import os
import threading

import numpy as np
import pytest

from bow_amd import capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 1000
AGGS = [("WindowStart", 0), ("Sum", 1), ("ArithmeticMean", 1), ("Min", 1), ("Max", 1), ("Count", 1), ("First", 1), ("Last", 1)]


def _snap(out):
    """an output column as comparable bytes: type, length, null count, validity bits, the values of the valid rows"""
    vals, _ = out.host_arrays()
    m = out.valid_mask()
    return (out.type, out.length, out.null_count, m.tobytes(), vals.view(np.uint64)[m].tobytes())


def _snaps(outs):
    return tuple(_snap(o) for o in outs)


def _calls():
    """name -> a function that makes the call and returns its result as comparable values.  The inputs are device-resident and state no
    null count, so that the count of a column's nulls runs inside the calls; whole-number values, so that no sum depends on its order."""
    rng = np.random.default_rng(20)
    ts = np.cumsum(rng.integers(1, 5, N)).astype(np.int64)
    vals = rng.integers(-50, 50, N).astype(np.float64)
    valid = rng.random(N) > 0.3
    valid[0] = valid[-1] = True
    bm = np.packbits(valid, bitorder="little")
    key = rng.permutation(N).astype(np.int64)
    d_ts = capi.Column(ts, None, capi.INT64).to_device()
    d_val = capi.Column(vals, bm, capi.FLOAT64, 0, N, -1).to_device()
    d_key = capi.Column(key, None, capi.INT64).to_device()
    parquet = os.path.join(HERE, "golden", "bow1-1000-rows.parquet")

    def aggregate():
        return _snaps(capi.rolling_aggregate([d_ts, d_val], 0, 10, AGGS, offset=3)[0])

    def aggregate_planned():
        plan = capi.plan_windows_ex(d_ts, 10, 3)
        return _snaps(capi.rolling_aggregate([d_ts, d_val], 0, 10, AGGS, offset=3, plan=plan)[0])

    def interpolate():   # count + fill; padded device-resident outputs: their bitmaps are written in place
        interps = [{"kind": "WindowStart", "col": 0}, {"kind": "Linear", "col": 1}]
        return _snaps(capi.rolling_interpolate([d_ts, d_val], 0, 10, interps, offset=3, out_residency=capi.DEVICE, padded=True))

    def fill_previous():
        out, unchanged = capi.fill(d_val, "Previous")
        return _snap(out), unchanged

    def fill_linear():
        out, unchanged = capi.fill_linear([d_ts, d_val], 0, 1)
        return _snap(out), unchanged

    def is_col_sorted():
        return capi.is_col_sorted(d_ts), capi.is_col_sorted(d_key), capi.is_col_sorted(d_val)

    def aggregate_whole():
        return _snaps(capi.aggregate_whole([d_ts, d_val], 0, AGGS[1:]))

    def sort_by_col():   # the key, and a nullable value column whose nulls are counted under the call
        outs, unchanged = capi.sort_by_col([d_key, d_val], 0)
        return _snaps(outs), unchanged

    def filter_rows():
        outs, first, count, contiguous = capi.filter([d_key, d_val], [(1, [float(v) for v in range(-50, 50, 4)])])
        return _snaps(outs), first, count, contiguous

    def convert():
        return _snaps(capi.convert([d_val, d_key], ["int64", "float64"]))

    def find():
        return capi.find_next(d_key, 17), capi.find_next(d_val, None), capi.find_next(d_key, N + 5)

    def parquet_column():
        f = capi.ParquetFile(parquet)
        try:
            i = next(i for i, (_, typ, _) in enumerate(f.columns) if typ in (capi.INT64, capi.FLOAT64))
            return _snap(f.read_column(i))
        finally:
            f.close()

    fns = [aggregate, aggregate_planned, interpolate, fill_previous, fill_linear, is_col_sorted, aggregate_whole, sort_by_col, filter_rows,
           convert, find, parquet_column]
    return {f.__name__: f for f in fns}


def _on_a_thread(work):
    box = {}

    def run():
        try:
            box["result"] = work()
        except BaseException as ex:   # noqa: BLE001 - raised again by the caller's thread
            box["error"] = ex

    th = threading.Thread(target=run)
    th.start()
    th.join(timeout=120)
    assert not th.is_alive(), "the worker hangs"
    if "error" in box:
        raise box["error"]
    return box["result"]


@pytest.fixture(scope="module")
def calls():
    return _calls()


@pytest.fixture(scope="module")
def fresh(calls):
    """every call as the first call of a thread of its own: computed once, never changed"""
    return {name: _on_a_thread(fn) for name, fn in calls.items()}


def test_the_calls_do_something(fresh):
    """(the comparison below is worth what the calls compute: outputs with rows, with nulls, and a search that finds its row)"""
    aggs = fresh["aggregate"]
    assert aggs[0][1] > 50 and any(a[2] > 0 for a in aggs) and fresh["aggregate_planned"] == aggs
    assert fresh["interpolate"][0][1] > N and fresh["interpolate"][0][2] == 0
    assert fresh["fill_previous"][1] is False and fresh["fill_linear"][1] is False
    assert fresh["is_col_sorted"] == (True, False, False)
    assert fresh["sort_by_col"][1] is False and fresh["sort_by_col"][0][1][2] > 0
    assert 50 < fresh["filter_rows"][2] < N and fresh["filter_rows"][3] is False
    assert fresh["convert"][0][2] > 0
    assert fresh["find"][0] >= 0 and fresh["find"][1] >= 0 and fresh["find"][2] == -1
    assert fresh["parquet_column"][1] == N


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_a_call_does_not_depend_on_what_ran_before_it_on_the_thread(calls, fresh, order):
    names = list(calls)
    # backward, and rotated: every call also follows another one than in the forward order's first round
    seq = names + names[3:] + names[:3] if order == "forward" else names[::-1] + names[::-2]
    got = _on_a_thread(lambda: [(name, calls[name]()) for name in seq])
    for k, (name, result) in enumerate(got):
        assert result == fresh[name], "%s as call %d of %s differs from the same call on a fresh thread" % (name, k, seq)
