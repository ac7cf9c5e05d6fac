"""Differential fuzzing of aggregation.Aggregate over the whole frame (bowgpu_aggregate_whole: whole_api.cpp, the whole_* kernels of
interp_fill.hip, mode.hip) against the MODEL of tests/whole_model.py.  The oracle walks to the next valid point from every row, so the
tests that compare with it (tests/test_gpu_callers.py) keep sparse points inside one workgroup; the model costs O(n log n), and
tests/test_whole_model_cpu.py proves it against the oracle and the reference's vectors, asserts what the cases cover and that they tell
eleven wrong models from the right one.  Here, sizes from the kernel's structure (capi.whole_layout): around the 512-row step, the
65 536-row workgroup and its four wavefront quarters, up to 16 workgroups in the seeds; points planted on the last row of a workgroup /
quarter / step and the first of the next, two points with whole workgroups between them, frames that begin or end in more than a
workgroup of nulls; interval columns with duplicates, negative, at nanosecond scale beyond 2^53, also read as a value column; NaN seeds,
signalling NaNs, zeros of both signs, infinities, Int64 across all 64 bits; 1 to 64 reducers (65 declined), more than 16 on a column,
Mode next to streaming reducers, Factor chains; Arrow offsets with the bits around the column set; host, registered and device inputs,
host and device output slots.  Every case runs through the product route and through ROUTE_FORCE_GENERAL.
BOW_FUZZ_SEEDS=N runs N / 2 seeds instead of 32.

Comparison: type, length, null_count, the validity byte and the bits of a nil slot (zero) are exact; every kind outside the
order-sensitive set is bit for bit; Sum, ArithmeticMean and the four time-weighted reducers are bit for bit where the model says every
partial sum is exact (integer terms, sum |T_i| < 2^53), else |got - exact| stays within THE STATED TOLERANCE (include/bowgpu.h,
tests/tolerance.py) of one window of n rows, NaN / infinite results agree in kind.  A decline is accepted only where whole_model.outside()
says so from the inputs alone.

The planted tests use integer data, so that every expected value is int64 numpy arithmetic: 16 777 217 and 40 000 003 rows (257 and 611
workgroup records: runs of 2 and 3 records per thread of the merge), dense, 30 % nulls around one workgroup without a point, and points
in workgroups 0, 300, 302 and the last only (a record without a point between two threads' runs and inside one run); the capped
shape (2048 * 65536 + 1 rows) is in tests/test_gpu_fullsize.py.

Measured on an MI355X: a seed of test_fuzz_whole (16 cases, each through both routes) takes 0.4 s on average and 1.3 s at most, the 32
default seeds 13 s; the planted tests 0.8 s (16 777 217 rows) and 1.0 s (40 000 003 rows); the file 16 s, with BOW_FUZZ_SEEDS=256 70 s
(2.5 s the slowest seed).  Over the default seeds 512 cases ran per route: 486 served, 26 declined (16 with -9, 6 with -6, 4 with -13),
all 26 outside the domain; of the 6042 results compared per route 4142 were of bit-exact kinds, 1164 order-sensitive and integer-exact
(bit for bit), 736 order-sensitive within the bound.  Nothing differed from the model, neither there nor over 256 seeds (2048 cases per
route, 25 464 results).  Three libraries broken on purpose were seen: a merge thread's run started at t instead of t * per (the planted
tests and the capped shape fail; no older test does), no stitch across a record without a point inside a thread's run (40 000 003 rows
and the capped shape fail), Int64 First carried through a double (28 of the 32 default seeds fail)."""
import os
from collections import Counter

import numpy as np
import pytest

import whole_model as wm
from bow_amd import capi
from whole_model import FLOAT64, INT64, M

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")) // 2)
ROUTES = (("product", 0), ("general", capi.ROUTE_FORCE_GENERAL))
_seen = Counter()


def slot(o):
    """(bits, validity byte) of a one-slot output"""
    v, b = o.host_arrays()
    return int(v.view(np.uint64)[0]), int(b[0])


def check(label, a, got, want):
    """one reducer's OutColumn against the model's Res"""
    kind, factors = a[0], (list(a[2]) if len(a) > 2 and a[2] else [])
    assert got.type == want.typ and got.length == want.length, (label, a, got.type, want.typ, got.length, want.length)
    if want.length == 0:
        return
    bits, byte = slot(got)
    assert byte == (1 if want.valid else 0) and got.null_count == (0 if want.valid else 1), (label, a, byte, got.null_count, want.valid)
    if not want.valid:
        assert bits == 0, (label, a, hex(bits))                # (bowbuffer.go:84-104: a failed assertion stores the zero value)
        return
    if bits == int(want.bits):
        return
    g = float(np.array([bits], np.uint64).view(np.float64)[0])
    if kind not in wm.ORDER_SENSITIVE:
        # bit for bit; a NaN the Factor multiplication produced may differ in payload, a row's own NaN may not
        assert want.typ == FLOAT64 and factors and np.isnan(g) and np.isnan(want.as_float()), (label, a, hex(bits), hex(int(want.bits)))
        return
    e = want.exact
    if not (np.isfinite(e) and np.isfinite(g)):
        assert (np.isnan(g) and np.isnan(e)) or g == e, (label, a, g, e)
        return
    assert not want.int_exact, (label, a, "integer-exact, yet not the reference's bits", g, want.as_float())
    b = wm.bound(want, kind, factors)
    assert abs(g - e) <= b, (label, a, g, e, abs(g - e), b)


def device_cols(c):
    """(columns for the C ABI in the case's residency, cleanup)"""
    cols = wm.ccols(c)
    if c["residency"] == "device":
        return [x.to_device() for x in cols], lambda: None
    if c["residency"] == "pinned":
        pinned = []
        for x in cols:
            v = capi.page_aligned(max(x.values.size, 1), x.values.dtype)
            v[:x.values.size] = x.values
            b = None
            if x.validity is not None:
                b = capi.page_aligned(max(x.validity.size, 1), np.uint8)
                b[:x.validity.size] = x.validity
            pinned.append(capi.Column(v, b, x.type, x.offset, x.length, x.null_count).pin())
        return pinned, lambda: [x.unpin() for x in pinned]
    return cols, lambda: None


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_whole(seed):
    for c in wm.cases(seed):
        out = wm.outside(c)
        want = M.aggregate(wm.mcols(c), 0, c["aggs"]) if out is None else None
        cols, done = device_cols(c)
        try:
            for route, mask in ROUTES:
                label = "%s route=%s" % (c["label"], route)
                _seen["cases", route] += 1
                try:
                    with capi.route(mask):
                        got = capi.aggregate_whole(cols, c["ts_col"], c["aggs"], out_residency=capi.DEVICE if c["out_device"] else capi.HOST)
                except capi.BowGpuError as e:
                    assert out is not None and e.code == out, (label, out, e)
                    _seen["declined %d" % out, route] += 1
                    continue
                assert out is None, (label, "served, outside the domain", out)
                assert len(got) == len(want)
                for a, g, w in zip(c["aggs"], got, want):
                    check(label, a, g, w)
                    _seen["order-sensitive, integer-exact" if w.exact is not None and w.valid and w.int_exact else
                          "order-sensitive, within the bound" if w.exact is not None and w.valid else "bit-exact kinds", route] += 1
        finally:
            done()
    if seed == SEEDS[-1]:
        print("\ntest_fuzz_whole over %d seeds: %s" % (len(SEEDS), sorted(_seen.items())))


# ------------------------------------------------------------------ planted: the per-thread runs of the merge, integer data
PLANTED_KINDS = ("Sum", "ArithmeticMean", "Min", "Max", "First", "Last", "Count", "IntegralStep", "IntegralTrapezoid", "WeightedAverageStep",
                 "WeightedAverageLinear")


def planted_frame(n):
    """(ts, values as int64) of n rows, built once: dt is 1 or 6, values in [-50, 50] - every sum far below 2^53"""
    i = np.arange(n, dtype=np.int64)
    ts = 5 * i + i % 5
    vals = (i * 7919) % 101 - 50
    return ts, vals


def planted_valid(n, layout):
    nblocks, chunk = capi.whole_layout(n)
    if layout == "dense":
        return None
    last = (n - 1) // chunk                        # the last workgroup that has rows
    per = (nblocks + 255) // 256                   # records per thread of the merge
    mid = min(300, last // 2) // per * per         # the first record of a thread's run: 300 (128 of 257 records, 296 at the cap)
    if layout == "30 % nulls":                     # ... and one workgroup without a point, inside a thread's run where a run has three records
        valid = np.random.default_rng(n).random(n) >= 0.3
        valid[(mid + 1) * chunk:(mid + 2) * chunk] = False
        return valid
    # points in workgroups 0, mid, mid + 2 and the last only: records without a point between threads' runs and inside one
    valid = np.zeros(n, bool)
    for rows in ((17, chunk - 1), (mid * chunk, mid * chunk + 4099), ((mid + 2) * chunk + 5, (mid + 3) * chunk - 1), (last * chunk, n - 1)):
        valid[list(rows)] = True
    return valid


def planted_expected(ts, vals, valid):
    """kind -> (valid, python number) from int64 arithmetic"""
    n = len(ts)
    rows = np.arange(n) if valid is None else np.flatnonzero(valid)
    t, v = ts[rows], vals[rows]
    dt = np.diff(t)
    step = int((v[:-1] * dt).sum()) + int(v[-1]) * int(ts[-1] - t[-1])
    trap2 = int(((v[:-1] + v[1:]) * dt).sum())
    wide = float(int(ts[-1]) - int(ts[0]))
    s = int(v.sum())
    return {"Sum": float(s), "ArithmeticMean": float(s) / float(len(rows)), "Min": float(v.min()), "Max": float(v.max()), "First": int(v[0]),
            "Last": int(v[-1]), "Count": len(rows), "IntegralStep": float(step), "IntegralTrapezoid": trap2 / 2.0,
            "WeightedAverageStep": float(step) / wide, "WeightedAverageLinear": (trap2 / 2.0) / wide}


def run_planted(n, layouts=("dense", "30 % nulls", "sparse workgroups"), types=(FLOAT64, INT64)):
    ts, vals = planted_frame(n)
    dts = capi.Column(ts, None, capi.INT64, 0, n, 0).to_device()
    dvals = {typ: capi.DeviceBuffer.from_numpy(vals if typ == INT64 else vals.astype(np.float64)) for typ in types}
    aggs = [(k, 1) for k in PLANTED_KINDS]
    for layout in layouts:
        valid = planted_valid(n, layout)
        want = planted_expected(ts, vals, valid)
        dbm = None if valid is None else capi.DeviceBuffer.from_numpy(np.concatenate((np.packbits(valid, bitorder="little"), np.zeros(8, np.uint8))))
        for typ in types:
            col = capi.Column(dvals[typ], dbm, typ, 0, n, -1 if dbm is not None else 0)
            for route, mask in ROUTES:
                with capi.route(mask):
                    got = capi.aggregate_whole([dts, col], 0, aggs)
                for k, g in zip(PLANTED_KINDS, got):
                    label = (n, layout, typ, route, k)
                    w = want[k]
                    is_int = k == "Count" or (k in ("First", "Last") and typ == INT64)
                    assert g.type == (INT64 if is_int else FLOAT64) and g.length == 1 and g.null_count == 0, label
                    bits = slot(g)[0]
                    wbits = int(w) % 2 ** 64 if is_int else int(wm.f2b(float(w)))
                    assert bits == wbits, (label, hex(bits), hex(wbits), g.to_list(), w)


@pytest.mark.parametrize("n", [16_777_217, 40_000_003])
def test_whole_merge_runs_of_two_and_three_records(n):
    """nblocks = 257 and 611: thread t of whole_finish_kernel / whole_merge_kernel folds records [t * per, (t + 1) * per) with per = 2 and
    3 - a run started at t instead of t * per, or a stitch skipped at an empty record, changes Sum / First / Last / the integrals"""
    assert capi.whole_layout(n)[0] == {16_777_217: 257, 40_000_003: 611}[n]
    run_planted(n)


# ------------------------------------------------------------------ the cases of tests/test_gpu_callers.py's whole-frame tests, under the model's bound
def test_small_call_shapes():
    """64 reducers of one column served, 65 declined; WindowStart naming a Float64 column comes back nil; device-resident slots"""
    n = 1000
    ts = np.arange(n, dtype=np.int64) * 3
    vals = np.arange(n, dtype=np.float64) - 400.0
    cols = [capi.Column(ts), capi.Column(vals)]
    mcols = [wm.MCol(ts, np.ones(n, bool), INT64), wm.MCol(vals, np.ones(n, bool), FLOAT64)]
    aggs = [(wm.KINDS[i % len(wm.KINDS)], 1) for i in range(64)]
    for route, mask in ROUTES:
        with capi.route(mask):
            for resid in (capi.HOST, capi.DEVICE):
                for a, g, w in zip(aggs, capi.aggregate_whole(cols, 0, aggs, out_residency=resid), M.aggregate(mcols, 0, aggs)):
                    check("64 reducers %s" % route, a, g, w)
            with pytest.raises(capi.BowGpuError) as e:
                capi.aggregate_whole(cols, 0, aggs + [("Sum", 1)])
            assert e.value.code == -9 and "64" in e.value.message
            g = capi.aggregate_whole(cols, 0, [("WindowStart", 1), ("WindowStart", 0)])
            assert g[0].type == FLOAT64 and g[0].null_count == 1 and slot(g[0]) == (0, 0)
            assert g[1].type == INT64 and g[1].to_list() == [0]
