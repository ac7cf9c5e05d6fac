"""Differential fuzzing of Rolling.Interpolate, Interpolate(...).Aggregate(...) as one call and Bow.FillPrevious / FillNext / FillMean /
FillLinear (interpolate.hip, interp_fill.hip, rolling_fused.hip and their drivers in interpolate_api.cpp and fill_api.cpp) against the MODEL of tests/interp_model.py
- the oracle walks every null run again from every window, so tests/test_gpu_fuzz.py::test_fuzz_interpolate_and_fills, which compares
with the oracle itself, stops at 700 rows.  The model costs O(n log n); tests/test_interp_model_cpu.py proves it against the oracle
and the reference's vectors, asserts what the cases cover and that they tell eight wrong models from the right one.  Here: row counts
around the trip (512), the near walk (2048) and the index block (4096) up to 70 001 rows, null runs past 2048 / 4096 rows and on the
32 / 64 / 4096-bit edges of the offset bitmap, all-null columns, runs of thousands of empty windows, rows below s0, the -1 sentinel,
duplicates on window starts, nanosecond scale, a trip that spans 2^31, Int64 and Float64 under every interpolator, PrevRow with valid
and null halves, one to three value columns, Arrow offsets, null_count stated or not, host / device residency, both window kinds.
Bit-exact (the chain runs with strict_order: info.long_windows == 0).  BOW_FUZZ_SEEDS=N runs N / 2 seeds per test instead of 32.

A device decline (-9, -14) is accepted only where interp_model.outside() says so from the inputs alone; the CPU file bounds those
cases at a tenth of a seed's.

Measured on an MI355X, the 32 default seeds per test (24 Interpolate, 16 fill, 24 chain cases a seed): a seed of test_fuzz_interpolate
takes 0.14 s (0.36 at most), of test_fuzz_fills 0.06 s, of test_fuzz_interpolate_then_aggregate 0.08 s; the tile test 3.6 s; the file
13 s, with BOW_FUZZ_SEEDS=256 42 s.  Over the default seeds bowgpu_last_kernel_name reported: Interpolate 768 cases - interp_wave3_kernel
482, interp_tile_kernel 271 on the product's own route (negative frames, the -1 sentinel, nanosecond scale, a trip spanning 2^31) and
457 under ROUTE_INTERP_TILE, 15 declined, all 15 outside the domain (one case a seed at most); fills 512 cases, fill_kernel in every
one, in 55 with a null run beyond the near walk (the repeat with the neighbour index built); chain 768 cases - rolling_fused_kernel 400
(287 drawn inside its documented shape), the two calls 360, 8 declined (4 with -9, 4 with -14), all 8 outside.  Nothing differed from
the model, neither there nor over 256 seeds (3072 + 2048 + 3072 cases)."""
import os
from collections import Counter

import numpy as np
import pytest

import interp_model as im
from bow_amd import capi
from interp_model import M
from test_gpu_aggregate import compare
from test_gpu_callers import both_interp_kernels, cmp_out
from test_gpu_filter import POISON, make_outs, raw

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")) // 2)
GUARD = 64                 # rows of poison kept behind the capacity a call is told about

_seen = Counter()          # kernels bowgpu_last_kernel_name reported, declines, cases: over the seeds run so far (printed by the last seed)


def guarded_outs(ncols, cap, residency):
    """poisoned outputs of cap + GUARD rows that tell the call they hold `cap`"""
    outs = make_outs(ncols, cap + GUARD, residency)
    for o in outs:
        o.slots = cap
    return outs


def assert_nothing_behind(label, outs, cap):
    for o in outs:
        v, b = raw(o, cap + GUARD)
        assert (v[cap:] == POISON).all() and (b[(cap + 7) // 8:] == 0xA5).all(), label


def report(test, seed):
    if seed == SEEDS[-1]:
        print("\n%s over %d seeds: %s" % (test, len(SEEDS), sorted((k, v) for k, v in _seen.items() if k[0] == test)))


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_interpolate(seed):
    """every case through both_interp_kernels (interp_wave3_kernel, ROUTE_INTERP_TILE, device outputs padded and exact) and through the
    one-call form with a capacity of exactly the rows and of one row less (-10 naming the size, nothing written behind the buffer)"""
    T = "interp"
    for c in im.cases(seed, "interp"):
        ccols, label = im.ccols(c), c["label"]
        kw = dict(offset=c["offset"], inclusive=c["inclusive"])
        want = [w.column() for w in M.interpolate(c["ts"], im.mcols(c), c["interval"], c["interps"], **kw)]
        n_out, res = want[0].length, capi.DEVICE if c["device"] else capi.HOST
        out = im.outside(c)
        _seen[T, "cases"] += 1
        _seen[T, "outside"] += out is not None
        try:
            got = both_interp_kernels(lambda: capi.rolling_interpolate(ccols, 0, c["interval"], c["interps"], **kw))
        except capi.BowGpuError as e:
            assert out is not None and e.code == out[0] == -9 and "inclusive windows" in e.message, (label, out, e)
            with pytest.raises(capi.BowGpuError) as e1:         # the one-call form declines alike
                capi.rolling_interpolate_onepass(ccols, 0, c["interval"], c["interps"], **kw)
            assert e1.value.code == -9, (label, e1.value)
            _seen[T, "declined"] += 1
            continue
        for k in range(len(want)):
            cmp_out("%s col %d" % (label, k), got[k], want[k])
        _seen[T, capi.last_kernel_name()] += 1                 # (both_interp_kernels ends with the route the product takes)
        with capi.route(capi.ROUTE_INTERP_TILE):
            capi.rolling_interpolate(ccols, 0, c["interval"], c["interps"], **kw)
            _seen[T, capi.last_kernel_name() + " (ROUTE_INTERP_TILE)"] += 1
        # bowgpu_rolling_interpolate_fill on its own: buffers of exactly the rows ...
        outs = guarded_outs(len(want), n_out, res)
        capi.rolling_interpolate_onepass(ccols, 0, c["interval"], c["interps"], outs=outs, **kw)
        for k in range(len(want)):
            cmp_out("%s one call, exact capacity, col %d" % (label, k), outs[k], want[k])
        assert_nothing_behind(label + " one call, exact capacity", outs, n_out)
        # ... and one row short
        if n_out > 0:
            outs = guarded_outs(len(want), n_out - 1, res)
            with pytest.raises(capi.BowGpuError) as e:
                capi.rolling_interpolate_onepass(ccols, 0, c["interval"], c["interps"], outs=outs, **kw)
            assert e.value.code == -10 and str(n_out) in e.value.message, (label, e.value)
            assert_nothing_behind(label + " one call, one row short", outs, n_out - 1)
    report(T, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_fills(seed):
    """the three methods of bowgpu_fill and bowgpu_fill_linear (plain and with the reference column checked by the caller), each into a
    host-resident output, a device-resident one of exactly the rows and one padded to 512 rows: values, validity, null_count, `unchanged`"""
    T = "fill"
    for c in im.cases(seed, "fill"):
        ccols, label, n = im.ccols(c), c["label"], c["n"]
        col, ref = im.mcols(c)[0], im.ref_mcol(c)
        forms = ((capi.HOST, None), (capi.DEVICE, None), (capi.DEVICE, (n + 511) // 512 * 512))
        _seen[T, "cases"] += 1
        _seen[T, "null run beyond the near walk: the index is built"] += im.fill_needs_the_index(col.valid)
        for method in ("Previous", "Next", "Mean"):
            want, wu = M.fill(col, method)
            for resid, cap in forms:
                got, gu = capi.fill(ccols[0], method, out_residency=resid, capacity=cap)
                assert gu == wu, (label, method)
                cmp_out("%s Fill%s" % (label, method), got, want.column())
            _seen[T, capi.last_kernel_name()] += 1
        r = M.fill_linear(ref, col)
        for checked in (False, True):
            if checked and not (len(r) == 2 and ref.valid.any()):
                continue         # (bowgpu_fill_linear_sorted is for a caller whose own bowfill.go:35-42 passed: a ref column with a value, in order)
            for resid, cap in forms:
                if len(r) == 1:
                    with pytest.raises(capi.BowGpuError) as e:
                        capi.fill_linear([ccols[1], ccols[0]], 0, 1, out_residency=resid, capacity=cap)
                    assert e.value.code == r[0], (label, e.value)
                    continue
                got, gu = capi.fill_linear([ccols[1], ccols[0]], 0, 1, out_residency=resid, capacity=cap, ref_checked=checked)
                assert gu == r[1], (label, checked)
                cmp_out("%s FillLinear checked=%d" % (label, checked), got, r[0].column())
    report(T, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_interpolate_then_aggregate(seed):
    """bowgpu_rolling_interpolate_aggregate as one call and in the two-call form of the same entry point (ROUTE_NO_FUSED), both against
    model -> oracle aggregate; the two forms decline alike, and only where interp_model.outside() says so.  rolling_fused_kernel has to
    serve half as many cases of a seed as lie inside the kernel's documented shape (include/bowgpu.h; interp_model.in_the_fused_shape -
    tests/test_interp_model_cpu.py asserts FUSED_SHAPED_MIN of them and more in every seed): a tile the kernel cannot describe may still
    send such a call back to the two calls, and frames outside the stated shape may be served."""
    T = "chain"
    fused = shaped = 0
    for c in im.cases(seed, "chain"):
        ccols, label = im.ccols(c), c["label"]
        kw = dict(offset=c["offset"], inclusive=c["inclusive"])
        out = im.outside(c)
        _seen[T, "cases"] += 1
        _seen[T, "outside"] += out is not None
        shaped += im.in_the_fused_shape(c)
        res = {}
        for form, mask in (("one call", 0), ("two-call form", capi.ROUTE_NO_FUSED)):
            with capi.route(mask):
                try:
                    res[form] = capi.rolling_interpolate_aggregate(ccols, 0, c["interval"], c["interps"], c["aggs"], strict_order=True, **kw)
                    if mask == 0:
                        took = capi.last_kernel_name() == "rolling_fused_kernel"
                        fused += took
                        _seen[T, "rolling_fused_kernel" if took else "two calls"] += 1
                except capi.BowGpuError as e:
                    res[form] = e
        errs = [r for r in res.values() if isinstance(r, capi.BowGpuError)]
        if errs:
            assert len(errs) == 2 and errs[0].code == errs[1].code, (label, res)
            assert out is not None and errs[0].code == out[0], (label, out, errs[0])
            assert out[0] == -14 or "inclusive windows" in errs[0].message, (label, errs[0])
            _seen[T, "declined %d" % out[0]] += 1
            continue
        want, nic = M.interpolate_aggregate(c["ts"], im.mcols(c), c["interval"], c["interps"], c["aggs"], **kw)
        for form, (outs, info) in res.items():
            assert info.new_interval_col == nic and info.long_windows == 0, label
            for a, g, w in zip(c["aggs"], outs, want):
                compare("%s %s %s" % (label, form, a[0]), g, w)
    assert fused >= max(im.FUSED_FLOOR, shaped // 2), (fused, shaped)
    _seen[T, "in the fused kernel's shape"] += shaped
    report(T, seed)


# ------------------------------------------------------------------ the neighbour index across its tiles
TILE_BITS = 1024 * im.BLOCK_BITS       # interp_fill.hip nbr_scan_kernel: a tile is 1024 blocks of kNbrBlockBits bits = 4 194 304


def planted_layouts(nbits):
    """valid BITS of the offset bitmap (bit = Arrow offset + row), by layout"""
    T1, T2 = TILE_BITS, 2 * TILE_BITS
    return {
        # leading nulls; a run that ends on the last bit of tile 0; rows either side of both edges; a run that begins on the first bit of
        # tile 2; trailing nulls
        "runs on the edges": [7000, 7001, 1_000_000, T1 - 3000, T1, T1 + 1, T1 + 2, 6_000_000, T2 - 2, T2 - 1, T2 + 3000, nbits - 9000],
        # the whole of tile 1 null: its tile_hi is -1 and the carry of everything behind it comes from tile 0 (and tile_lo from tile 2)
        "tile 1 all null": [3, 4, 2_000_000, T1 - 2, T1 - 1, T2, T2 + 1, nbits - 1],
    }


def test_neighbour_index_across_its_tiles():
    """nbr_scan_kernel folds the tiles before and after its own into a carry; a second tile exists only above 4 194 304 bits, and no other
    test builds the index of a value column that long (the seeded sizes end at 70 001 rows).  9 000 000 Float64 rows, valid only at
    planted bits, one layout at Arrow offset 0 and one at 3: the three fills and FillLinear with ref = row number, Interpolate Linear (both kernels) and
    StepPrevious over ~3000 windows whose starts lie inside the runs - all against the model."""
    nbits = 9_000_000 + 3
    vals = np.arange(nbits, dtype=np.float64) * 0.5 - 1e6
    tsb = np.arange(nbits, dtype=np.int64) * 5 + 11
    refb = np.arange(nbits, dtype=np.int64)
    for (name, bits_at), offsets in zip(planted_layouts(nbits).items(), ((0,), (3,))):     # (each layout at one offset: the test stays at a few seconds)
        bits = np.zeros(nbits, bool)
        bits[bits_at] = True
        bm = np.packbits(bits, bitorder="little")
        for off in offsets:
            n = 9_000_000
            valid = bits[off:off + n]
            col = im.MCol(vals[off:off + n], valid, im.FLOAT64)
            assert im.fill_needs_the_index(valid) and im.longest_null_run(valid) > TILE_BITS // 2       # far beyond the near walk: the repeat with the index
            dcol = capi.Column(vals, bm, capi.FLOAT64, off, n, -1).to_device()
            label = "%s off=%d" % (name, off)
            for method in ("Previous", "Next", "Mean"):
                want, _ = M.fill(col, method)
                got, unchanged = capi.fill(dcol, method, out_residency=capi.DEVICE, capacity=(n + 511) // 512 * 512)
                assert not unchanged and capi.last_kernel_name() == "fill_kernel"
                cmp_out("%s Fill%s" % (label, method), got, want.column())
            dref = capi.Column(refb, None, capi.INT64, off, n, 0).to_device()
            want, _ = M.fill_linear(im.MCol(refb[off:off + n], np.ones(n, bool), im.INT64), col)
            got, _ = capi.fill_linear([dref, dcol], 0, 1, out_residency=capi.DEVICE)
            cmp_out(label + " FillLinear", got, want.column())
            del dref
            ts = tsb[off:off + n]
            dts = capi.Column(tsb, None, capi.INT64, off, n, 0).to_device()
            interval = 5 * 3001 + 2
            far = Counter()

            class Far(im.Model):
                def note(self, **f):
                    if "linear" in f:
                        L = f["linear"]
                        far["across"] += int((L["ok"] & (L["back"] > 1000) & (L["ahead"] > 1000) & (L["back"] + L["ahead"] + 8 >= TILE_BITS)).sum())
            for kind, masks in (("Linear", (0, capi.ROUTE_INTERP_TILE)), ("StepPrevious", (0,))):
                ip = [{"kind": "WindowStart", "col": 0}, {"kind": kind, "col": 1, "prev": (float(ts[0] - 3), True, 42.5, True, 42)}]
                want = [w.column() for w in Far().interpolate(ts, [col], interval, ip, offset=7)]
                assert want[0].length - n in range(2000, 4000)
                for mask in masks:
                    with capi.route(mask):
                        got = capi.rolling_interpolate([dts, dcol], 0, interval, ip, offset=7, out_residency=capi.DEVICE)
                        assert capi.last_kernel_name() == ("interp_tile_kernel" if mask else "interp_wave3_kernel")
                    for k in range(2):
                        cmp_out("%s %s route=%d col %d" % (label, kind, mask, k), got[k], want[k])
                    del got
            if name == "tile 1 all null":
                assert far["across"] > 100, far          # synthetic rows inside tile 1: their two points lie in tile 0 and in tile 2
            del dts, dcol
