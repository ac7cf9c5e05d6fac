"""Differential fuzzing of the frame operations - bowgpu_argsort, take, sort_by_col, sort_by_col_sharded, filter_mask, compact, filter,
valid_mask, drop_nils, diff, distinct, append, find_next, join_rows, join - alone and chained on the device, against the model of
tests/frame_model.py.  frame_model.plans(seed) is data (frames, arguments, the model's expectation for every step); this file places the
frames in memory as the plan says (Arrow offsets into longer buffers with junk around the slice, bitmaps absent or present, null_count
stated or -1, HOST / DEVICE / HOST_PINNED per column), makes the calls and compares after every step: values as uint64 with 0 in the
null slots, validity bytes with clear padding bits, null_count, length and type, index outputs index for index, every count, and the
sentinels of the output buffers past the slots produced - everywhere when a call declines, answers contiguous or unchanged, or finds
nothing distinct.  The one exception: a Diff slot the model marks as a NaN the subtraction generates must be a NaN, of any bits.
BOW_FUZZ_SEEDS=N runs N seeds instead of 64 (half of them per test, as tests/test_gpu_fuzz.py does).  What the plans cover, and that a
subtly wrong kernel would be seen, is asserted without a GPU in tests/test_frame_model_cpu.py."""
import copy
import os

import numpy as np
import pytest

import frame_model as fm
from bow_amd import capi
from oracle import pyoracle as orc
from test_gpu_aggregate import compare
from test_gpu_filter import POISON, assert_untouched, make_outs, raw

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("BOW_FUZZ_SEEDS", "64")) // 2)
M = fm.Model()
UNDEFINED_ON_ERROR = ("take", "sort_by_col_sharded")      # include/bowgpu.h: "the output is then undefined"


# ------------------------------------------------------------------ frames in memory
def build_column(mc, phys, pinned):
    """the model column at phys["offset"] rows into longer buffers: junk values and stray validity bits before and behind the slice"""
    n, off, dt = len(mc.bits), phys["offset"], fm.DTYPE[mc.typ]
    values = np.concatenate([np.full(off, -77, dt), mc.bits.view(dt), np.full(3, -78, dt)])
    if phys["bitmap"]:
        bm = np.packbits(np.concatenate([np.arange(off) % 2 == 0, mc.valid, np.ones(5, bool)]), bitorder="little")
        nulls = int((~mc.valid).sum()) if phys["known"] else -1
    else:
        assert mc.valid.all()
        bm, nulls = None, 0
    if phys["res"] == fm.PINNED:
        pv, pb = capi.page_aligned(len(values), dt), None if bm is None else capi.page_aligned(len(bm), np.uint8)
        pv[:] = values
        if bm is not None:
            pb[:] = bm
        c = capi.Column(pv, pb, mc.typ, off, n, nulls).pin()
        pinned.append(c)
        return c
    c = capi.Column(values, bm, mc.typ, off, n, nulls)
    return c.to_device() if phys["res"] == fm.DEVICE else c


def slice_col(c, first, count):
    """rows [first, first + count) of a column: the same buffers, a new Arrow offset"""
    s = copy.copy(c)
    s.offset, s.length, s.null_count = c.offset + first, count, 0 if c.validity is None else -1
    return s


def cut_cols(cols, lens):
    out, at = [], 0
    for n in lens:
        out.append([slice_col(c, at, n) for c in cols])
        at += n
    return out


def mask_arg(bits, res):
    m = M.pack(bits)
    return capi.DeviceBuffer.from_numpy(m) if res == fm.DEVICE else m


def mask_bytes(buf, n):
    nb = (n + 7) // 8
    return buf.to_numpy(np.uint8, nb) if isinstance(buf, capi.DeviceBuffer) else np.asarray(buf[:nb])


# ------------------------------------------------------------------ the comparison
def assert_cols(label, want, outs, cap, gen_nan=None):
    assert len(outs) == len(want), label
    for i, (w, o) in enumerate(zip(want, outs)):
        n = len(w.bits)
        nb = (n + 7) // 8
        v, b = raw(o, cap)
        assert (o.length, o.type, o.null_count) == (n, w.typ, int((~w.valid).sum())), (label, i)
        got, bits = v[:n], w.bits
        if gen_nan is not None and gen_nan[i].any():
            g = gen_nan[i]
            assert np.isnan(got[g].view(np.float64)).all(), (label, i)       # a NaN the subtraction generated: the device's bits
            got, bits = got[~g], bits[~g]
        bad = np.flatnonzero(got != bits)
        assert bad.size == 0, (label, i, bad[:8], got[bad[:4]], bits[bad[:4]])       # raw payloads; null slots hold 0
        assert np.array_equal(b[:nb], M.pack(w.valid)), (label, i)                  # validity; the padding bits of the last byte clear
        assert (v[n:cap] == POISON).all() and (b[nb:] == 0xA5).all(), (label, i)    # nothing past the slots produced


def outs_for(step, r, pieces):
    """(number of outputs, capacity) of a call that fills output columns"""
    op, a, fr = step["op"], step["args"], step["frames"]
    n = fm.rows_of(fr[0]) if fr else 0
    if op == "take":
        return 1, len(a["idx"]) + 3
    if op == "sort_by_col":
        return len(fr[0]), n + 3
    if op in ("compact", "filter", "drop_nils"):
        return len(fr[0]), n if a.get("cap") is None else a["cap"]
    if op == "diff":
        sel = M.select_cols(len(fr[0]), a["col_idx"])
        return len(sel), n + 3
    if op == "distinct":
        return 1, n if a.get("cap") is None else a["cap"]
    if op == "append":
        return len(fr[0]), sum(fm.rows_of(f) for f in fr) + 3 if a.get("cap") is None else a["cap"]
    if op == "join":
        nouts = len(fr[0]) + len(fr[1]) - (0 if a["lk"] == -1 else 1)
        want = 0 if fm.declined(r) else r.rows
        return nouts, want + 3 if a.get("cap") is None else a["cap"]
    return 0, 0


def call(step, frames, outs):
    """the call of one step -> what it answered, in the model's words"""
    op, a = step["op"], step["args"]
    f = frames[0] if frames else []
    res = step["out_res"]
    if op == "argsort":
        perm, srt = capi.argsort(f[a["col"]], out_residency=fm.DEVICE if res == fm.DEVICE else fm.HOST)
        if perm is not None and isinstance(perm, capi.DeviceBuffer):
            perm = perm.to_numpy(np.int64, f[a["col"]].length)
        return fm.R(sorted=int(srt), idx=None if srt else [perm])
    if op == "take":
        idx = capi.DeviceBuffer.from_numpy(a["idx"]) if a["idx_res"] == fm.DEVICE else a["idx"]
        capi.take(f[a["col"]], idx, n_idx=len(a["idx"]), out=outs[0])
        return fm.R(cols=outs)
    if op == "sort_by_col":
        _, unchanged = capi.sort_by_col(f, a["key"], outs=outs)
        return fm.R(unchanged=int(unchanged), cols=None if unchanged else outs)
    if op in ("filter_mask", "valid_mask"):
        am = None if a.get("and_mask") is None else mask_arg(a["and_mask"], a["mask_res"])
        mres = fm.DEVICE if a["mask_res"] == fm.DEVICE else fm.HOST
        if op == "filter_mask":
            buf, sel, first, last = capi.filter_mask(f, a["preds"], and_mask=am, out_residency=mres)
        else:
            buf, sel, first, last = capi.valid_mask(f, a["col_idx"], and_mask=am, out_residency=mres, want_mask=a["want_mask"])
        return fm.R(selected=sel, first=first, last=last, mask_bytes=None if buf is None else mask_bytes(buf, f[0].length))
    if op in ("compact", "filter", "drop_nils"):
        if op == "compact":
            _, first, count, contiguous = capi.compact(f, mask_arg(a["mask"], a["mask_res"]), outs=outs)
        elif op == "filter":
            am = None if a.get("and_mask") is None else mask_arg(a["and_mask"], a.get("mask_res", fm.HOST))
            _, first, count, contiguous = capi.filter(f, a["preds"], and_mask=am, outs=outs)
        else:
            _, first, count, contiguous = capi.drop_nils(f, a["col_idx"], outs=outs)
        return fm.R(contiguous=int(contiguous), first=first, count=count, cols=None if contiguous else outs)
    if op == "diff":
        capi.diff(f, a["col_idx"], outs=outs)
        return fm.R(cols=outs)
    if op == "distinct":
        _, nd = capi.distinct(f[a["col"]], out=outs[0])
        return fm.R(n_distinct=nd, cols=outs if nd else None)
    if op == "append":
        _, unchanged = capi.append(frames, outs=outs)
        return fm.R(unchanged=int(unchanged), cols=None if unchanged else outs)
    if op == "find_next":
        return fm.R(row=capi.find_next(f[a["col"]], a["value"], a["row_start"]))
    if op == "join_rows":
        lk, rk = frames[0][a["lk"]], frames[1][a["rk"]]
        _, _, rows, pairs = capi.join_rows(lk, rk, a["kind"], count_only=True)
        gl, gr, rows2, pairs2 = capi.join_rows(lk, rk, a["kind"], out_residency=fm.DEVICE if res == fm.DEVICE else fm.HOST,
                                               capacity=rows + 3)
        assert (rows2, pairs2) == (rows, pairs)
        if res == fm.DEVICE:
            gl, gr = gl.to_numpy(np.int64, rows), gr.to_numpy(np.int64, rows)
        else:
            assert (gl[rows:] == -7).all() and (gr[rows:] == -7).all()       # nothing past the rows produced
        return fm.R(rows=rows, pairs=pairs, idx=[gl[:rows], gr[:rows]])
    if op == "join":
        _, rows = capi.join(frames[0], a["lk"], frames[1], a["rk"], a["kind"], outs=outs)
        return fm.R(rows=rows, cols=outs)
    raise ValueError(op)


def check(label, step, got, cap):
    want = step["expect"]
    for k, v in want.items():
        if isinstance(v, (int, np.integer)) and k not in ("merged_ranks", "pairs") or k == "pairs" and "pairs" in got:
            assert got[k] == v, (label, k, got[k], v)
    if want.idx is not None or got.idx is not None:
        assert len(got.idx) == len(want.idx), label
        for g, w in zip(got.idx, want.idx):
            assert np.array_equal(g, w), (label, np.flatnonzero(g != w)[:8])
    if want.mask is not None and got.mask_bytes is not None:
        assert np.array_equal(got.mask_bytes, M.pack(want.mask)), label
    if want.cols is not None:
        assert_cols(label, want.cols, got.cols, cap, want.gen_nan)


def run_sharded(label, step, cols):
    """bowgpu_sort_by_col_sharded on one device id repeated: against the model, and against bowgpu_sort_by_col of the concatenation"""
    a, want, res = step["args"], step["expect"], step["out_res"]
    ranks = cut_cols(cols, a["cuts"])
    n, nc = cols[0].length, len(cols)
    outs = [make_outs(nc, m + 2, res) for m in a["cuts"]]
    one = make_outs(nc, n, res)
    if fm.declined(want):
        for f in (lambda: capi.sort_by_col_sharded(ranks, a["key"], [0] * len(ranks), outs=outs), lambda: capi.sort_by_col(cols, a["key"], outs=one)):
            with pytest.raises(capi.BowGpuError) as e:
                f()
            assert e.value.code == want[0], (label, e.value)
        return None
    _, unchanged = capi.sort_by_col_sharded(ranks, a["key"], [0] * len(ranks), outs=outs)
    info = capi.sort_by_col_sharded_info()
    _, unchanged1 = capi.sort_by_col(cols, a["key"], outs=one)
    assert unchanged == unchanged1 == bool(want.unchanged), label
    if unchanged:
        for o, m in zip(outs + [one], a["cuts"] + [n - 2]):
            assert_untouched(o, m + 2)
        return None
    if want.merged_ranks:
        assert info.merged_ranks > 0, (label, want.merged_ranks)
    for r, (o, w, m) in enumerate(zip(outs, want.ranks, a["cuts"])):
        assert_cols("%s rank %d" % (label, r), w, o, m + 2)
    for i in range(nc):      # the header's guarantee: the outputs concatenated are what the one-device call gives, bit for bit
        v1, b1 = raw(one[i], n)
        assert np.array_equal(np.concatenate([raw(o[i], m + 2)[0][:m] for o, m in zip(outs, a["cuts"])]), v1[:n]), (label, i)
        assert np.array_equal(M.pack(np.concatenate([w[i].valid for w in want.ranks])), b1[:(n + 7) // 8]), (label, i)
    return outs


def run_step(label, step, frames):
    """one step on the physical frames -> the outputs it filled (None: it filled none)"""
    want = step["expect"]
    if step["op"] == "sort_by_col_sharded":
        return run_sharded(label, step, frames[0])
    nouts, cap = outs_for(step, want, frames)
    outs = make_outs(nouts, cap, step["out_res"])
    if fm.declined(want):
        with pytest.raises(capi.BowGpuError) as e:
            call(step, frames, outs)
        assert e.value.code == want[0], (label, e.value)
        if step["op"] not in UNDEFINED_ON_ERROR:
            assert_untouched(outs, cap)
        return None
    got = call(step, frames, outs)
    check(label, step, got, cap)
    if want.cols is None:
        assert_untouched(outs, cap)          # contiguous, unchanged, nothing distinct: the outputs are not written
        return None
    return outs


def release(pinned):
    for c in pinned:
        c.unpin()


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_frame_ops(seed):
    for i, (kind, step) in enumerate(fm.plans(seed)):
        if kind != "op":
            continue
        pinned = []
        try:
            frames = [[build_column(c, p, pinned) for c, p in zip(f["cols"], f["phys"])] for f in step["inputs"]]
            run_step("seed %d case %d %s" % (seed, i, step["op"]), step, frames)
        finally:
            release(pinned)


def run_chain(label, chain, pinned):
    """-> the physical frames behind the last step"""
    current = None
    for j, step in enumerate(chain["steps"]):
        mine = iter(current or [])
        frames = [[build_column(c, p, pinned) for c, p in zip(f["cols"], f["phys"])] if f["phys"] else next(mine) for f in step["inputs"]]
        outs = run_step("%s step %d %s" % (label, j, step["op"]), step, frames)
        nxt = step.get("next", ("same",))
        if nxt is None:
            return None
        at = [step.get("self", 0)]
        if nxt[0] == "outs":
            current = [[capi.out_as_column(o) for o in outs]]
        elif nxt[0] == "ranks":
            current = [[capi.out_as_column(o) for o in rank] for rank in outs]
        elif nxt[0] == "slice":
            current = [[slice_col(c, nxt[1], nxt[2]) for c in frames[at[0]]]]
        elif step["op"] != "find_next":
            current = [frames[at[0]]]
    return current


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_frame_chains(seed):
    for i, (kind, chain) in enumerate(fm.plans(seed)):
        if kind != "chain":
            continue
        pinned = []
        try:
            run_chain("seed %d chain %d" % (seed, i), chain, pinned)
        finally:
            release(pinned)


@pytest.mark.parametrize("seed", [0, 1])
def test_chain_ends_in_a_rolling_call(seed):
    """The pipeline of the header: a frame with nulls and an unsorted Int64 time column goes through DropNils, Filter and SortByCol
    with device-resident outputs, and the sorted frame is handed, still in HBM, to Rolling.Aggregate.  The value columns hold
    multiples of 1/2 and small integers, so every sum is exact and the means are the same bits in whatever order a route adds."""
    chain = fm.rolling_plan(seed)
    pinned = []
    try:
        cols = run_chain("rolling seed %d" % seed, chain, pinned)[0]
        assert all(c.residency == capi.DEVICE for c in cols)
        frame = chain["final"][1]
        assert M.is_sorted(frame[0]) and frame[0].valid.all() and fm.rows_of(frame) > 100
        aggs = [("WindowStart", 0), ("Count", 1), ("ArithmeticMean", 1), ("Count", 2), ("ArithmeticMean", 2)]
        interval = 3 if seed % 2 else 7
        ocols = [orc.Column(fm.vals(c), M.pack(c.valid), {fm.INT64: orc.INT64, fm.FLOAT64: orc.FLOAT64}[c.typ]) for c in frame]
        want, _ = orc.aggregate(ocols, 0, interval, aggs)
        got, _ = capi.rolling_aggregate(cols, 0, interval, aggs, out_residency=capi.DEVICE)
        for a, g, w in zip(aggs, got, want):
            compare("rolling seed %d %s col %d" % (seed, a[0], a[1]), g, w)
    finally:
        release(pinned)
