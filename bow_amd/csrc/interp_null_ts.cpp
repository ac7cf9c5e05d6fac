// interp_null_ts.cpp - Rolling.Interpolate over an interval column WITH NULLS: the kept rows compacted, the ordinary count and fill
// (interpolate_api.cpp) on them, the copies of null-timestamp rows patched afterwards; what a count builds is kept for its fill.
#include <string.h>

#include <algorithm>
#include <vector>

#include "interp_host.h"

namespace bowgpu {

// What bowgpu_rolling_interpolate_count builds for an interval column with nulls and the bowgpu_rolling_interpolate_fill that follows
// it needs again: the kept rows compacted (one 8-byte column and one bitmap per column of the Bow, the marker column, the flags) and the
// compacted call's descriptors.  Kept per thread between the two calls, keyed like the count -> fill prefix of the ordinary path
// (Ctx::InterpCache): DEVICE-resident columns, the same pointers / offsets / lengths / null counts / interpolators / options, nothing
// written to or freed from device memory through the library in between (device_write_epoch) - include/bowgpu.h states the contract
// for the ordinary path, this is the same one.  Dropped by the fill that uses it, by any other Interpolate of the thread over an interval
// column with nulls, by bowgpu_trim, bowgpu_set_device and at thread exit (round 5 ran the whole compaction twice: ADVICE r04).
namespace {
struct NullTsState {
    std::vector<bowgpu_col> key_cols;
    std::vector<bowgpu_interp> key_interps;
    int32_t ts_col = 0;
    int64_t interval = 0;
    bowgpu_options o = {0, 0, 0};
    uint64_t epoch = 0;
    DevBuf flags, marker, marker_bits, ts_bits;
    std::vector<DevBuf> cvals, cbits;
    CompactCols cc;
    std::vector<bowgpu_col> cols2;
    std::vector<bowgpu_interp> interps2;
    int64_t m = 0, m_out = 0;
};
void null_ts_state_free(void *p) { delete reinterpret_cast<NullTsState *>(p); }
void null_ts_cache_drop(Ctx *c) {
    if (c->null_ts_cache) { void *p = c->null_ts_cache; c->null_ts_cache = nullptr; null_ts_state_free(p); }
}
bool null_ts_cache_hit(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options &o,
                       const bowgpu_interp *interps, int32_t ninterps) {
    const NullTsState *st = reinterpret_cast<const NullTsState *>(c->null_ts_cache);
    if (!st || st->ts_col != ts_col || st->interval != interval || (int32_t)st->key_cols.size() != ncols || (int32_t)st->key_interps.size() != ninterps) return false;
    if (st->o.offset != o.offset || st->o.inclusive != o.inclusive || st->o.strict_order != o.strict_order) return false;
    if (st->epoch != device_write_epoch()) return false;
    for (int i = 0; i < ncols; i++) {
        const bowgpu_col &a = st->key_cols[i], &b = cols[i];
        if (b.residency != BOWGPU_DEVICE || a.values != b.values || a.validity != b.validity || a.offset != b.offset || a.length != b.length ||
            a.null_count != b.null_count || a.type != b.type) return false;
    }
    return memcmp(st->key_interps.data(), interps, sizeof(bowgpu_interp) * (size_t)ninterps) == 0;
}
}  // namespace

// The build step: the keep-bitmap of the rows that belong to a window, its scan, the kept rows compacted, and the compacted call's
// descriptors and row count - all into S.  *nothing: the result has no rows (S is then not complete)
static int null_ts_build(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options &o,
                         const bowgpu_interp *interps, int32_t ninterps, const Plan &plan, const DevCol &dts, NullTsState &S, bool *nothing) {
    const bowgpu_col *tsc = &cols[ts_col];
    const int64_t n = tsc->length;
    const int incl = o.inclusive ? 1 : 0;
    *nothing = true;
    int last_valid = 1;
    BG_TRY(fetch_valid(c, tsc, n - 1, &last_valid));
    if (!last_valid || plan.W == 0) return 0;      // HasNext (rolling.go:162-173) is false from the start: no window, no rows
    // the rows that belong to a window, compacted
    DevBuf ixbuf, ts_eff, keep, plain_ts, dropped, counts, base, sums;
    NbrIndex ix;
    BG_TRY(ixbuf.alloc(nbr_index_bytes(n, dts.vbit0)));
    BG_TRY(nbr_index_build(c, dts.vbits, dts.vbit0, n, ixbuf.p, &ix));
    BG_TRY(ts_eff.alloc((size_t)n * 8 + 16));
    const int64_t nw = (n + 63) >> 6;
    BG_TRY(keep.alloc((size_t)nw * 8 + 8));
    BG_TRY(dropped.alloc(32));
    BG_HIP(hipMemsetAsync(dropped.p, 0, 32, c->stream));
    if (incl) BG_TRY(plain_ts.alloc((size_t)nw * 8 + 8));
    // (inclusive iteration: mode 2 - the rows on a window start with a null timestamp behind them stay, ts_nulls.hip; slot 1 of `dropped`
    // counts the two shapes of them this path cannot express)
    BG_TRY(launch_ts_nullfill(c, reinterpret_cast<const int64_t *>(dts.values), dts.vbits, dts.vbit0, n, ix, plan.s0, plan.interval, plan.magic, incl ? 2 : 0,
                              reinterpret_cast<int64_t *>(ts_eff.p), reinterpret_cast<uint64_t *>(keep.p), reinterpret_cast<uint64_t *>(plain_ts.p),
                              reinterpret_cast<unsigned long long *>(dropped.p)));
    if (incl) {
        unsigned long long h_out = 0;
        BG_HIP(hipMemcpyAsync(&h_out, reinterpret_cast<unsigned long long *>(dropped.p) + 1, 8, hipMemcpyDeviceToHost, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
        if (h_out)
            return fail(BOWGPU_ERR_TS_NULLS, "inclusive Interpolate over an interval column with nulls: %llu row(s) on a window start with null timestamps behind them are "
                        "followed by an equal timestamp or sit on -1: outside the device path", h_out);
    }
    BG_TRY(counts.alloc((size_t)nw * 4 + 16));
    BG_TRY(base.alloc((size_t)(nw + 1) * 8 + 16));
    BG_TRY(sums.alloc((size_t)((nw + 2047) / 2048 + 2) * 8));
    BG_TRY(launch_keep_counts(c, reinterpret_cast<const uint64_t *>(keep.p), nw, reinterpret_cast<int32_t *>(counts.p)));
    int64_t *d_total = reinterpret_cast<int64_t *>(dropped.p) + 2;
    BG_TRY(launch_exclusive_scan(c, reinterpret_cast<const int32_t *>(counts.p), nw, reinterpret_cast<int64_t *>(base.p), reinterpret_cast<int64_t *>(sums.p), d_total));
    int64_t m = 0;
    BG_HIP(hipMemcpyAsync(&m, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (m <= 0) return 0;
    const size_t mbm = (size_t)((m + 63) >> 6) * 8 + 8;
    std::vector<DevCol> dcs(ncols);
    CompactCols &cc = S.cc;
    S.cvals.resize(ncols); S.cbits.resize(ncols);
    memset(&cc, 0, sizeof cc);
    cc.ncols = ncols; cc.ts_col = ts_col;
    for (int i = 0; i < ncols; i++) {
        BG_TRY(S.cvals[i].alloc((size_t)m * 8 + 16));
        cc.out_values[i] = reinterpret_cast<uint64_t *>(S.cvals[i].p);
        if (i == ts_col) continue;
        BG_TRY(devcol_prepare(c, &cols[i], &dcs[i], true, true));
        cc.values[i] = reinterpret_cast<const uint64_t *>(dcs[i].values); cc.vbits[i] = dcs[i].vbits; cc.vbit0[i] = dcs[i].vbit0;
        BG_TRY(S.cbits[i].alloc(mbm));
        cc.lookup_bits[i] = reinterpret_cast<uint64_t *>(S.cbits[i].p);
    }
    BG_TRY(S.flags.alloc((size_t)m * 4 + 16));
    BG_TRY(S.marker.alloc((size_t)m * 8 + 16));
    BG_TRY(S.marker_bits.alloc(mbm));
    if (incl) { BG_TRY(S.ts_bits.alloc(mbm)); cc.ts_bits = reinterpret_cast<uint64_t *>(S.ts_bits.p); }
    BG_TRY(launch_compact_rows(c, reinterpret_cast<const uint64_t *>(keep.p), reinterpret_cast<const int64_t *>(base.p), n, reinterpret_cast<const int64_t *>(ts_eff.p),
                               dts.vbits, dts.vbit0, reinterpret_cast<const uint64_t *>(plain_ts.p), cc, reinterpret_cast<int64_t *>(S.marker.p),
                               reinterpret_cast<uint32_t *>(S.flags.p)));
    BG_TRY(launch_pack_flags(c, reinterpret_cast<const uint32_t *>(S.flags.p), m, cc, reinterpret_cast<uint64_t *>(S.marker_bits.p)));
    device_write_epoch_bump();      // (temporaries may sit where an earlier call's columns sat: no count -> fill reuse across this point)
    // the compacted call: the Bow's columns + the marker under interpolation.None
    S.cols2.assign(ncols + 1, bowgpu_col());
    S.interps2.assign(interps, interps + ninterps);
    for (int i = 0; i <= ncols; i++) {
        bowgpu_col &t = S.cols2[i];
        memset(&t, 0, sizeof t);
        t.offset = 0; t.length = m; t.residency = BOWGPU_DEVICE;
        if (i == ncols) { t.values = S.marker.p; t.validity = reinterpret_cast<const uint8_t *>(S.marker_bits.p); t.type = BOWGPU_INT64; t.null_count = -1; }
        else if (i == ts_col) { t.values = S.cvals[i].p; t.validity = nullptr; t.type = BOWGPU_INT64; t.null_count = 0; }
        else { t.values = S.cvals[i].p; t.validity = reinterpret_cast<const uint8_t *>(S.cbits[i].p); t.type = cols[i].type; t.null_count = -1; }
    }
    {
        bowgpu_interp mk;
        memset(&mk, 0, sizeof mk);
        mk.kind = BOWGPU_INTERP_NONE; mk.col = ncols;
        S.interps2.push_back(mk);
    }
    int64_t m_out = 0;
    BG_TRY(interp_count_impl(S.cols2.data(), ncols + 1, ts_col, interval, &o, S.interps2.data(), ninterps + 1, &m_out, nullptr, nullptr));
    S.m = m; S.m_out = m_out;
    *nothing = false;
    return 0;
}

// an interpolator's Options.PrevRow and constant, as PatchInterps lays them out (interpolate_api.cpp has InterpCol's form)
static void patch_interps_take(PatchInterps *px, int i, const bowgpu_interp &ip) {
    px->const_value[i] = ip.const_value;
    px->has_prev[i] = ip.has_prev_row; px->prev_t_valid[i] = ip.prev_t_valid; px->prev_v_valid[i] = ip.prev_v_valid;
    px->prev_t[i] = ip.prev_t; px->prev_v[i] = ip.prev_v; px->prev_v_i64[i] = ip.prev_v_i64;
}

// The patch step: the compacted call's outputs in tmp (the Bow's columns and the marker) corrected where they are copies of
// null-timestamp rows, recounted and handed to the caller
static int null_ts_patch(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int incl, const bowgpu_interp *interps, const NullTsState &S,
                         const DevFrame &tmp, bowgpu_out *outs) {
    const int64_t m = S.m, m_out = S.m_out;
    PatchInterps px;
    memset(&px, 0, sizeof px);
    px.m = m;
    std::vector<DevBuf> nbrbufs(ncols);
    if (incl) {
        for (int i = 0; i < ncols; i++) {
            px.both_bits[i] = i == ts_col ? reinterpret_cast<const uint64_t *>(S.ts_bits.p) : reinterpret_cast<const uint64_t *>(S.cbits[i].p);
            BG_TRY(nbrbufs[i].alloc(nbr_index_bytes(m, 0)));
            BG_TRY(nbr_index_build(c, reinterpret_cast<const uint32_t *>(px.both_bits[i]), 0, m, nbrbufs[i].p, &px.nbr[i]));
            px.type[i] = cols[i].type; px.kind[i] = interps[i].kind;
            patch_interps_take(&px, i, interps[i]);
        }
    }
    BG_TRY(launch_interp_patch(c, tmp.values[ncols].as<const int64_t>(), tmp.bits[ncols].as<const uint32_t>(), m_out,
                               reinterpret_cast<const uint32_t *>(S.flags.p), S.cc, px));
    BG_HIP(hipStreamSynchronize(c->stream));       // (nbrbufs are released at the end of this scope)
    for (int i = 0; i < ncols; i++) {
        int64_t nulls = 0;
        BG_TRY(recount_nulls(c, tmp.bits[i].p, m_out, &nulls));
        BG_TRY(temp_to_caller(c, tmp, i, m_out, cols[i].type, nulls, &outs[i], i < 16 ? i : -1));
    }
    device_write_epoch_bump();
    return 0;
}

// Rolling.Interpolate over an interval column WITH NULLS (ts_nulls.hip has the semantics and the kernels): the
// call is made on the kept rows - those inside some window's slice - compacted into device temporaries, plus a marker column that
// tells afterwards which output rows are copies of null-timestamp rows; those get their null timestamp and their values' own
// validity back; after an inclusive iteration the second copy of a row on a window start with null timestamps behind it becomes the
// synthetic start row of the window that begins behind it.  outs == nullptr: the row count only.  *applies = false: the interval
// column has no nulls.
static int interp_null_ts(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                          const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out, bowgpu_out *outs, bool *applies) {
    *applies = false;
    if (!cols || ncols <= 0 || ts_col < 0 || ts_col >= ncols) return 0;       // (the ordinary path reports these)
    const bowgpu_col *tsc = &cols[ts_col];
    if (!tsc->validity || tsc->null_count == 0 || tsc->length == 0) return 0;
    const bowgpu_options o = options_or(opts);
    Plan plan;
    BG_TRY(plan_make(nullptr, tsc, interval, o.offset, &plan));                // ctor errors first (rolling.go:69-112)
    BG_TRY(interp_validate(cols, ncols, ts_col, &o, interps, ninterps));
    Ctx *c;
    BG_TRY(ctx_get(&c));
    // the _fill right behind its _count: the compaction is there (NullTsState above)
    const bool reuse = outs && null_ts_cache_hit(c, cols, ncols, ts_col, interval, o, interps, ninterps);
    if (!reuse) null_ts_cache_drop(c);
    DevCol dts;
    if (!reuse) {
        BG_TRY(devcol_prepare(c, tsc, &dts, true, true));
        if (dts.null_count <= 0) return 0;
    }
    *applies = true;
    const int64_t n = tsc->length;
    if (ncols > kMaxCompactCols) return fail(BOWGPU_ERR_UNSUPPORTED, "Interpolate over an interval column with nulls: at most %d columns", kMaxCompactCols);
    for (int i = 0; i < ncols; i++)
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "column %d has a different length", i);
    auto nothing = [&]() -> int {
        if (n_out) *n_out = 0;
        if (outs) outs_empty(outs, ninterps, [&](int i) { return cols[i].type; });
        return 0;
    };
    // (the state of this call: a fresh one, or the one the count left; a fresh one is kept for the fill only when the count succeeded on
    // DEVICE-resident columns)
    struct StateOwner { NullTsState *p = nullptr; bool keep = false; ~StateOwner() { if (p && !keep) delete p; } } owner;
    if (reuse) { owner.p = reinterpret_cast<NullTsState *>(c->null_ts_cache); c->null_ts_cache = nullptr; }   // (one use: this fill owns it now)
    else owner.p = new NullTsState();
    NullTsState &S = *owner.p;
    if (!reuse) {
        bool empty = false;
        BG_TRY(null_ts_build(c, cols, ncols, ts_col, interval, o, interps, ninterps, plan, dts, S, &empty));
        if (empty) return nothing();
    }
    if (n_out) *n_out = S.m_out;
    if (!outs) {
        // the count alone: what it built stays for the fill that follows (DEVICE-resident columns: the contract of the ordinary path) -
        // the compacted call's own count -> fill prefix (c->interp_cache) with it, its interval column lives in the kept state
        bool all_device = true;
        for (int i = 0; i < ncols; i++) all_device = all_device && cols[i].residency == BOWGPU_DEVICE;
        if (all_device && S.m_out > 0) {
            S.key_cols.assign(cols, cols + ncols); S.key_interps.assign(interps, interps + ninterps);
            S.ts_col = ts_col; S.interval = interval; S.o = o; S.epoch = device_write_epoch();
            BG_HIP(hipStreamSynchronize(c->stream));
            c->null_ts_cache = owner.p; c->null_ts_cache_free = null_ts_state_free;
            owner.keep = true;
        } else c->interp_cache.valid = false;
        return 0;
    }
    if (S.m_out == 0) return nothing();
    DevFrame tmp;   // the compacted call's outputs: the Bow's columns and the marker
    BG_TRY(tmp.alloc(c, ncols + 1, S.m_out, true));
    for (int i = 0; i < ncols; i++) { S.cc.patch_values[i] = tmp.values[i].as<uint64_t>(); S.cc.patch_valid[i] = tmp.bits[i].as<uint32_t>(); }
    BG_TRY(interp_fill_impl(S.cols2.data(), ncols + 1, ts_col, interval, &o, S.interps2.data(), ninterps + 1, tmp.outs.data(), nullptr, nullptr));
    c->interp_cache.valid = false;
    if (tmp.outs[0].length != S.m_out) return fail(BOWGPU_ERR_ARG, "internal: Interpolate over an interval column with nulls produced %lld rows, counted %lld", (long long)tmp.outs[0].length, (long long)S.m_out);
    return null_ts_patch(c, cols, ncols, ts_col, o.inclusive ? 1 : 0, interps, S, tmp, outs);
}

// ... for Bows wider than the compaction's 16 columns (round 6; BOWGPU_ERR_UNSUPPORTED before): the value columns in groups of 15, each
// group with the interval column in front as a frame of its own.  A column's output depends on the interval column and on itself only
// (the interpolators look at one column each: interpolation.go:139-155), so the groups' outputs side by side are the call's; the row count
// comes from the first group, the interval column's output is written by every group (the same bytes).  Errors are the whole frame's:
// it is validated before anything runs.
int interp_null_ts_any(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                              const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out, bowgpu_out *outs, bool *applies) {
    *applies = false;
    if (!cols || ncols <= kMaxCompactCols || ts_col < 0 || ts_col >= ncols || !interps || ninterps != ncols)
        return interp_null_ts(cols, ncols, ts_col, interval, opts, interps, ninterps, n_out, outs, applies);
    const bowgpu_col *tsc = &cols[ts_col];
    if (!tsc->validity || tsc->null_count == 0 || tsc->length == 0) return 0;
    const bowgpu_options o = options_or(opts);
    Plan plan;
    BG_TRY(plan_make(nullptr, tsc, interval, o.offset, &plan));
    BG_TRY(interp_validate(cols, ncols, ts_col, &o, interps, ninterps));
    for (int i = 0; i < ncols; i++) if (interps[i].col != i) return interp_null_ts(cols, ncols, ts_col, interval, opts, interps, ninterps, n_out, outs, applies);
    std::vector<int> values;
    for (int i = 0; i < ncols; i++) if (i != ts_col) values.push_back(i);
    bool first = true;
    for (size_t at = 0; at < values.size(); at += kMaxCompactCols - 1) {
        const size_t m = std::min<size_t>(kMaxCompactCols - 1, values.size() - at);
        std::vector<bowgpu_col> sc(m + 1);
        std::vector<bowgpu_interp> si(m + 1);
        std::vector<bowgpu_out> so(m + 1);
        sc[0] = cols[ts_col]; si[0] = interps[ts_col]; si[0].col = 0;
        if (outs) so[0] = outs[ts_col];
        for (size_t k = 0; k < m; k++) {
            sc[k + 1] = cols[values[at + k]];
            si[k + 1] = interps[values[at + k]]; si[k + 1].col = (int32_t)k + 1;
            if (outs) so[k + 1] = outs[values[at + k]];
        }
        bool ap = false;
        int64_t cnt = 0;
        BG_TRY(interp_null_ts(sc.data(), (int32_t)m + 1, 0, interval, opts, si.data(), (int32_t)m + 1, (n_out && first) ? &cnt : nullptr, outs ? so.data() : nullptr, &ap));
        if (!ap) return 0;   // (the interval column turned out to have no nulls: the ordinary path takes the call)
        *applies = true;
        if (n_out && first) *n_out = cnt;
        if (outs) {
            outs[ts_col] = so[0];
            for (size_t k = 0; k < m; k++) outs[values[at + k]] = so[k + 1];
        }
        first = false;
        if (!outs) break;   // (the count: one group tells it)
    }
    return 0;
}

}  // namespace bowgpu
