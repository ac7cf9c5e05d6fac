// filter_api.cpp — C-ABI entry points of Bow.Filter (reference bowsetters.go:58-132): bowgpu_filter_mask, bowgpu_compact, bowgpu_filter.
// Host code validates, prepares residency and orchestrates the kernels of filter.hip; no value is compared and no row is moved on the
// CPU.
#include <stdio.h>
#include <string.h>

#include "common.h"

using namespace bowgpu;

namespace {

constexpr int64_t kFilterMaxRows = (int64_t)1 << 31;   // rows and counts inside the kernels are 32 bits wide

// everything that can be said about the frame and the predicates without reading a column; *n: rows of the frame
int frame_checks(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds, int64_t *n) {
    if (ncols < 0 || npreds < 0) return fail(BOWGPU_ERR_ARG, "negative column or predicate count");
    if ((ncols > 0 && !cols) || (npreds > 0 && !preds)) return fail(BOWGPU_ERR_ARG, "null argument");
    if (npreds > BOWGPU_FILTER_MAX_PREDS)
        return fail(BOWGPU_ERR_UNSUPPORTED, "%d comparators: the device filter serves at most BOWGPU_FILTER_MAX_PREDS = %d", npreds, BOWGPU_FILTER_MAX_PREDS);
    *n = ncols > 0 ? cols[0].length : 0;
    BG_TRY(frame_cols_checks(cols, ncols, *n, true));
    for (int p = 0; p < npreds; p++) {
        if (preds[p].col < 0 || preds[p].col > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d'", preds[p].col);
        if (preds[p].n_values < 0) return fail(BOWGPU_ERR_ARG, "negative value count");
        if (preds[p].n_values > BOWGPU_FILTER_MAX_VALUES)
            return fail(BOWGPU_ERR_UNSUPPORTED, "%d values in one comparator: the device filter serves at most BOWGPU_FILTER_MAX_VALUES = %d",
                        preds[p].n_values, BOWGPU_FILTER_MAX_VALUES);
        if (preds[p].n_values > 0 && !preds[p].values) return fail(BOWGPU_ERR_ARG, "null argument");
    }
    if (*n >= kFilterMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the frame has %lld rows: the device filter serves fewer than 2^31 = 2147483648 rows", (long long)*n);
    return 0;
}

// the predicate pass (bracketed by the context's events) and its three numbers; synchronises
int mask_device(Ctx *c, const bowgpu_col *cols, const bowgpu_filter_pred *preds, int32_t npreds, const uint8_t *and_mask, int32_t and_residency,
                int64_t n, MaskWork *w) {
    FilterMaskArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    a.npreds = npreds;
    if (and_mask) {
        const void *dp;
        BG_TRY(aux_in(c, and_mask, (size_t)((n + 7) >> 3), and_residency, "mask", &dp, &w->staged_mask));
        a.and_mask = reinterpret_cast<const uint8_t *>(dp);
    }
    for (int p = 0; p < npreds; p++) {
        const int32_t col = preds[p].col;
        StagedCols &pc = w->pcols;
        const DevCol *dc = pc.find(col);
        if (!dc) {
            DevCol *fresh = pc.add(col);
            BG_TRY(devcol_prepare(c, &cols[col], fresh, true, true));
            dc = fresh;
        }
        FilterPredDev &P = a.preds[p];
        P.values = reinterpret_cast<const uint64_t *>(dc->values);
        P.vbits = dc->vbits;
        P.vbit0 = dc->vbit0;
        P.n_values = preds[p].n_values;
        P.match_null = preds[p].match_null != 0;
        P.is_float = cols[col].type == BOWGPU_FLOAT64;
        if (P.n_values > 0) memcpy(P.set, preds[p].values, (size_t)P.n_values * 8);
    }
    BG_TRY(mask_work_prepare(c, n, w, &a.t));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(launch_filter_mask(c, a));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    return mask_work_collect(c, w);
}

// one scatter launch over a prepared group, and the counts of valid rows of its nullable columns on their way to valid[] (no synchronise)
int scatter_launch(Ctx *c, const MoveGroup &g, int64_t n, const MaskWork &w, unsigned long long *valid) {
    const int64_t count = w.selected;
    FilterScatterArgs a;
    a.cols = g.cols;
    a.n = n;
    a.mask = w.mask.as<const unsigned long long>();
    a.tile_base = w.tiles.as<const uint32_t>();
    for (int i = 0; i < g.cols.ncols; i++) BG_HIP(hipMemsetAsync(g.cols.out_valid[i], 0, (size_t)((count + 63) >> 6) * 8, c->stream));
    BG_TRY(launch_filter_scatter(c, a));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    // null_count = rows - set bits of the finished bitmap (an input column without nulls has none to count)
    uint64_t *d_valid;
    BG_TRY(scratch_at(c, kScrMoveCounts, &d_valid));
    bool counted = false;
    for (int i = 0; i < g.cols.ncols; i++) {
        if (!g.cols.vbits[i]) continue;
        BG_TRY(launch_popcount(c, reinterpret_cast<const uint32_t *>(g.cols.out_valid[i]), 0, count, d_valid + i));
        counted = true;
    }
    if (counted) BG_HIP(hipMemcpyAsync(valid, d_valid, kScrMoveCounts.size, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

}  // namespace

namespace bowgpu {

int mask_work_prepare(Ctx *c, int64_t n, MaskWork *w, TileRecords *t) {
    const int64_t ntiles = (n + kFilterTileRows - 1) / kFilterTileRows;
    BG_TRY(scratch_at(c, kScrFlags, &t->stats));
    BG_TRY(registered_at(c, kRegFilterStats, &t->host_stats));   // filter_stats_kernel stores the three numbers there itself
    BG_TRY(w->mask.alloc((size_t)ntiles * (kFilterTileRows / 8)));
    BG_TRY(w->tiles.alloc((size_t)ntiles * 4));
    BG_TRY(w->spans.alloc((size_t)ntiles * 4));
    t->mask = w->mask.as<unsigned long long>();
    t->tile_counts = w->tiles.as<uint32_t>();
    t->tile_spans = w->spans.as<uint32_t>();
    w->back = t->host_stats;
    BG_HIP(hipMemsetAsync(t->stats, 0, kScrFlags.size, c->stream));
    return 0;
}

int mask_work_collect(Ctx *c, MaskWork *w) {
    BG_HIP(hipStreamSynchronize(c->stream));
    const volatile uint32_t *back = w->back;
    w->selected = back[0];
    w->first = back[0] ? (int64_t)back[1] : -1;
    w->last = back[0] ? (int64_t)back[2] : -1;
    return 0;
}

// outs[i] = the selected rows of cols[i], for every column of the frame (the caller has checked the capacities)
int scatter_device(Ctx *c, const bowgpu_col *cols, int32_t ncols, int64_t n, MaskWork *w, bowgpu_out *outs) {
    const int64_t ntiles = (n + kFilterTileRows - 1) / kFilterTileRows, count = w->selected;
    BG_TRY(w->sums.alloc((size_t)((ntiles + 4095) / 4096) * 4));
    // the context's events: from the scan to the last scatter launch.  For a frame of up to kMoveCols device-resident columns that is
    // the scan, the memsets and the scatter kernel; with more groups or host-resident columns their staging and copies fall inside
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(launch_scan_u32(c, w->tiles.as<uint32_t>(), ntiles, w->sums.as<uint32_t>()));
    for (int g0 = 0; g0 < ncols; g0 += kMoveCols) {
        MoveGroup g;
        BG_TRY(move_group_prepare(c, cols, ncols, g0, w->pcols, outs, count, &g));
        unsigned long long valid[kMoveCols] = {};
        BG_TRY(synced(c, scatter_launch(c, g, n, *w, valid)));
        // the copies of the finished columns are queued behind the counts: one synchronise for the group, the null counts filled in after it
        const int64_t none[kMoveCols] = {};
        BG_TRY(move_group_finish(c, &g, cols, g0, count, none));
        for (int i = 0; i < g.cols.ncols; i++)
            if (g.cols.vbits[i]) outs[g0 + i].null_count = count - (int64_t)valid[i];
    }
    return 0;
}

// what follows the mask pass of a call that moves rows: the contiguous answer, or the capacity check, the scan and the scatter
int mask_work_compact(Ctx *c, const bowgpu_col *cols, int32_t ncols, int64_t n, MaskWork *w, const char *mask_kernel, bowgpu_out *outs,
                      int64_t *first, int64_t *count, int32_t *contiguous) {
    *count = w->selected;
    *first = w->selected ? w->first : 0;
    *contiguous = w->selected == 0 || w->selected == w->last - w->first + 1;
    if (*contiguous) {   // bowsetters.go:74-82: the empty slice, or a slice of the receiver
        kernel_done(c, mask_kernel);
        return 0;
    }
    for (int i = 0; i < ncols; i++)
        if (outs[i].length < w->selected)
            return fail(BOWGPU_ERR_ARG, "output column %d has %lld slots, %lld needed", i, (long long)outs[i].length, (long long)w->selected);
    const bool device_out = any_device_out(outs, ncols);
    BG_TRY(synced(c, scatter_device(c, cols, ncols, n, w, outs)));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "filter_scatter_kernel");
    return 0;
}

}  // namespace bowgpu

namespace {

// bowgpu_filter and bowgpu_compact after their argument checks
int filter_run(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds, const uint8_t *and_mask,
               int32_t and_residency, int64_t n, bowgpu_out *outs, int64_t *first, int64_t *count, int32_t *contiguous) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    MaskWork w;
    BG_TRY(synced(c, mask_device(c, cols, preds, npreds, and_mask, and_residency, n, &w)));
    return mask_work_compact(c, cols, ncols, n, &w, "filter_mask_kernel", outs, first, count, contiguous);
}

}  // namespace

extern "C" {

int bowgpu_filter_mask(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds, const uint8_t *and_mask,
                       int32_t and_mask_residency, uint8_t *mask_out, int32_t mask_residency, int64_t *selected, int64_t *first, int64_t *last) {
    if (!selected || !first || !last) return fail(BOWGPU_ERR_ARG, "null argument");
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, preds, npreds, &n));
    if (and_mask && !residency_ok(and_mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", and_mask_residency);
    if (!residency_ok(mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", mask_residency);
    *selected = 0;
    *first = *last = -1;
    if (n == 0) return 0;
    if (!mask_out) return fail(BOWGPU_ERR_ARG, "null argument");
    const size_t nb = (size_t)((n + 7) >> 3);
    if (npreds == 0 && !and_mask && mask_residency != BOWGPU_DEVICE) {   // the empty filter into host memory: every row
        memset(mask_out, 0xFF, nb);
        if (n & 7) mask_out[nb - 1] = (uint8_t)((1u << (n & 7)) - 1u);
        *selected = n;
        *first = 0;
        *last = n - 1;
        return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    MaskWork w;
    BG_TRY(synced(c, mask_device(c, cols, preds, npreds, and_mask, and_mask_residency, n, &w)));
    kernel_done(c, "filter_mask_kernel");
    BG_TRY(aux_out(c, mask_out, w.mask.p, nb, mask_residency));
    BG_HIP(hipStreamSynchronize(c->stream));
    *selected = w.selected;
    *first = w.first;
    *last = w.last;
    return 0;
}

int bowgpu_compact(const bowgpu_col *cols, int32_t ncols, const uint8_t *mask, int32_t mask_residency, bowgpu_out *outs, int64_t *first,
                   int64_t *count, int32_t *contiguous) {
    if (!first || !count || !contiguous || (ncols > 0 && !outs)) return fail(BOWGPU_ERR_ARG, "null argument");
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, nullptr, 0, &n));
    if (!residency_ok(mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", mask_residency);
    BG_TRY(outs_checks(outs, ncols, -1));
    *first = 0;
    *count = 0;
    *contiguous = 1;
    if (n == 0) return 0;
    if (!mask) return fail(BOWGPU_ERR_ARG, "null argument");
    return filter_run(cols, ncols, nullptr, 0, mask, mask_residency, n, outs, first, count, contiguous);
}

int bowgpu_filter(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds, const uint8_t *and_mask,
                  int32_t and_mask_residency, bowgpu_out *outs, int64_t *first, int64_t *count, int32_t *contiguous) {
    if (!first || !count || !contiguous || (ncols > 0 && !outs)) return fail(BOWGPU_ERR_ARG, "null argument");
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, preds, npreds, &n));
    if (and_mask && !residency_ok(and_mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", and_mask_residency);
    BG_TRY(outs_checks(outs, ncols, -1));
    *first = 0;
    *count = n;
    *contiguous = 1;
    if (n == 0 || (npreds == 0 && !and_mask)) return 0;   // no rows; or the empty filter: the receiver itself
    return filter_run(cols, ncols, preds, npreds, and_mask, and_mask_residency, n, outs, first, count, contiguous);
}

}  // extern "C"
