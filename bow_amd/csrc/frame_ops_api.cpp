// frame_ops_api.cpp — C-ABI entry points of Bow.DropNils (reference bow.go:188-224), Bow.Diff (bowdiff.go:8-73) and Bow.Distinct
// (bowgetters.go:333-358): bowgpu_valid_mask, bowgpu_drop_nils, bowgpu_diff, bowgpu_distinct.  Host code validates, prepares
// residency and puts the kernels of frame_ops.hip in front of the scan and the scatter of Bow.Filter and the argsort and the gather of
// Bow.SortByCol; no bit is tested, no value subtracted or compared and no row moved on the CPU.
#include <string.h>

#include <memory>
#include <vector>

#include "common.h"

using namespace bowgpu;

namespace {

constexpr int64_t kFrameOpsMaxRows = (int64_t)1 << 31;   // rows and counts inside the kernels are 32 bits wide

// selectCols (bowfill.go:268-288) and what can be said about the frame without reading a column.  *sel: the selected columns,
// ascending, each once; *n: rows of the frame
int frame_checks(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx, std::vector<int32_t> *sel, int64_t *n) {
    if (ncols < 0 || n_idx < 0) return fail(BOWGPU_ERR_ARG, "negative column or index count");
    if ((ncols > 0 && !cols) || (n_idx > 0 && !col_idx)) return fail(BOWGPU_ERR_ARG, "null argument");
    std::vector<uint8_t> on((size_t)ncols, n_idx == 0 ? 1 : 0);
    for (int k = 0; k < n_idx; k++) {
        if (col_idx[k] < 0 || col_idx[k] > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "selectCols: colIndex '%d' out of range", col_idx[k]);
        on[(size_t)col_idx[k]] = 1;
    }
    for (int i = 0; i < ncols; i++)
        if (on[(size_t)i]) sel->push_back(i);
    *n = ncols > 0 ? cols[0].length : 0;
    BG_TRY(frame_cols_checks(cols, ncols, *n, true));
    if (*n >= kFrameOpsMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the frame has %lld rows: the device path serves fewer than 2^31 = 2147483648 rows", (long long)*n);
    return 0;
}

// valid_mask_kernel over the bitmaps of the selected columns (kValidMaskCols a launch, ANDed into the same words), then the call's
// three numbers; bracketed by the context's events; synchronises
int valid_mask_device(Ctx *c, const bowgpu_col *cols, const std::vector<int32_t> &sel, const uint8_t *and_mask, int32_t and_residency, int64_t n,
                      MaskWork *w) {
    std::vector<int32_t> with;
    for (int32_t i : sel)
        if (has_bitmap(cols[i])) with.push_back(i);
    const int nb = (int)with.size();
    std::unique_ptr<DevCol[]> dcs(new DevCol[nb > 0 ? nb : 1]);   // the bitmaps only: no value byte is staged or read
    for (int k = 0; k < nb; k++) {
        const bowgpu_col col = uncounted(cols[with[(size_t)k]]);
        BG_TRY(devcol_prepare(c, &col, &dcs[k], false, true));
    }
    ValidMaskArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    if (and_mask) {
        const void *dp;
        BG_TRY(aux_in(c, and_mask, (size_t)((n + 7) >> 3), and_residency, "mask", &dp, &w->staged_mask));
        a.and_mask = reinterpret_cast<const uint8_t *>(dp);
    }
    BG_TRY(mask_work_prepare(c, n, w, &a.t));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    int k0 = 0;
    do {
        a.ncols = nb - k0 < kValidMaskCols ? nb - k0 : kValidMaskCols;
        a.accumulate = k0 > 0;
        for (int k = 0; k < a.ncols; k++) {
            a.vbits[k] = dcs[k0 + k].vbits;
            a.vbit0[k] = dcs[k0 + k].vbit0;
            a.vwords[k] = dcs[k0 + k].vwords;
        }
        BG_TRY(launch_valid_mask(c, a));
        a.and_mask = nullptr;   // (it is in the words now)
        k0 += kValidMaskCols;
    } while (k0 < nb);
    BG_TRY(launch_filter_stats(c, a.t, (n + kFilterTileRows - 1) / kFilterTileRows));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    return mask_work_collect(c, w);   // (the staged bitmaps go back behind this synchronise)
}

// one diff launch over a prepared group and the counts of valid rows of its outputs on their way to valid[] (no synchronise)
int diff_launch(Ctx *c, const MoveGroup &g, const bowgpu_col *scols, int32_t g0, int64_t n, unsigned long long *valid) {
    DiffArgs a;
    a.cols = g.cols;
    a.n = n;
    a.float_mask = 0;
    a._pad = 0;
    for (int i = 0; i < g.cols.ncols; i++)
        if (scols[g0 + i].type == BOWGPU_FLOAT64) a.float_mask |= 1u << i;
    BG_TRY(launch_diff(c, a));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    uint64_t *d_valid;
    BG_TRY(scratch_at(c, kScrMoveCounts, &d_valid));
    for (int i = 0; i < g.cols.ncols; i++) BG_TRY(launch_popcount(c, reinterpret_cast<const uint32_t *>(g.cols.out_valid[i]), 0, n, d_valid + i));
    BG_HIP(hipMemcpyAsync(valid, d_valid, kScrMoveCounts.size, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// the column's valid rows, in row order, into *vals (the scanned mask of its own validity, then the scatter); *m of them
int compact_valid_device(Ctx *c, const DevCol &dk, MaskWork *w, DevBuf *vals, DevBuf *bits, int64_t *m) {
    TileRecords t;
    BG_TRY(valid_rows_scanned(c, dk, w, &t));
    *m = w->selected;
    if (*m == 0) return 0;
    BG_TRY(vals->alloc((size_t)*m * 8));
    BG_TRY(bits->alloc((size_t)((*m + 63) >> 6) * 8));
    FilterScatterArgs s;
    memset(&s, 0, sizeof s);
    s.cols.ncols = 1;
    s.cols.values[0] = reinterpret_cast<const uint64_t *>(dk.values);   // (every kept row is valid: the bitmap is not read again)
    s.cols.out_values[0] = vals->as<uint64_t>();
    s.cols.out_valid[0] = bits->as<unsigned long long>();
    s.n = dk.length;
    s.mask = t.mask;
    s.tile_base = t.tile_counts;
    BG_HIP(hipMemsetAsync(bits->p, 0, bits->bytes, c->stream));
    return launch_filter_scatter(c, s);
}

// keys[perm[j]] for j < m into *vals: the gather of Bow.SortByCol over one column without nulls (no synchronise)
int gather_keys_device(Ctx *c, const uint64_t *keys, int64_t m, const uint32_t *perm, DevBuf *vals, DevBuf *bits) {
    BG_TRY(vals->alloc((size_t)m * 8));
    BG_TRY(bits->alloc((size_t)((m + 63) >> 6) * 8));
    MoveCols cols = MoveCols();
    cols.ncols = 1;
    cols.values[0] = keys;
    cols.out_values[0] = vals->as<uint64_t>();
    cols.out_valid[0] = bits->as<unsigned long long>();
    GatherIdx ix;
    ix.u32 = perm;
    return gather_enqueue(c, cols, 0, m, ix, m);
}

int distinct_device(Ctx *c, const bowgpu_col *col, bowgpu_out *out, int64_t *n_distinct) {
    const int is_float = col->type == BOWGPU_FLOAT64;
    DevCol dk;
    BG_TRY(devcol_prepare(c, col, &dk, true, true));   // (counts the nulls where the caller said -1)
    if (dk.null_count >= dk.length) return 0;          // all null
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(dk.values);
    int64_t m = dk.length;
    MaskWork vw, tw;
    DevBuf cvals, cbits, gvals, gbits;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    if (dk.vbits) {
        BG_TRY(synced(c, compact_valid_device(c, dk, &vw, &cvals, &cbits, &m)));
        if (m == 0) return 0;
        keys = cvals.as<const uint64_t>();
    }
    SortWork sw;
    int32_t sorted = 0;
    // the key as the argsort sees it: the compacted values, else the column as it lies
    const int rc = synced(c, dk.vbits ? argsort_device(c, DeviceKey(keys, m, col->type), &sw, &sorted) : argsort_device(c, col, dk, &sw, &sorted));
    if (rc == BOWGPU_ERR_UNSUPPORTED)
        return fail(BOWGPU_ERR_UNSUPPORTED, "column holds a NaN among its valid rows: every NaN is a key of its own in the reference's map and Less "
                                            "is no order there (the caller keeps the reference path)");
    BG_TRY(rc);
    if (!sorted) {
        BG_TRY(synced(c, gather_keys_device(c, keys, m, sw.perm(), &gvals, &gbits)));
        keys = gvals.as<const uint64_t>();
    }
    TileRecords t;
    BG_TRY(synced(c, mask_work_prepare(c, m, &tw, &t)));
    BG_TRY(synced(c, launch_distinct_tail(c, keys, m, is_float, t)));
    BG_TRY(synced(c, launch_filter_stats(c, t, (m + kFilterTileRows - 1) / kFilterTileRows)));
    BG_TRY(mask_work_collect(c, &tw));
    const int64_t nd = tw.selected;
    if (out->length < nd) return fail(BOWGPU_ERR_ARG, "output column has %lld slots, %lld needed", (long long)out->length, (long long)nd);
    if (!out->values || !out->validity) return fail(BOWGPU_ERR_ARG, "output column lacks a values or validity buffer");
    const bowgpu_col sc = device_col(keys, m, col->type);
    BG_TRY(synced(c, scatter_device(c, &sc, 1, m, &tw, out)));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (out->residency == BOWGPU_DEVICE) device_write_epoch_bump();
    kernel_done(c, "filter_scatter_kernel");
    *n_distinct = nd;
    return 0;
}

}  // namespace

namespace bowgpu {

int valid_rows_scanned(Ctx *c, const DevCol &dk, MaskWork *w, TileRecords *t) {
    const int64_t n = dk.length, ntiles = (n + kFilterTileRows - 1) / kFilterTileRows;
    ValidMaskArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    a.ncols = 1;
    a.vbits[0] = dk.vbits;
    a.vbit0[0] = dk.vbit0;
    a.vwords[0] = dk.vwords;
    BG_TRY(mask_work_prepare(c, n, w, &a.t));
    BG_TRY(launch_valid_mask(c, a));
    BG_TRY(launch_filter_stats(c, a.t, ntiles));
    BG_TRY(mask_work_collect(c, w));
    *t = a.t;
    if (w->selected == 0) return 0;   // (the counts are all 0 and so is their scan: nothing is left running behind the synchronise)
    BG_TRY(w->sums.alloc((size_t)((ntiles + 4095) / 4096) * 4));
    return launch_scan_u32(c, w->tiles.as<uint32_t>(), ntiles, w->sums.as<uint32_t>());
}

}  // namespace bowgpu

extern "C" {

int bowgpu_valid_mask(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx, const uint8_t *and_mask,
                      int32_t and_mask_residency, uint8_t *mask_out, int32_t mask_residency, int64_t *selected, int64_t *first, int64_t *last) {
    if (!selected || !first || !last) return fail(BOWGPU_ERR_ARG, "null argument");
    std::vector<int32_t> sel;
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, col_idx, n_idx, &sel, &n));
    if (and_mask && !residency_ok(and_mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", and_mask_residency);
    if (mask_out && !residency_ok(mask_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", mask_residency);
    *selected = 0;
    *first = *last = -1;
    if (n == 0) return 0;
    const size_t nb = (size_t)((n + 7) >> 3);
    bool read = and_mask != nullptr;
    for (int32_t i : sel) read |= has_bitmap(cols[i]);
    if (!read && (!mask_out || mask_residency != BOWGPU_DEVICE)) {   // no bitmap to look at: every row, and the device is not needed
        if (mask_out) {
            memset(mask_out, 0xFF, nb);
            if (n & 7) mask_out[nb - 1] = (uint8_t)((1u << (n & 7)) - 1u);
        }
        *selected = n;
        *first = 0;
        *last = n - 1;
        return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    MaskWork w;
    BG_TRY(synced(c, valid_mask_device(c, cols, sel, and_mask, and_mask_residency, n, &w)));
    kernel_done(c, "valid_mask_kernel");
    if (mask_out) {
        BG_TRY(aux_out(c, mask_out, w.mask.p, nb, mask_residency));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    *selected = w.selected;
    *first = w.first;
    *last = w.last;
    return 0;
}

int bowgpu_drop_nils(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx, bowgpu_out *outs, int64_t *first,
                     int64_t *count, int32_t *contiguous) {
    if (!first || !count || !contiguous || (ncols > 0 && !outs)) return fail(BOWGPU_ERR_ARG, "null argument");
    std::vector<int32_t> sel;
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, col_idx, n_idx, &sel, &n));
    BG_TRY(outs_checks(outs, ncols, -1));
    *first = 0;
    *count = n;
    *contiguous = 1;
    bool read = false;
    for (int32_t i : sel) read |= has_bitmap(cols[i]);
    if (n == 0 || !read) return 0;   // no rows; or no bitmap to look at: the receiver itself (bow.go:210-212)
    Ctx *c;
    BG_TRY(ctx_get(&c));
    MaskWork w;
    BG_TRY(synced(c, valid_mask_device(c, cols, sel, nullptr, BOWGPU_HOST, n, &w)));
    return mask_work_compact(c, cols, ncols, n, &w, "valid_mask_kernel", outs, first, count, contiguous);
}

int bowgpu_diff(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx, bowgpu_out *outs) {
    std::vector<int32_t> sel;
    int64_t n = 0;
    BG_TRY(frame_checks(cols, ncols, col_idx, n_idx, &sel, &n));
    const int32_t nsel = (int32_t)sel.size();
    if (nsel > 0 && !outs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(outs_checks(outs, nsel, -1));
    BG_TRY(outs_checks(outs, nsel, n));
    if (n == 0) {
        for (int i = 0; i < nsel; i++) out_empty(&outs[i], cols[sel[(size_t)i]].type);
        return 0;
    }
    if (nsel == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    std::vector<bowgpu_col> scols;
    for (int32_t i : sel) scols.push_back(uncounted(cols[i]));
    const bool device_out = any_device_out(outs, nsel);
    StagedCols none_staged;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    for (int g0 = 0; g0 < nsel; g0 += kMoveCols) {
        MoveGroup g;
        BG_TRY(move_group_prepare(c, scols.data(), nsel, g0, none_staged, outs, n, &g));
        unsigned long long valid[kMoveCols] = {};
        BG_TRY(synced(c, diff_launch(c, g, scols.data(), g0, n, valid)));
        const int64_t none[kMoveCols] = {};
        BG_TRY(move_group_finish(c, &g, scols.data(), g0, n, none));
        for (int i = 0; i < g.cols.ncols; i++) outs[g0 + i].null_count = n - (int64_t)valid[i];
    }
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "diff_kernel");
    return 0;
}

int bowgpu_distinct(const bowgpu_col *col, bowgpu_out *out, int64_t *n_distinct) {
    if (!col || !out || !n_distinct) return fail(BOWGPU_ERR_ARG, "null argument");
    if (!movable_type(col->type)) return fail(BOWGPU_ERR_UNSUPPORTED, "column is of unsupported type (Int64 / Float64 only)");
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (!residency_ok(col->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col->residency);
    if (col->length >= kFrameOpsMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the column has %lld rows: the device path serves fewer than 2^31 = 2147483648 rows", (long long)col->length);
    BG_TRY(outs_checks(out, 1, -1));
    *n_distinct = 0;
    if (col->length == 0) return 0;
    const int64_t nulls = host_count_nulls(col);
    if (nulls >= col->length) return 0;   // all null, known without the device
    Ctx *c;
    BG_TRY(ctx_get(&c));
    return distinct_device(c, col, out, n_distinct);
}

}  // extern "C"
