// sort_api.cpp — C-ABI entry points of Bow.SortByCol (reference bowsort.go:10-41): bowgpu_argsort, bowgpu_take, bowgpu_sort_by_col.
// Host code validates (mirroring the reference's driver), prepares residency and orchestrates the kernels of sort.hip; no key is
// compared and no row is moved on the CPU.
#include <stdio.h>
#include <string.h>

#include "common.h"

using namespace bowgpu;

namespace {

constexpr int64_t kSortMaxRows = (int64_t)1 << 31;   // row indices inside the sort are 32 bits wide

thread_local char g_kernel_name[64];

int key_checks(const bowgpu_col *key) {
    if (!movable_type(key->type)) return fail(BOWGPU_ERR_TYPE, "column to sort by is of unsupported type (Int64 / Float64 only)");
    if (key->length < 0 || key->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    const int64_t nulls = host_count_nulls(key);
    if (nulls > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %d nil values", (int)nulls);
    if (key->length >= kSortMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "column to sort by has %lld rows: the device sort serves fewer than 2^31 = 2147483648 rows",
                    (long long)key->length);
    return 0;
}

}  // namespace

namespace bowgpu {

// Histogram + checks, then the passes.  *sorted = 1: the key is in order (sort.IsSorted) and nothing else was done.
// The caller brackets the call with the context's events and synchronises.
int argsort_device(Ctx *c, const bowgpu_col *key, const DevCol &dk, SortWork *w, int32_t *sorted) {
    const int64_t n = dk.length;
    const int is_float = key->type == BOWGPU_FLOAT64;
    uint32_t *d_hist, *d_flags;   // (the flags lie right behind the histogram: one memset and one copy for both)
    BG_TRY(scratch_at(c, kScrHist, &d_hist));
    BG_TRY(scratch_at(c, kScrFlags, &d_flags));
    const uint64_t *raw = reinterpret_cast<const uint64_t *>(dk.values);
    // a key read in place over the host link leaves its images in HBM during that one read
    const bool in_place_host = key->residency == BOWGPU_HOST_PINNED && !dk.own_values.p;
    if (in_place_host) BG_TRY(w->keys[1].alloc((size_t)n * 8));
    BG_HIP(hipMemsetAsync(d_hist, 0, span(kScrHist, kScrFlags), c->stream));
    BG_TRY(launch_sort_hist(c, raw, n, is_float, d_hist, d_flags, in_place_host ? w->keys[1].as<uint64_t>() : nullptr));
    uint32_t back[8 * 256 + 4];
    static_assert(sizeof back == span(kScrHist, kScrFlags), "histogram and flags");
    BG_HIP(hipMemcpyAsync(back, d_hist, sizeof back, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    const uint32_t *flags = back + 8 * 256;
    if (flags[1]) return fail(BOWGPU_ERR_UNSUPPORTED, "column to sort by holds a NaN: Less is not an order there (the caller keeps the reference path)");
    *sorted = flags[0] ? 0 : 1;
    if (*sorted) return 0;
    bool active[8];
    for (int p = 0; p < 8; p++) {
        int bins = 0;
        for (int d = 0; d < 256; d++) bins += back[256 * p + d] != 0;
        active[p] = bins > 1;
    }
    const int64_t ntiles = (n + kSortTileRows - 1) / kSortTileRows;
    const int64_t m = 256 * ntiles;
    for (int b = 0; b < 2; b++) {
        if (!w->keys[b].p) BG_TRY(w->keys[b].alloc((size_t)n * 8));
        BG_TRY(w->idx[b].alloc((size_t)n * 4));
    }
    BG_TRY(w->tiles.alloc((size_t)m * 4));
    BG_TRY(w->sums.alloc((size_t)((m + 4095) / 4096) * 4));
    const uint64_t *src = in_place_host ? w->keys[1].as<const uint64_t>() : raw;
    int mode = in_place_host ? 2 : is_float;
    const uint32_t *src_idx = nullptr;
    int dst = in_place_host ? 0 : 1;
    for (int p = 0; p < 8; p++) {
        if (!active[p]) continue;
        BG_TRY(launch_sort_pass(c, src, mode, src_idx, n, 8 * p, w->tiles.as<uint32_t>(), w->sums.as<uint32_t>(), w->keys[dst].as<uint64_t>(),
                                w->idx[dst].as<uint32_t>()));
        src = w->keys[dst].as<const uint64_t>();
        src_idx = w->idx[dst].as<const uint32_t>();
        mode = 2;
        w->cur = dst;
        dst ^= 1;
        w->passes++;
    }
    return 0;
}

// ---------------------------------------------------------------- the gather's host side
int gather_enqueue(Ctx *c, const MoveCols &cols, int32_t g0, int64_t length, const GatherIdx &ix, int64_t n_idx) {
    GatherNoRowArgs a;
    memset(&a, 0, sizeof a);
    a.cols = cols;
    a.n_idx = n_idx;
    a.length = length;
    uint32_t *flags;
    BG_TRY(scratch_at(c, kScrFlags, &flags));
    BG_TRY(scratch_at(c, kScrMoveCounts, &a.null_counts));
    a.bad = flags + 2;
    a.key_slot = ix.key_col >= g0 && ix.key_col < g0 + kMoveCols ? ix.key_col - g0 : -1;
    if (a.key_slot >= 0) {
        a.idx2 = ix.i32_2;
        a.values2 = reinterpret_cast<const uint64_t *>(ix.key2->values);
        a.vbits2 = ix.key2->vbits;
        a.vbit02 = ix.key2->vbit0;
    }
    BG_HIP(hipMemsetAsync(flags, 0, span(kScrFlags, kScrMoveCounts), c->stream));
    BG_TRY(launch_gather(c, a, ix));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    return 0;
}

int gather_launch(Ctx *c, const MoveGroup &g, int32_t g0, int64_t length, const GatherIdx &ix, int64_t n_idx, int64_t *nulls, bool *bad) {
    BG_TRY(gather_enqueue(c, g.cols, g0, length, ix, n_idx));
    struct { uint32_t flags[4]; unsigned long long nulls[kMoveCols]; } back;
    static_assert(sizeof back == span(kScrFlags, kScrMoveCounts), "flags and counts");
    const uint32_t *flags;
    BG_TRY(scratch_at(c, kScrFlags, &flags));
    BG_HIP(hipMemcpyAsync(&back, flags, sizeof back, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    *bad = back.flags[2] != 0;
    for (int i = 0; i < kMoveCols; i++) nulls[i] = (int64_t)back.nulls[i];
    return 0;
}

int gather_frame(Ctx *c, const bowgpu_col *cols, int32_t ncols, const StagedCols &have, const GatherIdx &ix, int64_t n_idx, bowgpu_out *outs,
                 bool *bad) {
    *bad = false;
    for (int g0 = 0; g0 < ncols; g0 += kMoveCols) {
        MoveGroup g;
        BG_TRY(move_group_prepare(c, cols, ncols, g0, have, outs, n_idx, &g));
        int64_t nulls[kMoveCols];
        BG_TRY(synced(c, gather_launch(c, g, g0, cols[g0].length, ix, n_idx, nulls, bad)));
        if (*bad) return 0;
        BG_TRY(move_group_finish(c, &g, cols, g0, n_idx, nulls));
    }
    return 0;
}

}  // namespace bowgpu

namespace {

// (a key whose nulls were counted on the host - none - goes without its bitmap: nothing is staged or counted a second time)
int key_prepare(Ctx *c, const bowgpu_col *key, DevCol *dk) {
    bowgpu_col k = *key;
    if (host_count_nulls(key) == 0) { k.validity = nullptr; k.null_count = 0; }
    return devcol_prepare(c, &k, dk, true, true);
}

// what last_kernel_ms of an argsort / a frame sort is reported under
const char *passes_name(int passes) {
    snprintf(g_kernel_name, sizeof g_kernel_name, "sort_scatter_kernel<%d of 8 passes>", passes);
    return g_kernel_name;
}

}  // namespace

extern "C" {

int bowgpu_argsort(const bowgpu_col *key, int64_t *perm, int32_t perm_residency, int32_t *sorted) {
    if (!key || !sorted) return fail(BOWGPU_ERR_ARG, "null argument");
    if (!residency_ok(perm_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", perm_residency);
    BG_TRY(key_checks(key));
    const int64_t n = key->length;
    *sorted = 1;
    if (n < 2) return 0;   // sort.IsSorted of 0 or 1 rows
    if (!perm) return fail(BOWGPU_ERR_ARG, "null argument");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dk;
    BG_TRY(key_prepare(c, key, &dk));
    if (dk.null_count > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %d nil values", (int)dk.null_count);
    SortWork w;
    DevBuf wide;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, argsort_device(c, key, dk, &w, sorted)));
    if (!*sorted) {
        int64_t *d_perm = perm;
        if (perm_residency != BOWGPU_DEVICE) {
            BG_TRY(wide.alloc((size_t)n * 8));
            d_perm = wide.as<int64_t>();
        }
        BG_TRY(launch_widen(c, w.perm(), nullptr, n, d_perm));
        BG_HIP(hipEventRecord(c->ev1, c->stream));
        BG_TRY(aux_out(c, perm, d_perm, (size_t)n * 8, perm_residency));
    } else {
        BG_HIP(hipEventRecord(c->ev1, c->stream));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    kernel_done(c, passes_name(w.passes));
    return 0;
}

int bowgpu_take(const bowgpu_col *col, const int64_t *idx, int64_t n_idx, int32_t idx_residency, bowgpu_out *out) {
    if (!col || !out || (!idx && n_idx > 0)) return fail(BOWGPU_ERR_ARG, "null argument");
    if (n_idx < 0) return fail(BOWGPU_ERR_ARG, "negative index count");
    if (!residency_ok(idx_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", idx_residency);
    if (!movable_type(col->type)) return fail(BOWGPU_ERR_UNSUPPORTED, "column is of unsupported type (Int64 / Float64 only)");
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    BG_TRY(outs_checks(out, 1, n_idx));
    if (n_idx == 0) {
        out_empty(out, col->type);
        return 0;
    }
    if (col->length == 0) return fail(BOWGPU_ERR_ARG, "index out of range: the column has no rows");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    StagedCols have;   // a frame of one column, staged here
    BG_TRY(devcol_prepare(c, col, have.add(0), true, true));
    const void *d_idx;
    DevBuf staged;
    BG_TRY(aux_in(c, idx, (size_t)n_idx * 8, idx_residency, "index", &d_idx, &staged));
    if (reinterpret_cast<uintptr_t>(d_idx) & 7) return fail(BOWGPU_ERR_ARG, "index buffer must be 8-byte aligned");
    GatherIdx ix;
    ix.i64 = reinterpret_cast<const int64_t *>(d_idx);
    bool bad = false;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(gather_frame(c, col, 1, have, ix, n_idx, out, &bad));
    if (bad) return fail(BOWGPU_ERR_ARG, "index out of range [0, %lld)", (long long)col->length);
    if (out->residency == BOWGPU_DEVICE) device_write_epoch_bump();
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    kernel_done(c, "gather_kernel");
    return 0;
}

int bowgpu_sort_by_col(const bowgpu_col *cols, int32_t ncols, int32_t key_col, bowgpu_out *outs, int32_t *unchanged) {
    // reference bowsort.go:10-41
    if (!cols || !outs || !unchanged) return fail(BOWGPU_ERR_ARG, "null argument");
    if (key_col < 0 || key_col > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d'", key_col);
    const bowgpu_col *key = &cols[key_col];
    if (!movable_type(key->type)) return fail(BOWGPU_ERR_TYPE, "column to sort by is of unsupported type (Int64 / Float64 only)");
    const int64_t n = key->length;
    BG_TRY(frame_cols_checks(cols, ncols, n, false));
    BG_TRY(key_checks(key));
    BG_TRY(outs_checks(outs, ncols, n));
    *unchanged = 1;
    if (n < 2) return 0;   // sort.IsSorted of 0 or 1 rows: the reference returns the receiver
    Ctx *c;
    BG_TRY(ctx_get(&c));
    StagedCols have;   // the key: sorted here, moved with its group
    DevCol &dk = *have.add(key_col);
    BG_TRY(key_prepare(c, key, &dk));
    if (dk.null_count > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %d nil values", (int)dk.null_count);
    SortWork w;
    int32_t sorted = 0;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, argsort_device(c, key, dk, &w, &sorted)));
    if (sorted) {
        BG_HIP(hipEventRecord(c->ev1, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
        kernel_done(c, passes_name(0));
        return 0;
    }
    *unchanged = 0;
    const bool device_out = any_device_out(outs, ncols);
    GatherIdx ix;
    ix.u32 = w.perm();
    bool bad = false;
    BG_TRY(gather_frame(c, cols, ncols, have, ix, n, outs, &bad));
    if (bad) return fail(BOWGPU_ERR_HIP, "internal: the sort produced a row index outside the frame");   // (nothing of that group was handed out)
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (device_out) device_write_epoch_bump();
    kernel_done(c, passes_name(w.passes));
    return 0;
}

}  // extern "C"
