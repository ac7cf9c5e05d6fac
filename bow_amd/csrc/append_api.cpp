// append_api.cpp — C-ABI entry points of AppendBows (reference bowappend.go:11-103) and Bow.Find / FindNext / Contains
// (bowfind.go:3-32): bowgpu_append, bowgpu_find_next.  Host code validates, prepares residency, builds the piece table and launches the
// kernels of append.hip; no value is copied or compared and no validity bit is moved on the CPU.
#include <string.h>

#include <cmath>
#include <vector>

#include "common.h"

using namespace bowgpu;

namespace {

constexpr int64_t kAppendMaxRows = (int64_t)1 << 31;   // rows inside the kernels are 32 bits wide
constexpr int32_t kAppendMaxPieces = 1 << 18;          // the piece table of a launch group: 100 bytes a piece

// everything that can be said about the pieces without reading a column; *total: rows of the result
int pieces_checks(const bowgpu_col *const *frames, int32_t nframes, int32_t ncols, int64_t *total) {
    if (nframes < 1) return fail(BOWGPU_ERR_ARG, "no frame to append (%d)", nframes);
    if (ncols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if (!frames) return fail(BOWGPU_ERR_ARG, "null argument");
    if (nframes > kAppendMaxPieces)
        return fail(BOWGPU_ERR_UNSUPPORTED, "%d frames: the device append serves at most 2^18 = %d in one call", nframes, kAppendMaxPieces);
    *total = 0;
    for (int32_t f = 0; f < nframes; f++) {
        if (ncols > 0 && !frames[f]) return fail(BOWGPU_ERR_ARG, "null argument");
        const int64_t n = ncols > 0 ? frames[f][0].length : 0;
        BG_TRY(frame_cols_checks(frames[f], ncols, n, true));
        for (int i = 0; i < ncols; i++)
            if (frames[f][i].type != frames[0][i].type)   // bowappend.go:40-42
                return fail(BOWGPU_ERR_TYPE, "incompatible types '%s' and '%s'", arrow_type_name(frames[0][i].type), arrow_type_name(frames[f][i].type));
        *total += n;
        if (*total >= kAppendMaxRows)
            return fail(BOWGPU_ERR_UNSUPPORTED, "the frames have %lld rows and more: the device path serves fewer than 2^31 = 2147483648 rows",
                        (long long)*total);
    }
    return 0;
}

}  // namespace

namespace bowgpu {

// one group of up to kMoveCols columns: every piece staged, the table built and uploaded, one append launch, the counts of valid rows
// of the columns whose nulls the arguments do not state on their way to valid[] (no synchronise)
int append_launch(Ctx *c, const bowgpu_col *const *frames, int32_t nframes, int32_t g0, int64_t total, const MoveGroup &g,
                  std::vector<DevCol> *staged, PieceTable *t, const bool *count_on_device, unsigned long long *valid) {
    const int gc = g.cols.ncols;
    AppendArgs a;
    memset(&a, 0, sizeof a);
    a.cols = g.cols;
    a.n = total;
    a.npieces = nframes;
    uint32_t *starts = t->starts();
    int64_t start = 0;
    for (int32_t f = 0; f < nframes; f++) {
        starts[f] = (uint32_t)start;
        const int64_t n = frames[f][g0].length;
        for (int i = 0; i < gc && n > 0; i++) {
            DevCol dc;
            const bowgpu_col col = uncounted(frames[f][g0 + i]);
            BG_TRY(devcol_prepare(c, &col, &dc, true, true));
            AppendPiece &p = t->pieces(i)[f];
            p.values = reinterpret_cast<const uint64_t *>(reinterpret_cast<uintptr_t>(dc.values) - (uintptr_t)start * 8);
            p.vbits = dc.vbits;
            p.vadj = dc.vbits ? dc.vbit0 - start : 0;
            if (dc.vbits) a.bitmap_mask |= 1u << i;
            if (dc.own_values.p || dc.own_validity.p) staged->push_back(std::move(dc));   // a staged copy: kept until the group is done
        }
        start += n;
    }
    starts[nframes] = (uint32_t)start;
    void *dt;
    BG_TRY(ctx_pool(c, kPoolAppend, t->bytes.size(), &dt));
    BG_TRY(copy_h2d(c, dt, t->bytes.data(), t->pieces_offset(gc)));   // (the arrays of the group's columns)
    a.starts = reinterpret_cast<const uint32_t *>(dt);
    for (int i = 0; i < gc; i++) a.pieces[i] = reinterpret_cast<const AppendPiece *>(reinterpret_cast<char *>(dt) + t->pieces_offset(i));
    BG_TRY(launch_append(c, a));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    uint64_t *d_valid;
    BG_TRY(scratch_at(c, kScrMoveCounts, &d_valid));
    bool counted = false;
    for (int i = 0; i < gc; i++) {
        if (!count_on_device[i]) continue;
        BG_TRY(launch_popcount(c, reinterpret_cast<const uint32_t *>(g.cols.out_valid[i]), 0, total, d_valid + i));
        counted = true;
    }
    if (counted) BG_HIP(hipMemcpyAsync(valid, d_valid, kScrMoveCounts.size, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

}  // namespace bowgpu

extern "C" {

int bowgpu_append(const bowgpu_col *const *frames, int32_t nframes, int32_t ncols, bowgpu_out *outs, int32_t *unchanged) {
    if (!unchanged || (ncols > 0 && !outs)) return fail(BOWGPU_ERR_ARG, "null argument");
    int64_t total = 0;
    BG_TRY(pieces_checks(frames, nframes, ncols, &total));
    BG_TRY(outs_checks(outs, ncols, -1));
    *unchanged = 0;
    if (nframes == 1) {   // bowappend.go:19-21 returns its argument
        *unchanged = 1;
        return 0;
    }
    if (total == 0) {
        for (int i = 0; i < ncols; i++) out_empty(&outs[i], frames[0][i].type);
        return 0;
    }
    BG_TRY(outs_checks(outs, ncols, total));
    if (ncols == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    const bool device_out = any_device_out(outs, ncols);
    PieceTable table(nframes);
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    for (int g0 = 0; g0 < ncols; g0 += kMoveCols) {
        // the nulls of a column: the sum of what its pieces state (host-resident bitmaps are counted here); else its finished bitmap is counted
        int64_t nulls[kMoveCols] = {};
        bool count_on_device[kMoveCols] = {};
        const int gc = ncols - g0 < kMoveCols ? ncols - g0 : kMoveCols;
        for (int i = 0; i < gc; i++)
            for (int32_t f = 0; f < nframes && !count_on_device[i]; f++) {
                const int64_t k = host_count_nulls(&frames[f][g0 + i]);
                if (k < 0) count_on_device[i] = true;
                else nulls[i] += k;
            }
        std::vector<DevCol> staged;   // the copies of BOWGPU_HOST pieces (they go back behind the group's synchronise)
        MoveGroup g;
        g.cols = MoveCols();
        BG_TRY(move_group_outputs(c, ncols, g0, outs, total, &g));
        unsigned long long valid[kMoveCols] = {};
        BG_TRY(synced(c, append_launch(c, frames, nframes, g0, total, g, &staged, &table, count_on_device, valid)));
        BG_TRY(move_group_finish(c, &g, frames[0], g0, total, nulls));
        for (int i = 0; i < gc; i++)
            if (count_on_device[i]) outs[g0 + i].null_count = total - (int64_t)valid[i];
    }
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "append_kernel");
    return 0;
}

int bowgpu_find_next(const bowgpu_col *col, int64_t row_start, const void *value, int64_t *row) {
    if (!col || !row) return fail(BOWGPU_ERR_ARG, "null argument");
    if (!movable_type(col->type)) return fail(BOWGPU_ERR_UNSUPPORTED, "column is of unsupported type (Int64 / Float64 only)");
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (!residency_ok(col->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col->residency);
    if (col->length >= kAppendMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the column has %lld rows: the device path serves fewer than 2^31 = 2147483648 rows", (long long)col->length);
    if (row_start < 0) return fail(BOWGPU_ERR_ARG, "negative row index %lld", (long long)row_start);
    *row = -1;
    if (col->length == 0) return 0;
    FindArgs a;
    memset(&a, 0, sizeof a);
    if (!value) {   // nil: the first null row, counted from row 0 whatever row_start says (bowfind.go:12-19)
        if (!has_bitmap(*col)) return 0;
    } else {
        if (row_start >= col->length) return 0;
        memcpy(&a.value, value, 8);
        a.is_float = col->type == BOWGPU_FLOAT64;
        double d;
        memcpy(&d, value, 8);
        if (a.is_float && std::isnan(d)) return 0;   // a NaN equals nothing
        a.row_start = row_start;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dc;
    const bowgpu_col k = uncounted(*col);
    BG_TRY(synced(c, devcol_prepare(c, &k, &dc, value != nullptr, true)));
    if (!value && !dc.vbits) return 0;
    a.values = value ? reinterpret_cast<const uint64_t *>(dc.values) : nullptr;
    a.vbits = dc.vbits;
    a.vbit0 = dc.vbit0;
    a.vwords = dc.vwords;
    a.n = col->length;
    BG_TRY(synced(c, scratch_at(c, kScrFlags, &a.result)));
    BG_TRY(synced(c, registered_at(c, kRegFindRow, &a.host_result)));   // the kernel stores the row there itself
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, launch_find(c, a)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    const uint32_t found = *const_cast<const volatile uint32_t *>(a.host_result);
    if (found != kFindNone) *row = (int64_t)found;
    kernel_done(c, value ? "find_kernel" : "find_null_kernel");
    return 0;
}

}  // extern "C"
