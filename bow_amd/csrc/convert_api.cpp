// convert_api.cpp — C-ABI entry point of Bow.Convert (reference bowsetters.go:52-56; Type.Convert, bowtypes.go:64-81; bowconvert.go)
// among Int64, Float64 and Boolean: bowgpu_convert.  Host code validates, stages the columns of a group through dev_cols.cpp - 8-byte
// values by devcol_prepare, a Boolean column's bits by devboolcol_prepare, outputs by devout_prepare / devout_finish - and launches
// convert_kernel of convert.hip once per group of kMoveCols columns; no value is converted and no bit is moved on the CPU.  The
// columns need not be a frame (lengths may differ), so the group driver is this file's own and frame_cols.cpp's move_group_*, whose
// contract is Int64 / Float64 columns of one length, stays as it is.
#include <string.h>

#include "common.h"

using namespace bowgpu;

namespace {

bool convertible_type(int32_t t) { return t == BOWGPU_INT64 || t == BOWGPU_FLOAT64 || t == BOWGPU_BOOLEAN; }

int type_check(int32_t t, int i, const char *what) {
    if (t == BOWGPU_STRING)
        return fail(BOWGPU_ERR_UNSUPPORTED, "column %d: %s type String is not served by the device path (the reference's Convert loop is)", i, what);
    if (!convertible_type(t)) return fail(BOWGPU_ERR_ARG, "column %d: unknown %s type %d", i, what, t);
    return 0;
}

// everything that can be said without a device, in the order it is reported
int convert_checks(const bowgpu_col *cols, const int32_t *to_types, int32_t ncols, const bowgpu_out *outs) {
    for (int i = 0; i < ncols; i++) {
        const bowgpu_col &col = cols[i];
        const bowgpu_out &out = outs[i];
        BG_TRY(type_check(col.type, i, "source"));
        BG_TRY(type_check(to_types[i], i, "target"));
        if (col.length < 0 || col.offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (!residency_ok(col.residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col.residency);
        if (!residency_ok(out.residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", out.residency);
        if (out.length < col.length)
            return fail(BOWGPU_ERR_ARG, "output column has %lld slots, %lld needed", (long long)out.length, (long long)col.length);
        if (col.length > 0 && !col.values) return fail(BOWGPU_ERR_ARG, "column has no values buffer");
        if (col.length > 0 && (!out.values || !out.validity)) return fail(BOWGPU_ERR_ARG, "output column lacks a values or validity buffer");
    }
    return 0;
}

// the staged inputs and output temporaries of one launch: they go back when the group does, behind its synchronise
struct ConvertGroup {
    DevCol wide[kMoveCols];
    DevBoolCol bits[kMoveCols];
    DevOut douts[kMoveCols];
};

// columns [g0, g0 + m) of the call: staged, converted by one launch, handed back; the group's one synchronise
int convert_group(Ctx *c, const bowgpu_col *cols, const int32_t *to_types, int32_t g0, int m, bowgpu_out *outs, ConvertGroup *g) {
    ConvertArgs a;
    memset(&a, 0, sizeof a);
    a.ncols = m;
    for (int i = 0; i < m; i++) {
        const bowgpu_col col = uncounted(cols[g0 + i]);   // (the kernel counts the valid rows in its own pass)
        ConvertCol &q = a.col[i];
        q.n = col.length;
        q.from = col.type;
        q.to = to_types[g0 + i];
        if (q.n > a.max_n) a.max_n = q.n;
        if (q.n == 0) continue;
        if (col.type == BOWGPU_BOOLEAN) {
            BG_TRY(devboolcol_prepare(c, &col, &g->bits[i]));
            q.src = g->bits[i].t.words;
            q.sbit0 = g->bits[i].t.bit0;
            q.swords = g->bits[i].t.nwords;
            q.vbits = g->bits[i].v.words;
            q.vbit0 = g->bits[i].v.bit0;
            q.vwords = g->bits[i].v.nwords;
        } else {
            BG_TRY(devcol_prepare(c, &col, &g->wide[i], true, true));
            q.src = g->wide[i].values;
            q.vbits = g->wide[i].vbits;
            q.vbit0 = g->wide[i].vbit0;
            q.vwords = g->wide[i].vwords;
        }
        BG_TRY(devout_prepare(c, &outs[g0 + i], q.n, &g->douts[i], -1, q.to == BOWGPU_BOOLEAN));
        q.out_values = g->douts[i].values;
        q.out_valid = reinterpret_cast<unsigned long long *>(g->douts[i].validity);
    }
    BG_TRY(scratch_at(c, kScrConvertCounts, &a.valid_counts));
    unsigned long long valid[kMoveCols][kConvertShards];
    static_assert(sizeof valid == kScrConvertCounts.size, "a count per column and shard");
    BG_HIP(hipMemsetAsync(a.valid_counts, 0, sizeof valid, c->stream));
    BG_TRY(launch_convert(c, a));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipMemcpyAsync(valid, a.valid_counts, sizeof valid, hipMemcpyDeviceToHost, c->stream));
    for (int i = 0; i < m; i++) {
        if (a.col[i].n == 0) out_empty(&outs[g0 + i], a.col[i].to);
        else BG_TRY(devout_finish(c, &g->douts[i], a.col[i].n, a.col[i].to, 0));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; i++) {
        int64_t set = 0;
        for (int k = 0; k < kConvertShards; k++) set += (int64_t)valid[i][k];
        outs[g0 + i].null_count = a.col[i].n - set;
    }
    return 0;
}

}  // namespace

extern "C" {

int bowgpu_convert(const bowgpu_col *cols, const int32_t *to_types, int32_t ncols, bowgpu_out *outs) {
    if (ncols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if (ncols == 0) return 0;
    if (!cols || !to_types || !outs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(convert_checks(cols, to_types, ncols, outs));
    bool rows = false;
    for (int i = 0; i < ncols; i++) rows |= cols[i].length > 0;
    if (!rows) {   // empty outputs of the target types, and the device is not needed
        for (int i = 0; i < ncols; i++) out_empty(&outs[i], to_types[i]);
        return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    for (int g0 = 0; g0 < ncols; g0 += kMoveCols) {
        ConvertGroup g;
        BG_TRY(synced(c, convert_group(c, cols, to_types, g0, ncols - g0 < kMoveCols ? ncols - g0 : kMoveCols, outs, &g)));
    }
    if (any_device_out(outs, ncols)) device_write_epoch_bump();
    kernel_done(c, "convert_kernel");
    return 0;
}

}  // extern "C"
