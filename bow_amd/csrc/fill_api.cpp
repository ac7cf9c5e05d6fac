// fill_api.cpp - Bow.IsColSorted, Bow.FillLinear and Bow.FillPrevious / FillNext / FillMean (reference bowassertion.go, bowfill.go):
// validation in the reference's order, residency, and the kernels of interp_fill.hip; no value is filled on the CPU.
#include <string.h>

#include "common.h"

using namespace bowgpu;

extern "C" {

static int col_order_flags(Ctx *c, const DevCol &dc, int32_t type, uint32_t *flags) {
    uint32_t *dflags;
    BG_TRY(scratch_at(c, kScrOrderFlags, &dflags));
    BG_TRY(launch_col_order(c, reinterpret_cast<const uint64_t *>(dc.values), dc.vbits, dc.vbit0, dc.length, type, dflags));
    BG_HIP(hipMemcpyAsync(flags, dflags, 4, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int bowgpu_is_col_sorted(const bowgpu_col *col, int32_t *sorted) {
    // reference bowassertion.go:15-81: empty column or unsupported type => false
    if (!col || !sorted) return fail(BOWGPU_ERR_ARG, "null argument");
    *sorted = 0;
    if (col->type != BOWGPU_INT64 && col->type != BOWGPU_FLOAT64) return 0;
    if (col->length == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dc;
    BG_TRY(devcol_prepare(c, col, &dc, true, true));
    uint32_t f = 0;
    BG_TRY(col_order_flags(c, dc, col->type, &f));
    *sorted = (f & 4) && !((f & 1) && (f & 2));
    return 0;
}

static int fill_finish(Ctx *c, FillParams &P, int64_t n, const DevCol &dfill, DevOut *dout, int type);

static int fill_linear_impl(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col, bowgpu_out *out, int32_t *unchanged,
                            bool ref_checked);
int bowgpu_fill_linear(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col, bowgpu_out *out, int32_t *unchanged) {
    return fill_linear_impl(cols, ncols, ref_col, fill_col, out, unchanged, false);
}
int bowgpu_fill_linear_sorted(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col, bowgpu_out *out, int32_t *unchanged) {
    return fill_linear_impl(cols, ncols, ref_col, fill_col, out, unchanged, true);
}
static int fill_linear_impl(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col, bowgpu_out *out, int32_t *unchanged,
                            bool ref_checked) {
    // reference bowfill.go:14-103
    if (!cols || !out || !unchanged) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ref_col < 0 || ref_col > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "refColIndex is out of range");
    if (fill_col < 0 || fill_col > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "toFillColIndex is out of range");
    if (ref_col == fill_col) return fail(BOWGPU_ERR_ARG, "refColIndex and toFillColIndex are equal");
    const int rt = cols[ref_col].type, ft = cols[fill_col].type;
    if (rt != BOWGPU_INT64 && rt != BOWGPU_FLOAT64) return fail(BOWGPU_ERR_TYPE, "refColIndex '%d' is of type '%s'", ref_col, arrow_type_name(rt));
    const int64_t n = cols[fill_col].length;
    if (cols[ref_col].length != n) return fail(BOWGPU_ERR_ARG, "columns differ in length");
    *unchanged = 0;
    if (ft != BOWGPU_INT64 && ft != BOWGPU_FLOAT64) {
        // the reference checks the fill column's type after the ref column's emptiness / order (bowfill.go:35-51)
        return fail(BOWGPU_ERR_UNSUPPORTED, "toFillColIndex '%d' is of unsupported type '%s'", fill_col, arrow_type_name(ft));
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dref, dfill;
    BG_TRY(devcol_prepare(c, &cols[ref_col], &dref, true, true));
    BG_TRY(devcol_prepare(c, &cols[fill_col], &dfill, true, true));
    DevOut dout;
    BG_TRY(devout_prepare(c, out, n, &dout, 0));
    // (ref_checked: the caller's own bowfill.go:35-42 - the ref column holds a value and IsColSorted - has run; the pass over the ref
    // column that establishes both, a quarter of the call at 1e8 rows, is not made a second time)
    uint32_t f = ref_checked ? 4u : 0u;
    if (n > 0 && !ref_checked) BG_TRY(col_order_flags(c, dref, rt, &f));
    const bool ref_empty = !(f & 4);                                  // IsColEmpty: bowassertion.go:84-86
    const bool ref_sorted = (f & 4) && !((f & 1) && (f & 2));
    if (!ref_empty && !ref_sorted) return fail(BOWGPU_ERR_NOT_SORTED, "refColIndex '%d' is empty or not sorted", ref_col);
    const bool nothing = ref_empty || dfill.null_count == 0;          // bowfill.go:35-37, :53-55 return the receiver
    *unchanged = nothing ? 1 : 0;
    FillParams P;
    memset(&P, 0, sizeof P);
    P.ref_values = reinterpret_cast<const uint64_t *>(dref.values); P.ref_vbits = dref.vbits; P.ref_vbit0 = dref.vbit0; P.ref_type = rt;
    P.fill_values = reinterpret_cast<const uint64_t *>(dfill.values); P.fill_vbits = dfill.vbits; P.fill_vbit0 = dfill.vbit0; P.fill_type = ft;
    P.method = kFillLinear;
    // (no special casing is needed for the two "return the receiver" cases: without nulls every row is copied,
    //  and with an all-null reference column no null row passes the valid1 test of bowfill.go:74)
    return fill_finish(c, P, n, dfill, &dout, ft);
}

// shared tail of the fill entry points: the kernel, the count of valid outputs, copy-back.
// The neighbour index of the fill column's bitmap (three small launches, ~25 us at 1e8 rows) is built only for a REPEAT: the kernel
// finds the valid row beyond a trip's ends by a bounded walk (2048 rows) and says so when a run of nulls is longer - the usual column
// never needs the index (Interpolate does the same since round 5).  A device-resident output bitmap that can take the kernel's whole
// 64-bit words - 8-byte aligned, capacity to the end of the word holding row n - 1 - is written in place: no copy behind the kernel.
static int fill_finish(Ctx *c, FillParams &P, int64_t n, const DevCol &dfill, DevOut *dout, int type) {
    BG_TRY(scratch_at(c, kScrFillFar, &P.far_flag));
    BG_TRY(scratch_at(c, kScrFillCount, &P.valid_count));
    P.n = n;
    P.out_values = reinterpret_cast<uint64_t *>(dout->values);
    // the kernel stores one whole 64-bit validity word per wavefront trip: ceil(n/64)*8 bytes, which the word-aligned working
    // copy of devout_prepare (temp_bits_bytes(ceil(n/8))) always holds
    const bowgpu_out *u = dout->user;
    const bool place = n > 0 && u->residency == BOWGPU_DEVICE && (reinterpret_cast<uintptr_t>(u->validity) & 7) == 0 &&
                       ((u->length + 7) >> 3) >= 8 * ((n + 63) >> 6);   // (u->length: still the capacity the caller handed in)
    P.out_valid_words = reinterpret_cast<uint32_t *>(place ? u->validity : dout->validity);
    memset(&P.nbr, 0, sizeof P.nbr);
    struct { uint32_t far, pad; uint64_t cnt; } back = {0, 0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        if (attempt == 1) {
            void *ix;
            BG_TRY(ctx_pool(c, kPoolInterp + 3, nbr_index_bytes(n, dfill.vbit0), &ix));
            BG_TRY(nbr_index_build(c, dfill.vbits, dfill.vbit0, n, ix, &P.nbr));
        }
        BG_HIP(hipMemsetAsync(P.far_flag, 0, span(kScrFillFar, kScrFillCount), c->stream));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        BG_TRY(fill_run(c, P));
        BG_HIP(hipEventRecord(c->ev1, c->stream));
        BG_HIP(hipMemcpyAsync(&back, P.far_flag, sizeof back, hipMemcpyDeviceToHost, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
        if (!back.far) break;
    }
    {   // (bowgpu_last_kernel_ms / _name: the fill kernel of this call)
        float ms = 0;
        BG_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->last_kernel_ms = ms;
        c->last_kernel_name = "fill_kernel";
    }
    BG_TRY(devout_finish(c, dout, n, type, n - (int64_t)back.cnt, !place));
    if (!place) BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int bowgpu_fill(const bowgpu_col *col, int32_t method, bowgpu_out *out, int32_t *unchanged) {
    // reference bowfill.go:105-160 (FillMean), :162-253 (FillNext / FillPrevious)
    if (!col || !out || !unchanged) return fail(BOWGPU_ERR_ARG, "null argument");
    if (method != BOWGPU_FILL_PREVIOUS && method != BOWGPU_FILL_NEXT && method != BOWGPU_FILL_MEAN) return fail(BOWGPU_ERR_ARG, "unknown fill method %d", method);
    const int ft = col->type;
    if (ft != BOWGPU_INT64 && ft != BOWGPU_FLOAT64)  // FillMean's own error (bowfill.go:119-122); Previous/Next on Boolean/String: declined
        return fail(BOWGPU_ERR_UNSUPPORTED, "column is of unsupported type '%s'", arrow_type_name(ft));
    const int64_t n = col->length;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dfill;
    BG_TRY(devcol_prepare(c, col, &dfill, true, true));
    DevOut dout;
    BG_TRY(devout_prepare(c, out, n, &dout, 0));
    *unchanged = dfill.null_count == 0 ? 1 : 0;
    FillParams P;
    memset(&P, 0, sizeof P);
    P.fill_values = reinterpret_cast<const uint64_t *>(dfill.values); P.fill_vbits = dfill.vbits; P.fill_vbit0 = dfill.vbit0; P.fill_type = ft;
    P.method = method;
    return fill_finish(c, P, n, dfill, &dout, ft);
}

}  // extern "C"
