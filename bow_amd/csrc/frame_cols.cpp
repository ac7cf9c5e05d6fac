// frame_cols.cpp — the host layer under the frame-level operations (the *_api.cpp files of Sort, Filter, DropNils / Diff / Distinct,
// Append / Find and Join): argument checks of a frame and its output columns, a caller's side buffers in and out, and the staging of
// the columns of a frame, kMoveCols a launch, around the kernel that moves their rows; and what the calls that keep a frame in
// device temporaries between two steps share (DevFrame, stage_rows, temp_to_caller).  No kernel of its own: recount_nulls goes
// through the library's popcount.
#include <string.h>

#include "common.h"

namespace bowgpu {

bool movable_type(int32_t t) { return t == BOWGPU_INT64 || t == BOWGPU_FLOAT64; }
bool residency_ok(int32_t r) { return r == BOWGPU_HOST || r == BOWGPU_DEVICE || r == BOWGPU_HOST_PINNED; }

int64_t host_count_nulls(const bowgpu_col *col) {
    if (!col->validity || col->null_count == 0 || col->length <= 0) return 0;
    if (col->null_count > 0) return col->null_count;
    if (col->residency == BOWGPU_DEVICE) return -1;
    int64_t set = 0;
    for (int64_t i = 0; i < col->length; i++) {
        const int64_t bit = col->offset + i;
        set += (col->validity[bit >> 3] >> (bit & 7)) & 1;
    }
    return col->length - set;
}

int frame_cols_checks(const bowgpu_col *cols, int32_t ncols, int64_t n, bool residencies) {
    for (int i = 0; i < ncols; i++) {
        if (residencies && (cols[i].length < 0 || cols[i].offset < 0)) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        if (cols[i].offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (!movable_type(cols[i].type)) return fail(BOWGPU_ERR_UNSUPPORTED, "column %d is of unsupported type (Int64 / Float64 only)", i);
        if (residencies && !residency_ok(cols[i].residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", cols[i].residency);
    }
    return 0;
}

int outs_checks(const bowgpu_out *outs, int32_t ncols, int64_t slots) {
    for (int i = 0; i < ncols; i++) {
        const bowgpu_out &o = outs[i];
        if (slots < 0) {
            if (!residency_ok(o.residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", o.residency);
            if (o.length < 0) return fail(BOWGPU_ERR_ARG, "output column %d has a negative capacity", i);
        } else if (o.length < slots) {
            return fail(BOWGPU_ERR_ARG, "output column has %lld slots, %lld needed", (long long)o.length, (long long)slots);
        }
        if ((slots < 0 ? o.length : slots) > 0 && (!o.values || !o.validity)) return fail(BOWGPU_ERR_ARG, "output column lacks a values or validity buffer");
    }
    return 0;
}

bowgpu_col device_col(const void *values, int64_t n, int32_t type) {
    bowgpu_col k;
    memset(&k, 0, sizeof k);
    k.values = values;
    k.length = n;
    k.type = type;
    k.residency = BOWGPU_DEVICE;
    return k;
}

DeviceKey::DeviceKey(const void *values, int64_t n, int32_t type) : col(device_col(values, n, type)) {
    dev.values = values;
    dev.length = n;
    dev.type = type;
}

bool any_device_out(const bowgpu_out *outs, int32_t n) {
    bool device_out = false;
    for (int i = 0; i < n; i++) device_out |= outs[i].residency == BOWGPU_DEVICE;
    return device_out;
}

void out_empty(bowgpu_out *out, int32_t type) {
    out->length = 0;
    out->null_count = 0;
    out->type = type;
}

int aux_in(Ctx *c, const void *p, size_t bytes, int32_t residency, const char *what, const void **dptr, DevBuf *own) {
    *dptr = p;
    if (residency == BOWGPU_HOST_PINNED) {
        if (!(*dptr = host_mapped(p, what))) return BOWGPU_ERR_ARG;
    } else if (residency == BOWGPU_HOST) {
        BG_TRY(own->alloc(bytes));
        BG_TRY(copy_h2d(c, own->p, p, bytes));
        *dptr = own->p;
    }
    return 0;
}

int aux_out(Ctx *c, void *dst, const void *src, size_t bytes, int32_t residency) {
    if (residency != BOWGPU_DEVICE) return copy_d2h(c, dst, src, bytes, residency == BOWGPU_HOST_PINNED);
    if (dst != src) BG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    device_write_epoch_bump();
    return 0;
}

void kernel_done(Ctx *c, const char *name) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) (void)hipGetLastError();
    c->last_kernel_ms = ms;
    c->last_kernel_name = name;
}

int synced(Ctx *c, int rc) {
    if (rc != 0) (void)hipStreamSynchronize(c->stream);
    return rc;
}

bool has_bitmap(const bowgpu_col &col) { return col.validity != nullptr && col.null_count != 0; }

bowgpu_col uncounted(const bowgpu_col &col) {
    bowgpu_col k = col;
    if (k.validity && k.null_count < 0) k.null_count = 1;
    return k;
}

int move_group_prepare(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t g0, const StagedCols &have, bowgpu_out *outs, int64_t count, MoveGroup *g) {
    MoveCols &m = g->cols;
    m = MoveCols();
    m.ncols = ncols - g0 < kMoveCols ? ncols - g0 : kMoveCols;
    for (int i = 0; i < m.ncols; i++) {
        const DevCol *dc = have.find(g0 + i);
        if (!dc) {
            const int rc = devcol_prepare(c, &cols[g0 + i], &g->staged[i], true, true);
            if (rc != 0) return synced(c, rc);
            dc = &g->staged[i];
        }
        m.values[i] = reinterpret_cast<const uint64_t *>(dc->values);
        m.vbits[i] = dc->vbits;
        m.vbit0[i] = dc->vbit0;
    }
    return move_group_outputs(c, ncols, g0, outs, count, g);
}

int move_group_outputs(Ctx *c, int32_t ncols, int32_t g0, bowgpu_out *outs, int64_t count, MoveGroup *g) {
    MoveCols &m = g->cols;
    m.ncols = ncols - g0 < kMoveCols ? ncols - g0 : kMoveCols;
    for (int i = 0; i < m.ncols; i++) {
        const int rc = devout_prepare(c, &outs[g0 + i], count, &g->douts[i]);
        if (rc != 0) return synced(c, rc);
        m.out_values[i] = reinterpret_cast<uint64_t *>(g->douts[i].values);
        m.out_valid[i] = reinterpret_cast<unsigned long long *>(g->douts[i].validity);
    }
    return 0;
}

int move_group_finish(Ctx *c, MoveGroup *g, const bowgpu_col *cols, int32_t g0, int64_t count, const int64_t *null_counts) {
    for (int i = 0; i < g->cols.ncols; i++) {
        const int rc = devout_finish(c, &g->douts[i], count, cols[g0 + i].type, null_counts[i]);
        if (rc != 0) return synced(c, rc);
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int DevFrame::alloc(Ctx *c, int32_t ncols, int64_t rows, bool zero_bits) {
    values.resize(ncols); bits.resize(ncols); outs.resize(ncols);
    for (int i = 0; i < ncols; i++) {
        BG_TRY(values[i].alloc(temp_values_bytes(rows)));
        BG_TRY(bits[i].alloc(temp_bits_bytes((size_t)((rows + 7) >> 3))));
        if (zero_bits) BG_HIP(hipMemsetAsync(bits[i].p, 0, bits[i].bytes, c->stream));
        memset(&outs[i], 0, sizeof outs[i]);
        outs[i].values = values[i].p;
        outs[i].validity = bits[i].as<uint8_t>();
        outs[i].length = rows;
        outs[i].residency = BOWGPU_DEVICE;
    }
    return 0;
}

void DevFrame::as_cols(const bowgpu_col *schema, int64_t n, bowgpu_col *cols) const {
    for (size_t i = 0; i < outs.size(); i++) {
        cols[i] = device_col(outs[i].values, n, schema[i].type);
        cols[i].validity = outs[i].validity;
        cols[i].null_count = n > 0 ? outs[i].null_count : 0;
    }
}

void DevFrame::clear() {
    values.clear(); bits.clear();
    for (bowgpu_out &o : outs) { o.values = nullptr; o.validity = nullptr; }
}

// bytes of a source column into a buffer of the destination's device, on the destination's stream
static int pull_bytes(Ctx *c, int dst_dev, int src_dev, void *dst, const void *src, size_t bytes, int32_t residency) {
    if (bytes == 0) return 0;
    if (residency != BOWGPU_DEVICE) return copy_h2d(c, dst, src, bytes, residency == BOWGPU_HOST_PINNED);
    if (dst_dev == src_dev) BG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    else BG_HIP(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, c->stream));
    return 0;
}

int stage_rows(Ctx *c, int dst_dev, int src_dev, const bowgpu_col &sc, int64_t a, int64_t b, DevBuf *values, DevBuf *bits, bowgpu_col *out) {
    const int64_t r0 = sc.offset + a, r1 = sc.offset + b, v0 = r0 & ~(int64_t)7;
    BG_TRY(values->alloc(temp_values_bytes(r1 - v0)));
    BG_TRY(pull_bytes(c, dst_dev, src_dev, values->p, reinterpret_cast<const char *>(sc.values) + 8 * v0, (size_t)(r1 - v0) * 8, sc.residency));
    *out = device_col(values->p, b - a, sc.type);
    out->offset = r0 - v0;
    if (has_bitmap(sc)) {
        const BitBytes src = bit_bytes(r0, r1 - r0);   // (stage_bits' upload, but the source may be another device)
        BG_TRY(bits->alloc(temp_bits_bytes(src.count)));
        BG_HIP(hipMemsetAsync(bits->p, 0, bits->bytes, c->stream));
        BG_TRY(pull_bytes(c, dst_dev, src_dev, bits->p, sc.validity + src.first, src.count, sc.residency));
        out->validity = bits->as<const uint8_t>();
        out->null_count = -1;
    }
    return 0;
}

int recount_nulls(Ctx *c, const void *bits, int64_t n, int64_t *nulls) {
    uint64_t *d_count;
    BG_TRY(scratch_at(c, kScrOneCount, &d_count));
    uint64_t set = 0;
    BG_TRY(launch_popcount(c, reinterpret_cast<const uint32_t *>(bits), 0, n, d_count));
    BG_HIP(hipMemcpyAsync(&set, d_count, 8, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    *nulls = n - (int64_t)set;
    return 0;
}

int temp_to_caller(Ctx *c, const DevFrame &f, int32_t i, int64_t n, int32_t type, int64_t null_count, bowgpu_out *out, int pool_slot) {
    DevOut d;
    BG_TRY(devout_prepare(c, out, n, &d, pool_slot));
    BG_HIP(hipMemcpyAsync(d.values, f.values[i].p, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
    BG_HIP(hipMemcpyAsync(d.validity, f.bits[i].p, (size_t)((n + 7) >> 3), hipMemcpyDeviceToDevice, c->stream));
    BG_TRY(devout_finish(c, &d, n, type, null_count, true));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace bowgpu
