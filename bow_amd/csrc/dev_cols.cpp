// dev_cols.cpp — the staging layer under every entry point: a caller's Arrow buffers made readable by a kernel (values aliased,
// mapped or uploaded; bits - a validity bitmap, a Boolean column's values - as an aligned 32-bit word pointer plus the bit index of
// row 0: stage_bits over the arithmetic of bit_span.h), output columns assembled on the device and handed back (devout_prepare /
// devout_finish, through a word-aligned working copy of every bitmap), and the copies of pageable host memory behind both.

#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "common.h"

namespace bowgpu {

int fetch_valid(Ctx *c, const bowgpu_col *col, int64_t row, int *valid) {
    if (!col->validity) { *valid = 1; return 0; }
    const int64_t bit = col->offset + row;
    uint8_t byte = 0;
    if (col->residency == BOWGPU_DEVICE) {
        if (!c) BG_TRY(ctx_get(&c));
        BG_HIP(hipMemcpyAsync(&byte, col->validity + (bit >> 3), 1, hipMemcpyDeviceToHost, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
    } else {
        byte = col->validity[bit >> 3];
    }
    *valid = (byte >> (bit & 7)) & 1;
    return 0;
}

int count_nulls_device(Ctx *c, DevCol *dc) {
    if (!dc->vbits || dc->length == 0) { dc->null_count = 0; return 0; }
    uint64_t *dcount;
    BG_TRY(scratch_at(c, kScrNullCount, &dcount));
    BG_TRY(launch_popcount(c, dc->vbits, dc->vbit0, dc->length, dcount));
    uint64_t set = 0;
    BG_HIP(hipMemcpyAsync(&set, dcount, 8, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    dc->null_count = dc->length - (int64_t)set;
    return 0;
}

const void *host_mapped(const void *p, const char *what) {
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) == hipSuccess && d) return d;
    (void)hipGetLastError();
    set_error("BOWGPU_HOST_PINNED: the %s buffer is not registered (bowgpu_host_register)", what);
    return nullptr;
}

// A caller's input buffer is copied into HBM rather than read where it lies: pageable memory always, registered memory under
// BOWGPU_ROUTE_PINNED_STAGE (A/B switch: staged by DMA like pageable memory instead of being read in place over the link)
static bool staged_residency(int32_t residency) {
    return residency == BOWGPU_HOST || (residency == BOWGPU_HOST_PINNED && (route_mask() & BOWGPU_ROUTE_PINNED_STAGE) != 0);
}

int stage_bits(Ctx *c, const uint8_t *bytes, int64_t offset, int64_t n, int32_t residency, const char *what, DevBits *out) {
    if (!residency_ok(residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", residency);
    const void *dev = bytes;
    if (staged_residency(residency)) {
        // the bytes that hold the rows, in a zeroed word-padded block
        const BitBytes src = bit_bytes(offset, n);
        BG_TRY(out->own.alloc(temp_bits_bytes(src.count)));
        BG_HIP(hipMemsetAsync(out->own.p, 0, out->own.bytes, c->stream));
        BG_TRY(copy_h2d(c, out->own.p, bytes + src.first, src.count, residency == BOWGPU_HOST_PINNED));
        dev = out->own.p;
        offset = src.bit0;
    } else if (residency == BOWGPU_HOST_PINNED && !(dev = host_mapped(bytes, what))) {
        return BOWGPU_ERR_ARG;
    }
    const BitWords w = bit_words(reinterpret_cast<uintptr_t>(dev), offset, n);
    out->words = reinterpret_cast<const uint32_t *>(w.addr);
    out->bit0 = w.bit0;
    out->nwords = w.words;
    return 0;
}

int devcol_prepare(Ctx *c, const bowgpu_col *col, DevCol *out, bool need_values, bool need_validity) {
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (col->length > 0 && !col->values) return fail(BOWGPU_ERR_ARG, "column has no values buffer");
    out->length = col->length;
    out->type = col->type;
    out->null_count = col->null_count;
    const int64_t n = col->length;
    if (n == 0) { out->null_count = 0; return 0; }
    if (!residency_ok(col->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col->residency);
    const bool has_bitmap = col->validity != nullptr && col->null_count != 0;
    const bool staged = staged_residency(col->residency);
    // values: device memory as it is, registered host memory where it lies (zero-copy: coalesced 16-byte loads over PCIe), or a copy
    if (!staged) {
        if (reinterpret_cast<uintptr_t>(col->values) & 7) return fail(BOWGPU_ERR_ARG, "values buffer must be 8-byte aligned");
        const void *dv = col->values;
        if (col->residency == BOWGPU_HOST_PINNED && !(dv = host_mapped(col->values, "values"))) return BOWGPU_ERR_ARG;
        out->values = reinterpret_cast<const char *>(dv) + 8 * col->offset;
    } else if (need_values) {
        BG_TRY(out->own_values.alloc(temp_values_bytes(n)));
        BG_TRY(copy_h2d(c, out->own_values.p, reinterpret_cast<const char *>(col->values) + 8 * col->offset, (size_t)n * 8,
                        col->residency == BOWGPU_HOST_PINNED));
        out->values = out->own_values.p;
    }
    // validity (a copy only where the caller reads it)
    if (has_bitmap && (!staged || need_validity)) {
        DevBits b;
        BG_TRY(stage_bits(c, col->validity, col->offset, n, col->residency, "validity", &b));
        out->vbits = b.words;
        out->vbit0 = b.bit0;
        out->vwords = b.nwords;
        out->own_validity = std::move(b.own);
    }
    if (has_bitmap && out->vbits && col->null_count < 0) BG_TRY(count_nulls_device(c, out));
    if (!has_bitmap) out->null_count = 0;
    if (out->null_count == 0) { out->vbits = nullptr; }
    return 0;
}

int devboolcol_prepare(Ctx *c, const bowgpu_col *col, DevBoolCol *out) {
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (col->length == 0) return 0;
    if (!col->values) return fail(BOWGPU_ERR_ARG, "column has no values buffer");
    BG_TRY(stage_bits(c, reinterpret_cast<const uint8_t *>(col->values), col->offset, col->length, col->residency, "values", &out->t));
    if (col->validity && col->null_count != 0) BG_TRY(stage_bits(c, col->validity, col->offset, col->length, col->residency, "validity", &out->v));
    return 0;
}

int devout_prepare(Ctx *c, bowgpu_out *out, int64_t slots, DevOut *d, int pool_slot, bool bit_values) {
    d->user = out;
    d->bit_values = bit_values;
    if (out->length < slots) return fail(BOWGPU_ERR_ARG, "output column has %lld slots, %lld needed", (long long)out->length, (long long)slots);
    if (slots == 0) return 0;
    if (!out->values || !out->validity) return fail(BOWGPU_ERR_ARG, "output column lacks a values or validity buffer");
    if (!residency_ok(out->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", out->residency);
    const bool device = out->residency == BOWGPU_DEVICE;
    const size_t bits_bytes = temp_bits_bytes((size_t)((slots + 7) >> 3));
    // values: 8-byte slots are written in place in a caller's device buffer; bits are assembled like the validity
    if (device && !bit_values) {
        if (reinterpret_cast<uintptr_t>(out->values) & 7) return fail(BOWGPU_ERR_ARG, "output values must be 8-byte aligned");
        d->values = out->values;
    } else {
        BG_TRY(d->own_values.alloc(bit_values ? bits_bytes : (size_t)slots * 8));
        d->values = d->own_values.p;
    }
    // The kernels update validity as 32-bit words; a caller buffer of exactly ceil(W/8) bytes may end
    // mid-word, so always assemble in an aligned temporary and copy the exact byte count back.
    if (device && pool_slot >= 0) {
        void *pp;
        BG_TRY(ctx_pool(c, pool_slot, bits_bytes, &pp));
        d->validity = reinterpret_cast<uint8_t *>(pp);
    } else {
        BG_TRY(d->own_validity.alloc(bits_bytes));
        d->validity = reinterpret_cast<uint8_t *>(d->own_validity.p);
    }
    return 0;
}

// Device <-> host copies of PAGEABLE caller buffers go through the context's own pinned staging (two kBouncePiece halves: the
// DMA of one overlaps the CPU copy of the other) and never hand the caller's pointer to the HIP runtime.  The runtime would pin
// the caller's pages itself (a userptr mapping, kept in a cache), and that goes wrong in ways the library cannot see: it refuses
// a range that lies only partly inside a registered one (a small malloc'ed buffer sharing a page with a buffer somebody
// registered), and on this pool GPU writes through such mappings were seen to die with "write access to a read-only page" on
// fresh machines.  Small copies (the runtime stages those itself) and BOWGPU_RUNTIME_PINS=1 (A/B switch) keep the direct form.
constexpr size_t kBouncePiece = 4u << 20;
constexpr size_t kBounceDirect = 16384;
static bool runtime_pins() {
    static const bool on = [] { const char *e = getenv("BOWGPU_RUNTIME_PINS"); return e && e[0] == '1'; }();
    return on;
}
static int bounce_get(Ctx *c, char **half0, char **half1) {
    if (!c->h_bounce) {
        BG_HIP(hipHostMalloc(&c->h_bounce, 2 * kBouncePiece, hipHostMallocDefault));   // (its own block: ctx_pinned's must not move)
        BG_HIP(hipEventCreateWithFlags(&c->bounce_ev[0], hipEventDisableTiming));
        BG_HIP(hipEventCreateWithFlags(&c->bounce_ev[1], hipEventDisableTiming));
    }
    *half0 = reinterpret_cast<char *>(c->h_bounce);
    *half1 = *half0 + kBouncePiece;
    return 0;
}
// The CPU side of the staging: one core copies at ~12 GB/s, the link takes 55.  Pieces of a megabyte or more are split over a small
// process-wide pool of helper threads (they only ever call memcpy; created on first use, BOWGPU_COPY_THREADS = 0 .. 8, default 3;
// the pool object is never destroyed, so no thread can wake up into a torn-down condition variable at exit).
namespace {
struct CopyPool {
    struct Job { char *d; const char *s; size_t n; std::atomic<int> *left; };
    std::mutex m;
    std::condition_variable work, done;
    std::vector<Job> q;
    int nthreads = 0;
    void run() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(m);
                work.wait(lk, [&] { return !q.empty(); });
                j = q.back();
                q.pop_back();
            }
            memcpy(j.d, j.s, j.n);
            if (j.left->fetch_sub(1) == 1) {
                std::lock_guard<std::mutex> lk(m);
                done.notify_all();
            }
        }
    }
};
CopyPool *copy_pool() {
    static CopyPool *pool = [] {
        CopyPool *p = new CopyPool();   // (leaked on purpose)
        const char *e = getenv("BOWGPU_COPY_THREADS");
        int n = e ? atoi(e) : 3;
        if (n < 0) n = 0;
        if (n > 8) n = 8;
        for (int i = 0; i < n; i++) {
            try { std::thread([p] { p->run(); }).detach(); p->nthreads++; } catch (...) { break; }
        }
        return p;
    }();
    return pool;
}
}  // namespace
void staged_memcpy(void *dst, const void *src, size_t n) {
    constexpr size_t kMinPart = 256u << 10;
    CopyPool *p = n >= 4 * kMinPart ? copy_pool() : nullptr;
    if (!p || p->nthreads == 0) { memcpy(dst, src, n); return; }
    const int parts = p->nthreads + 1;
    const size_t part = ((n / parts) + 63) & ~(size_t)63;
    std::atomic<int> left(0);
    char *d = reinterpret_cast<char *>(dst);
    const char *s = reinterpret_cast<const char *>(src);
    size_t off = part;   // [0, part) is the caller's own share
    {
        std::lock_guard<std::mutex> lk(p->m);
        for (int i = 1; i < parts && off < n; i++, off += part) {
            const size_t len = off + part < n && i + 1 < parts ? part : n - off;
            left.fetch_add(1);
            p->q.push_back({d + off, s + off, len, &left});
            if (len == n - off) { off = n; break; }
        }
    }
    p->work.notify_all();
    memcpy(d, s, part < n ? part : n);
    std::unique_lock<std::mutex> lk(p->m);
    p->done.wait(lk, [&] { return left.load() == 0; });
}

int copy_d2h(Ctx *c, void *dst, const void *src, size_t bytes, bool registered) {
    if (bytes == 0) return 0;
    if (bytes <= kBounceDirect || registered || runtime_pins()) {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) return 0;
        (void)hipGetLastError();
        if (e != hipErrorInvalidValue) return hip_fail(e, "hipMemcpyAsync (device to host)");
    }
    char *h[2];
    BG_TRY(bounce_get(c, &h[0], &h[1]));
    const size_t pieces = (bytes + kBouncePiece - 1) / kBouncePiece;
    auto len = [&](size_t k) { return k + 1 < pieces ? kBouncePiece : bytes - k * kBouncePiece; };
    for (size_t k = 0; k <= pieces; k++) {
        if (k < pieces) {   // piece k on its way into half k & 1 ...  (behind an earlier upload out of that half: stream order would do, but
                            // the caller may have switched streams since - bowgpu_set_stream - so wait for the upload's event)
            if (c->bounce_busy[k & 1]) BG_HIP(hipEventSynchronize(c->bounce_ev[k & 1]));
            c->bounce_busy[k & 1] = false;
            BG_HIP(hipMemcpyAsync(h[k & 1], reinterpret_cast<const char *>(src) + k * kBouncePiece, len(k), hipMemcpyDeviceToHost, c->stream));
            BG_HIP(hipEventRecord(c->bounce_ev[k & 1], c->stream));
        }
        if (k > 0) {        // ... while piece k - 1 leaves the other half
            BG_HIP(hipEventSynchronize(c->bounce_ev[(k - 1) & 1]));
            staged_memcpy(reinterpret_cast<char *>(dst) + (k - 1) * kBouncePiece, h[(k - 1) & 1], len(k - 1));
        }
    }
    return 0;
}
int copy_h2d(Ctx *c, void *dst, const void *src, size_t bytes, bool registered) {
    if (bytes == 0) return 0;
    if (bytes <= kBounceDirect || registered || runtime_pins()) {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) return 0;
        (void)hipGetLastError();
        if (e != hipErrorInvalidValue) return hip_fail(e, "hipMemcpyAsync (host to device)");
    }
    char *h[2];
    BG_TRY(bounce_get(c, &h[0], &h[1]));
    const size_t pieces = (bytes + kBouncePiece - 1) / kBouncePiece;
    for (size_t k = 0; k < pieces; k++) {
        const size_t m = k + 1 < pieces ? kBouncePiece : bytes - k * kBouncePiece;
        if (c->bounce_busy[k & 1]) BG_HIP(hipEventSynchronize(c->bounce_ev[k & 1]));   // the DMA that last read this half is done
        staged_memcpy(h[k & 1], reinterpret_cast<const char *>(src) + k * kBouncePiece, m);
        BG_HIP(hipMemcpyAsync(reinterpret_cast<char *>(dst) + k * kBouncePiece, h[k & 1], m, hipMemcpyHostToDevice, c->stream));
        BG_HIP(hipEventRecord(c->bounce_ev[k & 1], c->stream));
        c->bounce_busy[k & 1] = true;
    }
    return 0;
}

int devout_finish(Ctx *c, DevOut *d, int64_t slots, int32_t type, int64_t null_count, bool copy_bitmap) {
    bowgpu_out *out = d->user;
    out->length = slots;
    out->type = type;
    out->null_count = null_count;
    if (slots == 0) return 0;
    const size_t vb = (size_t)((slots + 7) >> 3);
    const size_t value_bytes = d->bit_values ? vb : (size_t)slots * 8;
    if (out->residency == BOWGPU_DEVICE) {
        if (d->bit_values) BG_HIP(hipMemcpyAsync(out->values, d->values, value_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (copy_bitmap) BG_HIP(hipMemcpyAsync(out->validity, d->validity, vb, hipMemcpyDeviceToDevice, c->stream));
    } else {
        // (registered buffers take the DMA directly; pageable ones go through the staging halves)
        BG_TRY(copy_d2h(c, out->values, d->values, value_bytes, out->residency == BOWGPU_HOST_PINNED));
        BG_TRY(copy_d2h(c, out->validity, d->validity, vb, out->residency == BOWGPU_HOST_PINNED));
    }
    return 0;
}

}  // namespace bowgpu
