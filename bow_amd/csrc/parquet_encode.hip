// parquet_encode.hip — the device side of bowgpu_parquet_write: rows [a, b) of one column (one column chunk of one row group)
// turned into what the pages of a Parquet file hold.  Hand-written for gfx950 (wave64); the file assembly is parquet_write.cpp.
//
//   pq_page_levels_kernel   one workgroup per page: the page's validity bits re-based so that its first row is bit 0 (64-bit words
//                           of a levels image, page p at byte p * page_rows / 8) and the count of its valid rows
//   (valid_mask_kernel, the scan, filter_scatter_kernel: the row group's non-null values in row order - frame_ops / filter.hip)
//   pq_minmax_kernel        per workgroup one (min, max, any usable value) record over the dense values; the host folds them
//   pq_delta_sizes_kernel   DELTA_BINARY_PACKED, one wavefront per block of 128 differences of a page's slice of the dense values:
//                           the block's minimum, its four miniblock widths, its byte count
//   (the scan of the byte counts: sort.hip launch_scan_u32)
//   pq_delta_pages_kernel   one thread per page: where the page's body lies in the values image, its header, its byte count
//   pq_delta_pack_kernel    one wavefront per block: the block's bytes assembled in LDS - one lane per 32-bit word of a miniblock,
//                           built from the remainders that overlap it - and stored with aligned 8-byte stores, bytes at the edges
//   (RLE_DICTIONARY: parquet_dict.hip finds the chunk's dictionary and packs the indices - pq_dict_chunk; a chunk without a value
//    or with more distinct patterns than the cap is written PLAIN here, and PqEncChunk::encoding says which it was)
//   (codec SNAPPY: the values sections stay on the device and snappy_encode.hip compresses them there - pq_snappy_chunk)
// The host side: pq_encode_chunk, a list of named steps, and pq_finish_chunk, the hand-over to parquet_write.cpp that it shares with
// pq_encode_bool_chunk (parquet_bool_encode.hip).  What crosses files is declared once, in parquet_encode.h.
//
// No atomics, no workgroup waits on another, every byte of the output is a function of the input alone.  Nothing reads or
// writes global memory unaligned: a block body starts at an arbitrary byte of the image, so its LDS copy is laid out at the same
// offset inside an 8-byte word as its destination.
#include <string.h>

#include "parquet_encode.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kDeltaBlock = 128;          // differences per block; 4 miniblocks of 32 (parquet-mr's layout for INT64)
constexpr int kPageSlack = 32;            // bytes of the values image between two pages' regions: room for a header (at most 18) and the 8-byte alignment

struct PqDevPage {       // one page of the chunk as the delta kernels see it; entry [npages] closes the table (blk0 = blocks in all)
    int64_t v0;          // first of the page's values in the dense array
    int32_t count;       // its non-null values
    uint32_t blk0;       // blocks of the earlier pages
};
struct PqDevInfo {       // what pq_delta_pages_kernel leaves per page
    uint64_t off;        // of the page's values section in the image (8-byte aligned)
    uint32_t bytes, hdr; // of the section; of its header
};

// ---------------------------------------------------------------- levels
__global__ __launch_bounds__(kThreads) void pq_page_levels_kernel(const uint32_t *vbits, int64_t vbit0, int64_t vwords, int64_t n, int32_t page_rows,
                                                                  unsigned long long *levels, uint32_t *counts) {
    __shared__ uint32_t wsum[kWaves];
    const int64_t page = blockIdx.x, row0 = page * page_rows;
    const int words = page_rows >> 6;
    uint32_t cnt = 0;
    for (int j = threadIdx.x; j < words; j += kThreads) {
        const int64_t base = row0 + (int64_t)j * 64;
        if (base >= n) break;
        const int64_t bit = vbit0 + base, wi = bit >> 5;
        const int sh = (int)(bit & 31);
        const uint64_t w0 = wi < vwords ? vbits[wi] : 0u, w1 = wi + 1 < vwords ? vbits[wi + 1] : 0u, w2 = wi + 2 < vwords ? vbits[wi + 2] : 0u;
        const uint64_t lo = (uint32_t)((w0 | (w1 << 32)) >> sh), hi = (uint32_t)((w1 | (w2 << 32)) >> sh);
        unsigned long long word = lo | (hi << 32);
        const int64_t left = n - base;
        if (left < 64) word &= (1ull << left) - 1ull;   // (the padding of the last group of 8 is zero bits)
        levels[page * words + j] = word;
        cnt += (uint32_t)__popcll(word);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) t += wsum[i];
        counts[page] = t;
    }
}

// ---------------------------------------------------------------- statistics
// rec[3 * block + {0, 1, 2}] = min, max (raw payloads), whether any value took part.  Int64: signed order.  Float64: a NaN takes no
// part; the two zeroes compare equal here and the host writes the sign the format asks for.
template <bool kFloat>
__global__ __launch_bounds__(kThreads) void pq_minmax_kernel(const uint64_t *v, int64_t m, uint64_t *rec) {
    __shared__ uint64_t smin[kWaves], smax[kWaves];
    __shared__ uint32_t sany[kWaves];
    uint64_t mn = 0, mx = 0;
    bool any = false;
    auto less = [](uint64_t a, uint64_t b) {
        return kFloat ? __longlong_as_double((long long)a) < __longlong_as_double((long long)b) : (int64_t)a < (int64_t)b;
    };
    auto take = [&](uint64_t x, uint64_t y, bool ok) {   // (x, y): a minimum and a maximum that took part when ok
        if (ok) {
            if (!any || less(x, mn)) mn = x;
            if (!any || less(mx, y)) mx = y;
            any = true;
        }
    };
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        const uint64_t x = v[i];
        const double d = __longlong_as_double((long long)x);
        take(x, x, !kFloat || d == d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)mn, o), y = (uint64_t)__shfl_xor((unsigned long long)mx, o);
        const bool ok = __shfl_xor((int)any, o) != 0;
        take(x, y, ok);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smin[w] = mn; smax[w] = mx; sany[w] = any; }
    __syncthreads();
    if (threadIdx.x == 0) {
        any = false;
        for (int i = 0; i < kWaves; i++) take(smin[i], smax[i], sany[i] != 0);
        rec[3 * (int64_t)blockIdx.x + 0] = mn;
        rec[3 * (int64_t)blockIdx.x + 1] = mx;
        rec[3 * (int64_t)blockIdx.x + 2] = any ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- DELTA_BINARY_PACKED
__device__ __forceinline__ int width_of(uint64_t x) { return x ? 64 - __clzll((long long)x) : 0; }
__device__ __forceinline__ uint64_t zigzag64(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
__device__ __forceinline__ int varint_len(uint64_t v) { return v ? (width_of(v) + 6) / 7 : 1; }
__device__ __forceinline__ int put_varint(uint8_t *p, uint64_t v) {
    int k = 0;
    while (v >= 0x80) { p[k++] = (uint8_t)(v | 0x80); v >>= 7; }
    p[k++] = (uint8_t)v;
    return k;
}

// the page of block g: the last one whose blk0 is not above g (pages without a block share their blk0 with the page behind them)
__device__ __forceinline__ int64_t page_of_block(const PqDevPage *pages, int64_t npages, uint32_t g) {
    int64_t lo = 0, hi = npages - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (pages[mid].blk0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The wrapping differences of block g that this lane holds: number `lane` and number `lane + 64` of the block (miniblocks 0 / 1 are
// the two halves of the wave on the first, 2 / 3 on the second).  ok: the difference exists.
struct LaneDeltas { int64_t d[2]; bool ok[2]; };
__device__ __forceinline__ LaneDeltas block_deltas(const uint64_t *v, const PqDevPage &pg, uint32_t b, int lane) {
    LaneDeltas r;
    const int64_t nd = (int64_t)pg.count - 1;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int64_t j = (int64_t)b * kDeltaBlock + h * 64 + lane;
        r.ok[h] = j < nd;
        r.d[h] = 0;
        if (r.ok[h]) r.d[h] = (int64_t)(v[pg.v0 + j + 1] - v[pg.v0 + j]);   // (the last index read: v0 + count - 1)
    }
    return r;
}

__global__ __launch_bounds__(kThreads) void pq_delta_sizes_kernel(const uint64_t *v, const PqDevPage *pages, int64_t npages, uint32_t nblocks,
                                                                  int64_t *blk_min, uint32_t *blk_widths, uint32_t *blk_bytes) {
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g >= nblocks) return;   // (wave-uniform; no barrier in this kernel)
    const int64_t p = page_of_block(pages, npages, g);
    const PqDevPage pg = pages[p];
    const LaneDeltas ld = block_deltas(v, pg, g - pg.blk0, lane);
    int64_t mn = INT64_MAX;
    if (ld.ok[0]) mn = ld.d[0];
    if (ld.ok[1] && ld.d[1] < mn) mn = ld.d[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = (int64_t)__shfl_xor((long long)mn, o); mn = y < mn ? y : mn; }
    // a miniblock's width is that of its largest remainder: of the OR of its remainders
    uint64_t r0 = ld.ok[0] ? (uint64_t)ld.d[0] - (uint64_t)mn : 0, r1 = ld.ok[1] ? (uint64_t)ld.d[1] - (uint64_t)mn : 0;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {   // (stays inside each half of the wave)
        r0 |= (uint64_t)__shfl_xor((unsigned long long)r0, o);
        r1 |= (uint64_t)__shfl_xor((unsigned long long)r1, o);
    }
    const int wa = width_of(r0), wb = width_of(r1);
    const uint32_t w0 = (uint32_t)__shfl(wa, 0), w1 = (uint32_t)__shfl(wa, 32), w2 = (uint32_t)__shfl(wb, 0), w3 = (uint32_t)__shfl(wb, 32);
    if (lane == 0) {
        blk_min[g] = mn;
        blk_widths[g] = w0 | (w1 << 8) | (w2 << 16) | (w3 << 24);
        blk_bytes[g] = (uint32_t)varint_len(zigzag64(mn)) + 4u + 4u * (w0 + w1 + w2 + w3);   // a miniblock of width w: 32 * w bits
    }
}

// scan: the exclusive scan of blk_bytes, nblocks + 1 entries (the last: all of them).  Page p's section starts 8-byte aligned at
// align8(scan[blk0]) + kPageSlack * p: the sections cannot meet, and no host round trip lies between the sizes and the pack pass.
__device__ __forceinline__ uint64_t page_region(const uint32_t *scan, uint32_t blk0, int64_t p) {
    return (((uint64_t)scan[blk0] + 7u) & ~(uint64_t)7) + (uint64_t)kPageSlack * (uint64_t)p;
}

__global__ __launch_bounds__(kThreads) void pq_delta_pages_kernel(const uint64_t *v, const PqDevPage *pages, int64_t npages, const uint32_t *scan,
                                                                  uint8_t *image, PqDevInfo *info) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= npages) return;
    const PqDevPage pg = pages[p];
    const uint64_t off = page_region(scan, pg.blk0, p);
    uint8_t *h = image + off;
    int k = 0;
    h[k++] = 0x80; h[k++] = 0x01;   // block size 128
    h[k++] = 4;                     // miniblocks per block
    k += put_varint(h + k, (uint64_t)pg.count);
    k += put_varint(h + k, zigzag64(pg.count > 0 ? (int64_t)v[pg.v0] : 0));
    info[p].off = off;
    info[p].hdr = (uint32_t)k;
    info[p].bytes = (uint32_t)k + (scan[pages[p + 1].blk0] - scan[pg.blk0]);
}

constexpr int kBlockMaxBytes = 10 + 4 + 4 * 4 * 64;        // minimum, widths, four miniblocks of width 64
constexpr int kBufWords = (7 + kBlockMaxBytes + 7) / 8 + 1;   // ... behind up to 7 bytes of offset
__global__ __launch_bounds__(kThreads) void pq_delta_pack_kernel(const uint64_t *v, const PqDevPage *pages, int64_t npages, uint32_t nblocks,
                                                                 const int64_t *blk_min, const uint32_t *blk_widths, const uint32_t *scan,
                                                                 const PqDevInfo *info, uint8_t *image) {
    __shared__ uint64_t srem[kWaves][kDeltaBlock];   // the block's remainders
    __shared__ uint64_t sbuf[kWaves][kBufWords];     // its bytes, at the offset inside an 8-byte word that they have in the image
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t g = blockIdx.x * kWaves + w;
    const bool active = g < nblocks;   // (wave-uniform; every wave takes part in the barriers)
    uint64_t dst = 0;
    uint32_t len = 0, widths = 0;
    int64_t mn = 0;
    if (active) {
        const int64_t p = page_of_block(pages, npages, g);
        const PqDevPage pg = pages[p];
        const LaneDeltas ld = block_deltas(v, pg, g - pg.blk0, lane);
        mn = blk_min[g];
        widths = blk_widths[g];
        srem[w][lane] = ld.ok[0] ? (uint64_t)ld.d[0] - (uint64_t)mn : 0;        // (a padded slot of the last miniblock: zero bits)
        srem[w][lane + 64] = ld.ok[1] ? (uint64_t)ld.d[1] - (uint64_t)mn : 0;
        dst = info[p].off + info[p].hdr + (uint64_t)(scan[g] - scan[pg.blk0]);
        len = scan[g + 1] - scan[g];
        for (int j = lane; j < kBufWords; j += 64) sbuf[w][j] = 0;
    }
    __syncthreads();
    const uint32_t s = (uint32_t)(dst & 7);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(&sbuf[w][0]);
    if (active) {
        const uint64_t zz = zigzag64(mn);
        const uint32_t hl = (uint32_t)varint_len(zz) + 4u;
        if (lane == 0) {
            const int k = put_varint(bytes + s, zz);
#pragma unroll
            for (int m = 0; m < 4; m++) bytes[s + k + m] = (uint8_t)(widths >> (8 * m));
        }
        uint32_t at = s + hl;   // byte of the LDS copy at which the next miniblock's body starts
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const uint32_t wd = (widths >> (8 * m)) & 0xFFu;
            if ((uint32_t)lane < wd) {   // one lane per 32-bit word of the miniblock: bits [32 q, 32 q + 32) of its 32 * wd
                const uint32_t q = (uint32_t)lane, B = 32u * q;
                const uint32_t i0 = B / wd, i1 = min(31u, (B + 31u) / wd);
                uint32_t word = 0;
                for (uint32_t i = i0; i <= i1; i++) {   // value i holds bits [i wd, i wd + wd): both shifts stay below 64 (resp. 32)
                    const uint64_t r = srem[w][32 * m + i];
                    const uint32_t bi = i * wd;
                    word |= bi >= B ? (bi - B < 32u ? (uint32_t)r << (bi - B) : 0u) : (uint32_t)(r >> (B - bi));
                }
                uint8_t *o = bytes + at + 4u * q;
                o[0] = (uint8_t)word; o[1] = (uint8_t)(word >> 8); o[2] = (uint8_t)(word >> 16); o[3] = (uint8_t)(word >> 24);
            }
            at += 4u * wd;
        }
    }
    __syncthreads();
    if (active) {
        // the copy's bytes [s, s + len) to the image: 8-byte word j of the copy is the aligned word at (dst - s) + 8 j
        uint8_t *gbase = image + (dst - s);
        const uint32_t end = s + len;
        for (uint32_t j = (uint32_t)lane; 8u * j < end; j += 64u) {
            const uint32_t lo = 8u * j, hi = lo + 8u;
            if (lo >= s && hi <= end) {
                reinterpret_cast<uint64_t *>(gbase)[j] = sbuf[w][j];
            } else {   // a word shared with the neighbouring block (or the header): its own bytes only
                const uint32_t k0 = lo > s ? lo : s, k1 = hi < end ? hi : end;
                for (uint32_t k = k0; k < k1; k++) gbase[k] = bytes[k];
            }
        }
    }
}

int checked_launch() {
    BG_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- the steps of pq_encode_chunk
// rows [a, b) on the device, from an 8-row boundary: one bit offset serves values and bits
int stage_chunk(Ctx *c, const bowgpu_col &col, int64_t a, int64_t b, DevBuf *svals, DevBuf *sbits, DevCol *dk) {
    bowgpu_col piece;
    BG_TRY(stage_rows(c, c->device, c->device, col, a, b, svals, sbits, &piece));
    piece = uncounted(piece);
    return devcol_prepare(c, &piece, dk, true, true);
}

// counts[p]: page p's valid rows, *m: the chunk's; d_levels: the levels image, where the column has a bitmap to read
int page_levels(Ctx *c, const DevCol &dk, const PqGrid &g, DevBuf *d_levels, DevBuf *d_counts, std::vector<uint32_t> *counts, int64_t *m) {
    counts->resize((size_t)g.npages);
    if (dk.vbits) {
        BG_TRY(d_levels->alloc((size_t)g.npages * g.level_bytes()));
        BG_TRY(d_counts->alloc((size_t)g.npages * 4));
        hipLaunchKernelGGL(pq_page_levels_kernel, dim3((unsigned)g.npages), dim3(kThreads), 0, c->stream, dk.vbits, dk.vbit0, dk.vwords, g.n, g.page_rows,
                           d_levels->as<unsigned long long>(), d_counts->as<uint32_t>());
        BG_TRY(checked_launch());
        BG_TRY(copy_d2h(c, counts->data(), d_counts->p, (size_t)g.npages * 4));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    *m = 0;
    for (int64_t p = 0; p < g.npages; p++) {
        if (!dk.vbits) (*counts)[(size_t)p] = (uint32_t)g.rows(p);
        *m += (*counts)[(size_t)p];
    }
    return 0;
}

// *dense: the chunk's m non-null values in row order (what frame_ops_api.cpp does for Bow.Distinct's key); a chunk without nulls
// is its own dense array
int compact_valid(Ctx *c, const DevCol &dk, int64_t m, MaskWork *w, DevBuf *vals, DevBuf *bits, const uint64_t **dense) {
    *dense = reinterpret_cast<const uint64_t *>(dk.values);
    if (m == 0 || m == dk.length) return 0;
    TileRecords t;
    BG_TRY(valid_rows_scanned(c, dk, w, &t));
    if (w->selected != m) return fail(BOWGPU_ERR_HIP, "parquet: the page counts (%lld) and the compaction (%lld) disagree", (long long)m, (long long)w->selected);
    BG_TRY(vals->alloc(temp_values_bytes(m)));
    BG_TRY(bits->alloc((size_t)((m + 63) >> 6) * 8));
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
    *dense = vals->as<const uint64_t>();
    return launch_filter_scatter(c, s);
}

// the (min, max, any) records of the m > 0 dense values on their way into rec: read them behind a synchronise (fold_minmax)
int launch_minmax(Ctx *c, bool is_float, const uint64_t *dense, int64_t m, DevBuf *d_rec, std::vector<uint64_t> *rec) {
    const int64_t grid = stream_grid(m, kThreads);
    rec->resize((size_t)grid * 3);
    BG_TRY(d_rec->alloc(rec->size() * 8));
    if (is_float) hipLaunchKernelGGL(pq_minmax_kernel<true>, dim3((unsigned)grid), dim3(kThreads), 0, c->stream, dense, m, d_rec->as<uint64_t>());
    else hipLaunchKernelGGL(pq_minmax_kernel<false>, dim3((unsigned)grid), dim3(kThreads), 0, c->stream, dense, m, d_rec->as<uint64_t>());
    BG_TRY(checked_launch());
    return copy_d2h(c, rec->data(), d_rec->p, rec->size() * 8);
}

void fold_minmax(const std::vector<uint64_t> &rec, bool is_float, PqwStats *st) {
    bool any = false;
    uint64_t mn = 0, mx = 0;
    auto less = [&](uint64_t x, uint64_t y) {
        if (!is_float) return (int64_t)x < (int64_t)y;
        double dx, dy;
        memcpy(&dx, &x, 8);
        memcpy(&dy, &y, 8);
        return dx < dy;
    };
    for (size_t k = 0; k + 2 < rec.size(); k += 3) {
        if (!rec[k + 2]) continue;
        if (!any || less(rec[k], mn)) mn = rec[k];
        if (!any || less(mx, rec[k + 1])) mx = rec[k + 1];
        any = true;
    }
    if (any && is_float) {   // TYPE_DEFINED_ORDER: a zero minimum is written as -0.0, a zero maximum as +0.0
        if ((mn << 1) == 0) mn = 0x8000000000000000ull;
        if ((mx << 1) == 0) mx = 0;
    }
    st->has_minmax = any;
    st->min = mn;
    st->max = mx;
}

// PLAIN: the sections lie in the dense values as they are
void plain_sections(const uint64_t *dense, const std::vector<uint32_t> &counts, PqSections *s) {
    s->image = reinterpret_cast<const uint8_t *>(dense);
    s->off.clear();
    s->len.clear();
    int64_t v0 = 0;
    for (const uint32_t cnt : counts) {
        s->off.push_back(8 * v0);
        s->len.push_back(8 * (int64_t)cnt);
        v0 += cnt;
    }
    s->used = (size_t)v0 * 8;
}

// DELTA_BINARY_PACKED: sizes, their scan, the page headers, the pack pass; the stream has drained when this returns
int delta_sections(Ctx *c, const uint64_t *dense, const std::vector<uint32_t> &counts, PqSections *s) {
    const int64_t npages = (int64_t)counts.size();
    DevBuf d_pages, d_min, d_widths, d_bytes, d_sums, d_info;
    std::vector<PqDevPage> pages((size_t)npages + 1);
    int64_t v0 = 0, nblocks = 0;
    for (int64_t p = 0; p <= npages; p++) {
        const int64_t cnt = p < npages ? counts[(size_t)p] : 0;
        pages[(size_t)p] = PqDevPage{v0, (int32_t)cnt, (uint32_t)nblocks};
        v0 += cnt;
        nblocks += cnt > 1 ? (cnt - 1 + kDeltaBlock - 1) / kDeltaBlock : 0;
    }
    BG_TRY(d_pages.alloc(pages.size() * sizeof(PqDevPage)));
    BG_TRY(copy_h2d(c, d_pages.p, pages.data(), pages.size() * sizeof(PqDevPage)));
    BG_TRY(d_min.alloc((size_t)(nblocks + 1) * 8));
    BG_TRY(d_widths.alloc((size_t)(nblocks + 1) * 4));
    BG_TRY(d_bytes.alloc((size_t)(nblocks + 1) * 4));
    BG_TRY(d_sums.alloc((size_t)((nblocks + 1 + 4095) / 4096) * 4));
    BG_TRY(d_info.alloc((size_t)npages * sizeof(PqDevInfo)));
    const unsigned wgrid = (unsigned)((nblocks + kWaves - 1) / kWaves);
    BG_HIP(hipMemsetAsync(d_bytes.as<uint32_t>() + nblocks, 0, 4, c->stream));
    if (nblocks > 0) {
        hipLaunchKernelGGL(pq_delta_sizes_kernel, dim3(wgrid), dim3(kThreads), 0, c->stream, dense, d_pages.as<const PqDevPage>(), npages, (uint32_t)nblocks,
                           d_min.as<int64_t>(), d_widths.as<uint32_t>(), d_bytes.as<uint32_t>());
        BG_TRY(checked_launch());
    }
    BG_TRY(launch_scan_u32(c, d_bytes.as<uint32_t>(), nblocks + 1, d_sums.as<uint32_t>()));
    uint32_t total = 0;   // a row group of at most 2^27 rows stays below 2^32 bytes (at most 1038 per 128 values)
    BG_HIP(hipMemcpyAsync(&total, d_bytes.as<uint32_t>() + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    const size_t image_bytes = (((size_t)total + 7) & ~(size_t)7) + (size_t)kPageSlack * (size_t)(npages + 1);
    BG_TRY(s->own.alloc(image_bytes));
    hipLaunchKernelGGL(pq_delta_pages_kernel, dim3((unsigned)((npages + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, dense,
                       d_pages.as<const PqDevPage>(), npages, d_bytes.as<const uint32_t>(), s->own.as<uint8_t>(), d_info.as<PqDevInfo>());
    BG_TRY(checked_launch());
    if (nblocks > 0) {
        hipLaunchKernelGGL(pq_delta_pack_kernel, dim3(wgrid), dim3(kThreads), 0, c->stream, dense, d_pages.as<const PqDevPage>(), npages, (uint32_t)nblocks,
                           d_min.as<const int64_t>(), d_widths.as<const uint32_t>(), d_bytes.as<const uint32_t>(), d_info.as<const PqDevInfo>(),
                           s->own.as<uint8_t>());
        BG_TRY(checked_launch());
    }
    std::vector<PqDevInfo> info((size_t)npages);
    BG_TRY(copy_d2h(c, info.data(), d_info.p, info.size() * sizeof(PqDevInfo)));
    BG_HIP(hipStreamSynchronize(c->stream));
    s->image = s->own.as<const uint8_t>();
    s->off.resize((size_t)npages);
    s->len.resize((size_t)npages);
    s->used = 0;
    for (int64_t p = 0; p < npages; p++) {
        s->off[(size_t)p] = (int64_t)info[(size_t)p].off;
        s->len[(size_t)p] = info[(size_t)p].bytes;
        if ((size_t)(s->off[(size_t)p] + s->len[(size_t)p]) > s->used) s->used = (size_t)(s->off[(size_t)p] + s->len[(size_t)p]);
    }
    if (s->used > image_bytes) return fail(BOWGPU_ERR_HIP, "parquet: a page's values section lies outside the image");
    return 0;
}

}  // namespace

int pq_finish_chunk(Ctx *c, const PqGrid &g, const std::vector<uint32_t> &valid, const void *d_levels, const PqSections &s, int32_t codec, PqEncChunk *out) {
    const bool snappy = codec == kPqSnappy;
    bool mixed = false;
    for (int64_t p = 0; p < g.npages; p++) mixed |= valid[(size_t)p] != 0 && valid[(size_t)p] != (uint32_t)g.rows(p);
    const size_t level_bytes = (size_t)g.npages * g.level_bytes();
    uint8_t *h_levels = mixed ? out->levels.take(level_bytes) : nullptr;
    if (mixed) BG_TRY(copy_d2h(c, h_levels, d_levels, level_bytes));
    std::vector<int64_t> coff, clen;
    if (snappy) {
        BG_TRY(pq_snappy_chunk(c, s, &out->comp, &coff, &clen));
    } else {
        BG_TRY(copy_d2h(c, out->values.take(s.used), s.image, s.used));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    out->pages.resize((size_t)g.npages);
    for (int64_t p = 0; p < g.npages; p++) {
        PqwPage &pg = out->pages[(size_t)p];
        pg.rows = (int32_t)g.rows(p);
        pg.valid = (int32_t)valid[(size_t)p];
        pg.level_bits = mixed ? h_levels + (size_t)p * g.level_bytes() : nullptr;
        pg.values = snappy ? nullptr : out->values.take(0) + s.off[(size_t)p];
        pg.value_bytes = s.len[(size_t)p];
        pg.comp = snappy ? out->comp.take(0) + coff[(size_t)p] : nullptr;
        pg.comp_bytes = snappy ? clen[(size_t)p] : 0;
    }
    return 0;
}

int pq_encode_chunk(Ctx *c, const bowgpu_col &col, int64_t a, int64_t b, int32_t page_rows, int32_t encoding, int32_t codec, bool minmax, PqEncChunk *out) {
    const PqGrid g(b - a, page_rows);
    const bool is_float = col.type == BOWGPU_FLOAT64;
    // (each step's device buffers live until the hand-over has drained the stream; they go back to the block cache in this order)
    DevBuf svals, sbits;
    DevCol dk;
    BG_TRY(stage_chunk(c, col, a, b, &svals, &sbits, &dk));
    DevBuf d_levels, d_counts;
    std::vector<uint32_t> counts;
    int64_t m = 0;
    BG_TRY(page_levels(c, dk, g, &d_levels, &d_counts, &counts, &m));
    MaskWork mw;
    DevBuf dvals, dbits;
    const uint64_t *dense = nullptr;
    BG_TRY(compact_valid(c, dk, m, &mw, &dvals, &dbits, &dense));
    DevBuf d_rec;
    std::vector<uint64_t> rec;
    if (minmax && m > 0) BG_TRY(launch_minmax(c, is_float, dense, m, &d_rec, &rec));
    PqSections s;
    out->dict.clear();
    if (encoding == kPqEncRleDict) {   // a chunk without a value, or with more distinct patterns than the cap, is written PLAIN
        bool fallback = m == 0;
        if (!fallback) BG_TRY(pq_dict_chunk(c, dense, m, counts, &out->dict, &s, &fallback));
        if (fallback) encoding = kPqEncPlain;
    }
    out->encoding = encoding;
    if (encoding == kPqEncPlain) plain_sections(dense, counts, &s);
    else if (encoding == kPqEncDelta) BG_TRY(delta_sections(c, dense, counts, &s));
    BG_TRY(pq_finish_chunk(c, g, counts, d_levels.p, s, codec, out));
    out->stats = PqwStats();
    out->stats.null_count = g.n - m;
    if (!rec.empty()) fold_minmax(rec, is_float, &out->stats);   // the hand-over has drained the stream: the records have landed
    return 0;
}

}  // namespace bowgpu
