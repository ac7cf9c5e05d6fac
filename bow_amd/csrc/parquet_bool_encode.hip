// parquet_bool_encode.hip — the device side of bowgpu_parquet_write_bool for a Boolean column: rows [a, b) of one bit-packed
// column (one column chunk of one row group) turned into what the pages of a Parquet BOOLEAN column hold.  Hand-written for gfx950
// (wave64); the Int64 / Float64 twin is parquet_encode.hip, whose pq_finish_chunk takes this driver's sections over.  This is the inverse of the
// loader's deposit32 (parquet_decode.hip): there the dense value bits are spread to the valid rows, here they are taken out from
// between the null rows.
//
//   pq_bool_pages_kernel   ONE WORKGROUP of 256 threads PER PAGE, one pass over the page's two bit ranges.  A page is the unit whose
//                          bit positions depend on each other (the exclusive prefix of the valid counts), and a page of the default
//                          65536 rows is 1024 words of 64 rows: four trips of a workgroup, where one wavefront would take sixteen
//                          with nothing to overlap its loads.  A file of few pages still fills the device poorly, but at 1/4 byte a
//                          row the pass is short beside the staging and the file system either way.
//     per trip, a thread takes 64 rows: the validity word and the value word, each funnel-shifted onto row alignment from its own
//     bit offset (bitmap_word64; the two offsets differ once a host column has been staged); rows past the chunk's end are masked
//     out.  The value bits at the valid positions are compressed to the low end of a word (compress64: the parallel-suffix method,
//     six rounds of prefix XORs; a word without a null is its own piece).  The exclusive prefix of the popcounts - a wave scan and
//     the four wave totals in LDS - plus the bit position the earlier trips have reached gives the piece its place in the section.
//     Pieces are merged with LDS ORs into an image of the trip's words, which starts with the word the last trip left unfinished;
//     the words that are full go to the section with aligned 8-byte stores, the unfinished one is carried, and the last one is
//     stored with its padding bits 0.  Every byte of ceil(k / 64) words is written, so nothing depends on what the image held.
//     The same pass stores the page's levels words (what pq_page_levels_kernel of parquet_encode.hip writes) and leaves the counts
//     of its valid rows and of its valid-true rows: the validity is read once.
//
// No global atomics, no unaligned global access, no workgroup waits on another, every byte of the output a function of the
// input alone (an OR does not depend on who arrives first).
#include <string.h>

#include "bitmap_word.h"
#include "parquet_encode.h"
#include "wave_scan.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// the bits of x at the set positions of m, moved together at the low end in order (Hacker's Delight 7-4, 64 bits wide)
__device__ __forceinline__ unsigned long long compress64(unsigned long long x, unsigned long long m) {
    x &= m;
    unsigned long long mk = ~m << 1;   // the positions that have a 0 to their right are counted from here
#pragma unroll
    for (int i = 0; i < 6; i++) {
        unsigned long long mp = mk ^ (mk << 1);   // the parallel suffix: bit j = parity of the zeros of m below j
        mp ^= mp << 2;
        mp ^= mp << 4;
        mp ^= mp << 8;
        mp ^= mp << 16;
        mp ^= mp << 32;
        const unsigned long long mv = mp & m;     // the bits that move by 1 << i in this round
        m = (m ^ mv) | (mv >> (1 << i));
        const unsigned long long t = x & mv;
        x = (x ^ t) | (t >> (1 << i));
        mk &= ~mp;
    }
    return x;
}

// tbits / vbits: the chunk's value and validity words (vbits nullptr: every row valid), row 0 at bit tbit0 / vbit0; n rows.
// levels (nullptr with vbits): page p's words at p * (page_rows / 64).  image: the same layout, page p's values section from its
// first word on.  counts[2 p], counts[2 p + 1]: the page's valid rows and its valid rows that are true.
__global__ __launch_bounds__(kThreads) void pq_bool_pages_kernel(const uint32_t *tbits, int64_t tbit0, int64_t twords, const uint32_t *vbits, int64_t vbit0,
                                                                 int64_t vwords, int64_t n, int32_t page_rows, unsigned long long *levels,
                                                                 unsigned long long *image, uint32_t *counts) {
    __shared__ unsigned long long sbuf[kThreads + 2];   // the trip's words: [0] starts as the carried one; a piece may reach [kThreads]
    __shared__ uint32_t swave[kWaves];
    __shared__ uint32_t scnt[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t page = blockIdx.x, row0 = page * page_rows;
    const int words = page_rows >> 6;
    unsigned long long *out = image + page * words;
    uint32_t placed = 0;                  // bits of the section placed by the earlier trips (the same in every thread)
    unsigned long long carried = 0;       // the section's word they left unfinished (the same in every thread)
    uint32_t nvalid = 0, ntrue = 0;
    for (int j0 = 0; j0 < words; j0 += kThreads) {   // (every thread makes every trip: the barriers are the workgroup's)
        const int j = j0 + tid;
        const int64_t base = row0 + (int64_t)j * 64;
        unsigned long long v = 0, t = 0;
        if (j < words && base < n) {
            v = vbits ? bitmap_word64(vbits, vbit0, vwords, base) : ~0ull;
            const int64_t left = n - base;
            if (left < 64) v &= (1ull << left) - 1ull;   // (the padding of the last group of 8 is zero bits)
            t = bitmap_word64(tbits, tbit0, twords, base) & v;   // what lies under a null or past the end is dropped here
            if (levels) levels[page * words + j] = v;
        }
        const uint32_t pc = (uint32_t)__popcll(v);
        nvalid += pc;
        ntrue += (uint32_t)__popcll(t);
        const unsigned long long piece = v == ~0ull ? t : compress64(t, v);
        const uint32_t incl = wave_inclusive_scan(pc, lane);
        if (lane == 63) swave[w] = incl;
        sbuf[tid + 1] = 0;
        if (tid == 0) { sbuf[0] = carried; sbuf[kThreads + 1] = 0; }
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) {
            const uint32_t s = swave[i];
            before += i < w ? s : 0u;
            total += s;
        }
        const uint32_t at = (placed & 63u) + before + incl - pc;   // the piece's bit in the trip's image: below 64 + 64 * tid
        if (pc) {
            const uint32_t q = at >> 6, s = at & 63u;
            atomicOr(&sbuf[q], piece << s);
            if (s + pc > 64u) atomicOr(&sbuf[q + 1], piece >> (64u - s));   // (s > 0 here)
        }
        __syncthreads();
        const uint32_t full = ((placed & 63u) + total) >> 6;   // words completed by this trip: at most kThreads
        for (uint32_t k = (uint32_t)tid; k < full; k += kThreads) out[(placed >> 6) + k] = sbuf[k];
        carried = sbuf[full];
        placed += total;
        __syncthreads();   // the image and the wave totals are read before the next trip overwrites them
    }
    if (tid == 0 && (placed & 63u)) out[placed >> 6] = carried;   // placed < page_rows here: the word lies in the page's region
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nvalid += __shfl_xor(nvalid, o); ntrue += __shfl_xor(ntrue, o); }
    if (lane == 0) { scnt[0][w] = nvalid; scnt[1][w] = ntrue; }
    __syncthreads();
    if (tid == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) { a += scnt[0][i]; b += scnt[1][i]; }
        counts[2 * page] = a;
        counts[2 * page + 1] = b;
    }
}

}  // namespace

int pq_encode_bool_chunk(Ctx *c, const bowgpu_col &col, int64_t a, int64_t b, int32_t page_rows, int32_t codec, bool minmax, PqEncChunk *out) {
    const PqGrid g(b - a, page_rows);
    const int64_t n = g.n, npages = g.npages;
    const size_t page_bytes = g.level_bytes();   // of a page's levels words, and of its region in the values image: a multiple of 8
    out->stats = PqwStats();
    out->encoding = kPqEncPlain;
    out->dict.clear();
    out->pages.clear();
    if (n <= 0) return 0;
    // ---- the rows on the device: a view of the column, so a host column's staging is bounded by the row group
    bowgpu_col view = col;
    view.offset = col.offset + a;
    view.length = n;
    DevBoolCol dc;
    BG_TRY(devboolcol_prepare(c, &view, &dc));

    // ---- one pass: levels, sections, counts
    DevBuf d_levels;
    PqSections s;
    DevBuf d_counts;
    if (dc.v.words) BG_TRY(d_levels.alloc((size_t)npages * page_bytes));
    BG_TRY(s.own.alloc((size_t)npages * page_bytes));
    BG_TRY(d_counts.alloc((size_t)npages * 8));
    hipLaunchKernelGGL(pq_bool_pages_kernel, dim3((unsigned)npages), dim3(kThreads), 0, c->stream, dc.t.words, dc.t.bit0, dc.t.nwords, dc.v.words, dc.v.bit0,
                       dc.v.nwords, n, page_rows, d_levels.as<unsigned long long>(), s.own.as<unsigned long long>(), d_counts.as<uint32_t>());
    BG_HIP(hipGetLastError());
    std::vector<uint32_t> counts((size_t)npages * 2), valid((size_t)npages);
    BG_TRY(copy_d2h(c, counts.data(), d_counts.p, counts.size() * 4));
    BG_HIP(hipStreamSynchronize(c->stream));
    // ---- the values sections: ceil(k / 8) bytes at the start of each page's region, which begins 8-byte aligned
    int64_t m = 0, trues = 0;
    s.image = s.own.as<const uint8_t>();
    s.off.resize((size_t)npages);
    s.len.resize((size_t)npages);
    for (int64_t p = 0; p < npages; p++) {
        const int64_t rows = g.rows(p), k = counts[2 * (size_t)p];
        if (k > rows || counts[2 * (size_t)p + 1] > k) return fail(BOWGPU_ERR_HIP, "parquet: page %lld of a Boolean chunk counts %lld valid rows of %lld", (long long)p, (long long)k, (long long)rows);
        valid[(size_t)p] = (uint32_t)k;
        m += k;
        trues += counts[2 * (size_t)p + 1];
        s.off[(size_t)p] = (int64_t)((size_t)p * page_bytes);
        s.len[(size_t)p] = (k + 7) >> 3;
        if (k > 0) s.used = (size_t)(s.off[(size_t)p] + s.len[(size_t)p]);
    }

    // ---- statistics: false < true
    out->stats.null_count = n - m;
    if (minmax && m > 0) {
        out->stats.has_minmax = true;
        out->stats.min = trues < m ? 0 : 1;
        out->stats.max = trues > 0 ? 1 : 0;
    }
    return pq_finish_chunk(c, g, valid, d_levels.p, s, codec, out);
}

}  // namespace bowgpu
