// snappy_encode.hip — the values sections of one column chunk compressed to raw Snappy streams on the device (the SNAPPY codec of
// bowgpu_parquet_write_codec).  Hand-written for gfx950 (wave64); called by pq_finish_chunk (parquet_encode.hip) on the values sections
// as they lie on the device (declared in parquet_encode.h); the page's preamble and its levels literal are the host's (parquet_write.cpp).
//
//   snenc_compress_kernel   one wavefront (one workgroup of 64) per fragment of kSnFrag bytes of a page's values section: the
//                           fragment in LDS, a hash table of 4-byte keys in LDS, the element stream built in LDS and stored with
//                           aligned 8-byte stores into the fragment's slot; its byte count
//   (the scan of the byte counts: sort.hip launch_scan_u32)
//   snenc_pages_kernel      one thread per page: (offset, bytes) of the page's stream in the packed image
//   snenc_pack_kernel       one thread per 8-byte word of the packed image: the slots' streams end to end
//
// A Snappy stream is a plain sequence of elements, so the streams of a page's fragments, one after the other, are one valid stream
// behind the host's preamble; a back-reference never leaves its fragment.  No atomics on global memory (the LDS table takes its
// entries with an LDS maximum, so that the entry left by 64 lanes is the same whatever order the hardware serves them in), no
// unaligned global access, every byte of the output a function of the input alone.
#include <string.h>

#include <vector>

#include "parquet_encode.h"

namespace bowgpu {

namespace {

constexpr int kSnFrag = 4096;                                            // input bytes one wavefront compresses
constexpr int kSnSlot = (kSnFrag + kSnFrag / 6 + 32 + 7) & ~7;           // what a fragment's stream may take: libsnappy's bound
constexpr int kSnHashBits = 11;                                          // 2048 entries: one per two input positions
constexpr int kSnThreads = 256;                                          // of the two helper kernels

struct SnPage {          // one page's values section in the image; entry [npages] closes the table (frag0 = fragments in all)
    uint64_t off;        // 8-byte aligned
    uint32_t bytes;
    uint32_t frag0;      // fragments of the earlier pages
};
struct SnPageOut { uint64_t off, bytes; };   // the page's stream in the packed image

// the page of fragment f: the last one whose frag0 is not above f (a page without a fragment shares its frag0 with the page behind it)
__device__ __forceinline__ int64_t page_of_frag(const SnPage *pages, int64_t npages, uint32_t f) {
    int64_t lo = 0, hi = npages - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (pages[mid].frag0 <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 4 / 8 bytes at any byte offset of an LDS array of 32-bit words (aligned reads only; up to 12 bytes from the offset's word on)
__device__ __forceinline__ uint32_t lds_u32_at(const uint32_t *w, uint32_t byte) {
    const uint32_t i = byte >> 2, sh = (byte & 3u) * 8u;
    return (uint32_t)(((uint64_t)w[i] | ((uint64_t)w[i + 1] << 32)) >> sh);
}
__device__ __forceinline__ uint64_t lds_u64_at(const uint32_t *w, uint32_t byte) {
    const uint32_t i = byte >> 2, sh = (byte & 3u) * 8u;
    const uint64_t a = w[i], b = w[i + 1], c = w[i + 2];
    return (uint64_t)(uint32_t)((a | (b << 32)) >> sh) | ((uint64_t)(uint32_t)((b | (c << 32)) >> sh) << 32);
}

// the literal in[from, from + n) at out[o ..): its tag by lane 0, its bytes by all lanes; returns the position behind it
__device__ __forceinline__ uint32_t emit_literal(uint8_t *out, uint32_t o, const uint8_t *in, uint32_t from, uint32_t n, int lane) {
    if (n == 0) return o;
    const uint32_t tag = n <= 60 ? 1u : n <= 256 ? 2u : 3u;   // (a fragment holds at most 4096 bytes: no longer form)
    if (lane == 0) {
        if (tag == 1) out[o] = (uint8_t)((n - 1) << 2);
        else if (tag == 2) { out[o] = 60 << 2; out[o + 1] = (uint8_t)(n - 1); }
        else { out[o] = 61 << 2; out[o + 1] = (uint8_t)(n - 1); out[o + 2] = (uint8_t)((n - 1) >> 8); }
    }
    for (uint32_t i = (uint32_t)lane; i < n; i += 64u) out[o + tag + i] = in[from + i];
    return o + tag + n;
}

__global__ __launch_bounds__(64) void snenc_compress_kernel(const uint8_t *image, const SnPage *pages, int64_t npages, uint8_t *slots, uint32_t *frag_bytes) {
    __shared__ uint64_t sin[kSnFrag / 8 + 2];    // the fragment, and 16 bytes that the wide compares may read past its end
    __shared__ uint64_t sout[kSnSlot / 8];       // its stream
    __shared__ uint32_t stab[1 << kSnHashBits];  // hash of 4 bytes -> 1 + the last position probed that held them (0: none)
    const int lane = threadIdx.x;
    const uint32_t f = blockIdx.x;
    const int64_t pi = page_of_frag(pages, npages, f);
    const SnPage pg = pages[pi];
    const uint32_t start = (f - pg.frag0) * (uint32_t)kSnFrag;          // (below pg.bytes: the page has this fragment)
    const uint32_t len = pg.bytes - start < (uint32_t)kSnFrag ? pg.bytes - start : (uint32_t)kSnFrag;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(image + pg.off + start);   // 8-byte aligned; read up to the next multiple of 8
    for (uint32_t j = (uint32_t)lane; j < (uint32_t)(kSnFrag / 8 + 2); j += 64u) sin[j] = 8u * j < len ? src[j] : 0;
    for (uint32_t j = (uint32_t)lane; j < (1u << kSnHashBits); j += 64u) stab[j] = 0;
    __syncthreads();
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(sin);
    const uint8_t *in8 = reinterpret_cast<const uint8_t *>(sin);
    uint8_t *out8 = reinterpret_cast<uint8_t *>(sout);

    uint32_t pos = 0, lit = 0, o = 0;   // wave-uniform: the next position to probe, the start of the pending literal, bytes of stream
    while (pos + 4u <= len) {
        // ---- 64 consecutive positions: the value 8 bytes back (the period of the columns' values), else the table's candidate
        const uint32_t p = pos + (uint32_t)lane;
        bool hit = false;
        uint32_t cand = 0;
        if (p + 4u <= len) {
            const uint32_t key = lds_u32_at(in32, p);
            const uint32_t h = (key * 0x1e35a7bdu) >> (32 - kSnHashBits);
            const uint32_t t = stab[h];
            atomicMax(&stab[h], p + 1u);
            if (p >= 8u && lds_u32_at(in32, p - 8u) == key) { hit = true; cand = p - 8u; }
            // (behind a match the probing goes on inside the 64 positions entered last: an entry may lie at or behind p)
            else if (t != 0u && t - 1u < p && lds_u32_at(in32, t - 1u) == key) { hit = true; cand = t - 1u; }
        }
        const unsigned long long any = __ballot(hit);
        if (any == 0ull) { pos += 64u; continue; }
        const int first = __ffsll((long long)any) - 1;
        const uint32_t m = pos + (uint32_t)first, dist = m - (uint32_t)__shfl((int)cand, first);
        // ---- the match extended: 8 bytes a lane, 512 a round, up to the fragment's end (it may overlap its own source)
        uint32_t L = 4;
        for (;;) {
            const uint32_t q = m + L + 8u * (uint32_t)lane;
            uint32_t eq = 0;
            if (q < len) {
                const uint64_t x = lds_u64_at(in32, q) ^ lds_u64_at(in32, q - dist);
                eq = x ? (uint32_t)(__ffsll((long long)x) - 1) >> 3 : 8u;
                if (q + eq > len) eq = len - q;
            }
            const unsigned long long part = __ballot(eq != 8u);
            if (part == 0ull) { L += 512u; continue; }
            const int stop = __ffsll((long long)part) - 1;
            L += 8u * (uint32_t)stop + (uint32_t)__shfl((int)eq, stop);
            break;
        }
        o = emit_literal(out8, o, in8, lit, m - lit, lane);
        // ---- copies of at most 64 bytes and never fewer than 4: full ones, then 60 + the rest where the rest alone would be 1..3
        const uint32_t nfull = L >= 68u ? (L - 68u) / 64u + 1u : 0u, rem = L - 64u * nfull;   // rem: 4 .. 67
        const bool split = rem > 64u;
        const uint32_t pieces = nfull + (split ? 2u : 1u), last = split ? rem - 60u : rem;
        const bool narrow = last <= 11u && dist < 2048u;   // the last piece in the 1-byte-offset form
        for (uint32_t e = (uint32_t)lane; e < pieces; e += 64u) {
            const uint32_t n = e < nfull ? 64u : e + 1u < pieces ? 60u : last;
            uint8_t *d = out8 + o + 3u * e;
            if (e + 1u == pieces && narrow) {
                d[0] = (uint8_t)(1u | ((n - 4u) << 2) | ((dist >> 8) << 5));
                d[1] = (uint8_t)dist;
            } else {
                d[0] = (uint8_t)(2u | ((n - 1u) << 2));
                d[1] = (uint8_t)dist;
                d[2] = (uint8_t)(dist >> 8);
            }
        }
        o += 3u * pieces - (narrow ? 1u : 0u);
        pos = m + L;
        lit = pos;
    }
    o = emit_literal(out8, o, in8, lit, len - lit, lane);
    __syncthreads();
    uint64_t *dst = reinterpret_cast<uint64_t *>(slots + (uint64_t)f * kSnSlot);
    for (uint32_t j = (uint32_t)lane; 8u * j < o; j += 64u) dst[j] = sout[j];
    if (lane == 0) frag_bytes[f] = o;
}

// scan: the exclusive scan of frag_bytes, nfrags + 1 entries (the last: all of them)
__global__ __launch_bounds__(kSnThreads) void snenc_pages_kernel(const SnPage *pages, int64_t npages, const uint32_t *scan, SnPageOut *out) {
    const int64_t p = (int64_t)blockIdx.x * kSnThreads + threadIdx.x;
    if (p >= npages) return;
    const uint32_t a = scan[pages[p].frag0], b = scan[pages[p + 1].frag0];
    out[p].off = a;
    out[p].bytes = b - a;
}

// packed: ceil(total / 8) words.  Every fragment's stream holds at least one byte, so the scan rises strictly.
__global__ __launch_bounds__(kSnThreads) void snenc_pack_kernel(const uint8_t *slots, const uint32_t *scan, uint32_t nfrags, uint32_t total, uint64_t *packed) {
    __shared__ uint32_t sfrag;
    const uint64_t d0 = (uint64_t)blockIdx.x * kSnThreads * 8u;
    if (threadIdx.x == 0) {   // the fragment of the workgroup's first byte
        uint32_t lo = 0, hi = nfrags - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (scan[mid] <= d0) lo = mid; else hi = mid - 1;
        }
        sfrag = lo;
    }
    __syncthreads();
    const uint64_t d = d0 + 8u * threadIdx.x;
    if (d >= total) return;
    uint32_t f = sfrag;
    while (scan[f + 1] <= d) f++;   // (d < total = scan[nfrags])
    uint64_t word = 0;
    if (d + 8u <= scan[f + 1]) {    // the word lies in one stream: two aligned words of its slot
        const uint64_t s = (uint64_t)f * kSnSlot + (d - scan[f]);
        const uint64_t *w = reinterpret_cast<const uint64_t *>(slots + (s & ~(uint64_t)7));
        const uint32_t sh = (uint32_t)(s & 7u) * 8u;
        word = sh ? (w[0] >> sh) | (w[1] << (64u - sh)) : w[0];   // (w[1]: inside the slot, or the 8 bytes behind the last one)
    } else {
        for (uint32_t k = 0; k < 8u && d + k < total; k++) {
            while (scan[f + 1] <= d + k) f++;
            word |= (uint64_t)slots[(uint64_t)f * kSnSlot + (d + k - scan[f])] << (8u * k);
        }
    }
    packed[d >> 3] = word;
}

}  // namespace

int pq_snappy_chunk(Ctx *c, const PqSections &s, PqHostBytes *out, std::vector<int64_t> *coff, std::vector<int64_t> *clen) {
    const std::vector<int64_t> &off = s.off, &len = s.len;
    const int64_t npages = (int64_t)off.size();
    coff->assign((size_t)npages, 0);
    clen->assign((size_t)npages, 0);
    std::vector<SnPage> pages((size_t)npages + 1);
    int64_t nfrags = 0;
    for (int64_t p = 0; p <= npages; p++) {
        const int64_t bytes = p < npages ? len[(size_t)p] : 0;
        pages[(size_t)p] = SnPage{p < npages ? (uint64_t)off[(size_t)p] : 0, (uint32_t)bytes, (uint32_t)nfrags};
        nfrags += (bytes + kSnFrag - 1) / kSnFrag;
    }
    if (nfrags == 0) {
        BG_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    // a row group of at most 2^27 rows: at most 2^30 bytes of values (DELTA: fewer than 9 a value), 2^18 fragments, streams below 2^31 bytes
    DevBuf d_pages, d_slots, d_bytes, d_sums, d_tab, d_packed;
    BG_TRY(d_pages.alloc(pages.size() * sizeof(SnPage)));
    BG_TRY(copy_h2d(c, d_pages.p, pages.data(), pages.size() * sizeof(SnPage)));
    BG_TRY(d_slots.alloc((size_t)nfrags * kSnSlot + 8));
    BG_TRY(d_bytes.alloc((size_t)(nfrags + 1) * 4));
    BG_TRY(d_sums.alloc((size_t)((nfrags + 1 + 4095) / 4096) * 4));
    BG_TRY(d_tab.alloc((size_t)npages * sizeof(SnPageOut)));
    BG_HIP(hipMemsetAsync(d_bytes.as<uint32_t>() + nfrags, 0, 4, c->stream));
    BG_HIP(hipMemsetAsync(d_slots.as<uint8_t>() + (size_t)nfrags * kSnSlot, 0, 8, c->stream));
    hipLaunchKernelGGL(snenc_compress_kernel, dim3((unsigned)nfrags), dim3(64), 0, c->stream, s.image, d_pages.as<const SnPage>(), npages, d_slots.as<uint8_t>(),
                       d_bytes.as<uint32_t>());
    BG_HIP(hipGetLastError());
    BG_TRY(launch_scan_u32(c, d_bytes.as<uint32_t>(), nfrags + 1, d_sums.as<uint32_t>()));
    hipLaunchKernelGGL(snenc_pages_kernel, dim3((unsigned)((npages + kSnThreads - 1) / kSnThreads)), dim3(kSnThreads), 0, c->stream, d_pages.as<const SnPage>(),
                       npages, d_bytes.as<const uint32_t>(), d_tab.as<SnPageOut>());
    BG_HIP(hipGetLastError());
    uint32_t total = 0;
    BG_HIP(hipMemcpyAsync(&total, d_bytes.as<uint32_t>() + nfrags, 4, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (total == 0 || (uint64_t)total > (uint64_t)nfrags * kSnSlot) return fail(BOWGPU_ERR_HIP, "parquet: the Snappy streams of a chunk hold %u bytes in %lld fragments", total, (long long)nfrags);
    const size_t words = ((size_t)total + 7) >> 3;
    BG_TRY(d_packed.alloc(words * 8));
    hipLaunchKernelGGL(snenc_pack_kernel, dim3((unsigned)((words + kSnThreads - 1) / kSnThreads)), dim3(kSnThreads), 0, c->stream, d_slots.as<const uint8_t>(),
                       d_bytes.as<const uint32_t>(), (uint32_t)nfrags, total, d_packed.as<uint64_t>());
    BG_HIP(hipGetLastError());
    std::vector<SnPageOut> tab((size_t)npages);
    BG_TRY(copy_d2h(c, out->take(total), d_packed.p, total));
    BG_TRY(copy_d2h(c, tab.data(), d_tab.p, tab.size() * sizeof(SnPageOut)));
    BG_HIP(hipStreamSynchronize(c->stream));
    for (int64_t p = 0; p < npages; p++) {
        const SnPageOut &t = tab[(size_t)p];
        const uint64_t n = (uint64_t)len[(size_t)p];
        if (t.off + t.bytes > total || t.bytes > 32 + n + n / 6 || (n == 0) != (t.bytes == 0))
            return fail(BOWGPU_ERR_HIP, "parquet: page %lld's Snappy stream (%llu bytes at %llu of %u, from %llu) is out of bounds", (long long)p,
                        (unsigned long long)t.bytes, (unsigned long long)t.off, total, (unsigned long long)n);
        (*coff)[(size_t)p] = (int64_t)t.off;
        (*clen)[(size_t)p] = (int64_t)t.bytes;
    }
    return 0;
}

}  // namespace bowgpu
