// parquet_dict.hip — RLE_DICTIONARY for bowgpu_parquet_write: the dictionary of one column chunk built on the device, and the
// chunk's values sections (bit width, one bit-packed run of dictionary indices per page).  Hand-written for gfx950 (wave64); called
// by pq_encode_chunk (parquet_encode.hip) with the chunk's dense values and page counts - pq_dict_chunk, declared in parquet_encode.h.
//
//   pq_dict_insert_kernel   the distinct 64-bit patterns of the dense values, capped.  A workgroup keeps the patterns it has met in a
//                           small LDS set, so that a value goes to global memory once per workgroup at the most while the set has
//                           room (a flag column: two candidates per workgroup).  Survivors go into one open-addressing table in global
//                           memory (kTableSlots slots, linear probing): a slot is read first and claimed by a 64-bit compare-and-swap
//                           only where it reads empty.  Whoever claims a slot takes the next entry number and leaves (pattern, slot)
//                           in the entry list; the entry that would pass the cap raises the overflow word instead, every thread
//                           looks at that word before each probe and leaves.
//   (the host: overflow -> the chunk is written PLAIN.  Else the entries, at most 512 KiB, are sorted as unsigned 64-bit integers -
//    the order is a rule of the contract, not of the arrival - and each entry's rank goes back up)
//   pq_dict_rank_kernel     slot_rank[slot of entry e] = rank of entry e
//   pq_dict_pack_kernel     one workgroup per 256 values of a page: each value looked up in the table (bounded; a miss raises a
//                           status bit and never spins), its rank OR-ed at `width` bits into the workgroup's LDS copy of its bytes,
//                           which lies at the offset inside an 8-byte word that it has in the image; aligned 8-byte stores, bytes at
//                           the two edges.  The first workgroup of a page writes the width byte and the run header in front.
//
// Every loop over the table is bounded by its size; nothing waits on another workgroup.  The table's layout depends on the arrival
// order, the file does not: a rank is a function of the value alone.  One pattern (all ones) marks an empty slot; as a value it
// lives in the extra slot kTableSlots.
#include <string.h>

#include <algorithm>
#include <numeric>

#include "parquet_encode.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kDictMax = BOWGPU_PARQUET_DICT_MAX;
constexpr uint32_t kTableSlots = 1u << 18;   // >= 2 * kDictMax: at most a quarter is taken when the cap is met; 2 MiB of patterns
constexpr uint64_t kEmpty = ~0ull;
constexpr int kSetSlots = 1024, kSetProbes = 4;   // the workgroup's LDS set: 8 KiB
constexpr int kPackValues = 256;                  // values per workgroup of the pack kernel: at most 512 bytes of indices
static_assert((kTableSlots & (kTableSlots - 1)) == 0 && kTableSlots >= 2 * kDictMax, "the table is a power of two of at least twice the cap");

struct PqDictCtl { uint32_t count, overflow, has_empty, status; };   // zeroed by the host
struct PqDictPage {      // one page of the chunk as the pack kernel sees it; entry [npages] closes the table (blk0 = workgroups in all)
    int64_t v0;          // first of the page's values in the dense array
    uint64_t off;        // of the page's values section in the image (8-byte aligned)
    int32_t count;       // its non-null values
    uint32_t blk0;       // workgroups of the earlier pages
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}
__device__ __forceinline__ uint32_t table_slot(uint64_t x) { return (uint32_t)(mix64(x) >> 32) & (kTableSlots - 1); }

// the entry number of a newly claimed slot; past the cap: the overflow word
__device__ __forceinline__ void new_entry(PqDictCtl *ctl, uint64_t *entries, uint32_t *eslot, uint64_t x, uint32_t slot) {
    const uint32_t e = atomicAdd(&ctl->count, 1u);
    if (e < kDictMax) { entries[e] = x; eslot[e] = slot; }
    else atomicExch(&ctl->overflow, 1u);
}

__device__ __forceinline__ void table_insert(unsigned long long *table, PqDictCtl *ctl, uint64_t *entries, uint32_t *eslot, uint64_t x) {
    uint32_t h = table_slot(x);
    for (uint32_t probe = 0; probe < kTableSlots; probe++) {
        if (__hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        // a slot only ever goes from empty to one pattern: what reads as a pattern is final, what reads as empty may be stale
        unsigned long long cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            cur = atomicCAS(&table[h], (unsigned long long)kEmpty, (unsigned long long)x);
            if (cur == kEmpty) { new_entry(ctl, entries, eslot, x, h); return; }
        }
        if (cur == x) return;
        h = (h + 1) & (kTableSlots - 1);
    }
    atomicExch(&ctl->overflow, 1u);   // (a full table: not reached below the cap)
}

__global__ __launch_bounds__(kThreads) void pq_dict_insert_kernel(const uint64_t *v, int64_t m, unsigned long long *table, PqDictCtl *ctl,
                                                                  uint64_t *entries, uint32_t *eslot) {
    __shared__ unsigned long long sset[kSetSlots];
    __shared__ uint32_t s_empty_seen;
    for (int j = threadIdx.x; j < kSetSlots; j += kThreads) sset[j] = kEmpty;
    if (threadIdx.x == 0) s_empty_seen = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        if (__hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // (no barrier behind this point)
        const uint64_t x = v[i];
        if (x == kEmpty) {   // the pattern that marks an empty slot: its own flag, once per workgroup while the set's word says so
            if (__hip_atomic_load(&s_empty_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u && atomicExch(&s_empty_seen, 1u) == 0u &&
                atomicExch(&ctl->has_empty, 1u) == 0u)
                new_entry(ctl, entries, eslot, x, kTableSlots);
            continue;
        }
        uint32_t hs = (uint32_t)mix64(x) & (kSetSlots - 1);
        bool seen = false, mine = false;
        for (int probe = 0; probe < kSetProbes && !seen && !mine; probe++) {
            unsigned long long cur = __hip_atomic_load(&sset[hs], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == kEmpty) cur = atomicCAS(&sset[hs], (unsigned long long)kEmpty, (unsigned long long)x);
            if (cur == kEmpty) mine = true;
            else if (cur == x) seen = true;
            hs = (hs + 1) & (kSetSlots - 1);
        }
        if (!seen) table_insert(table, ctl, entries, eslot, x);   // (this workgroup's first, or the set has no room near its slot)
    }
}

__global__ __launch_bounds__(kThreads) void pq_dict_rank_kernel(const uint32_t *eslot, const uint16_t *rank, uint32_t entries, uint16_t *slot_rank) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e < entries) slot_rank[eslot[e]] = rank[e];   // (eslot[e] <= kTableSlots: written by new_entry alone)
}

// the page of workgroup g: the last one whose blk0 is not above g (every page has at least one workgroup)
__device__ __forceinline__ int64_t page_of_group(const PqDictPage *pages, int64_t npages, uint32_t g) {
    int64_t lo = 0, hi = npages - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (pages[mid].blk0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__host__ __device__ inline uint32_t dict_run_header(int64_t count) { return (uint32_t)((((count + 7) >> 3) << 1) | 1); }   // < 2^21: at most 3 bytes
__host__ __device__ inline uint32_t dict_varint_len(uint32_t v) { return v < 0x80u ? 1u : v < 0x4000u ? 2u : 3u; }
// bytes in front of a page's indices: the width byte, and the run header where the page has a value
__host__ __device__ inline uint32_t dict_lead_bytes(int64_t count) { return count > 0 ? 1u + dict_varint_len(dict_run_header(count)) : 1u; }

constexpr int kPackBufWords = (7 + 4 + 2 * kPackValues + 7) / 8 + 1;   // up to 7 bytes of offset, the lead, 256 indices of width 16
__global__ __launch_bounds__(kThreads) void pq_dict_pack_kernel(const uint64_t *v, const PqDictPage *pages, int64_t npages, const unsigned long long *table,
                                                                const uint16_t *slot_rank, uint32_t width, uint32_t has_empty, PqDictCtl *ctl,
                                                                uint8_t *image) {
    __shared__ uint64_t sbuf[kPackBufWords];   // the workgroup's bytes, at the offset inside an 8-byte word that they have in the image
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const int64_t p = page_of_group(pages, npages, g);
    const PqDictPage pg = pages[p];
    const uint32_t j = g - pg.blk0;                                    // this workgroup's place in the page
    const int64_t first = (int64_t)j * kPackValues, left = (int64_t)pg.count - first;
    const uint32_t mine = left >= kPackValues ? (uint32_t)kPackValues : left > 0 ? (uint32_t)left : 0u;   // values of this workgroup
    const uint32_t lead_all = dict_lead_bytes(pg.count);
    const uint32_t lead = j == 0 ? lead_all : 0u;                      // the width byte and the run header go with the page's first
    const uint64_t dst = pg.off + (j == 0 ? 0u : (uint64_t)lead_all + (uint64_t)j * (kPackValues / 8) * width);
    const uint32_t s = (uint32_t)(dst & 7);
    const uint32_t len = lead + ((mine + 7u) >> 3) * width;            // (the last group of 8 is padded with zero bits)
    for (int k = (int)t; k < kPackBufWords; k += kThreads) sbuf[k] = 0;
    __syncthreads();
    uint32_t *words = reinterpret_cast<uint32_t *>(sbuf);
    if (t == 0 && lead) {   // (dst is the section's start here: s == 0)
        uint32_t h = width, at = 8;
        if (pg.count > 0) for (uint32_t r = dict_run_header(pg.count);; r >>= 7, at += 8) {
            h |= ((r & 0x7Fu) | (r >= 0x80u ? 0x80u : 0u)) << at;
            if (r < 0x80u) break;
        }
        atomicOr(&words[0], h);
    }
    if (t < mine) {
        const uint64_t x = v[pg.v0 + first + t];
        uint32_t rank = 0;
        bool found = false;
        if (x == kEmpty) {
            found = has_empty != 0;
            if (found) rank = slot_rank[kTableSlots];
        } else {
            uint32_t h = table_slot(x);
            for (uint32_t probe = 0; probe < kTableSlots; probe++) {
                const unsigned long long cur = table[h];
                if (cur == x) { found = true; rank = slot_rank[h]; break; }
                if (cur == kEmpty) break;
                h = (h + 1) & (kTableSlots - 1);
            }
        }
        if (!found) atomicOr(&ctl->status, 1u);
        const uint32_t pos = 8u * (s + lead) + t * width, wi = pos >> 5, sh = pos & 31u;   // rank < 2^width, width <= 16
        atomicOr(&words[wi], rank << sh);
        if (sh + width > 32u) atomicOr(&words[wi + 1], rank >> (32u - sh));
    }
    __syncthreads();
    // the copy's bytes [s, s + len) to the image: 8-byte word k of the copy is the aligned word at (dst - s) + 8 k
    uint8_t *gbase = image + (dst - s);
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(sbuf);
    const uint32_t end = s + len;
    for (uint32_t k = t; 8u * k < end; k += kThreads) {
        const uint32_t lo = 8u * k, hi = lo + 8u;
        if (lo >= s && hi <= end) {
            reinterpret_cast<uint64_t *>(gbase)[k] = sbuf[k];
        } else {   // a word shared with the neighbouring workgroup's bytes: its own bytes only
            const uint32_t k0 = lo > s ? lo : s, k1 = hi < end ? hi : end;
            for (uint32_t b = k0; b < k1; b++) gbase[b] = bytes[b];
        }
    }
}

}  // namespace

int pq_dict_chunk(Ctx *c, const uint64_t *dense, int64_t m, const std::vector<uint32_t> &counts, std::vector<uint64_t> *dict, PqSections *s, bool *fallback) {
    const int64_t npages = (int64_t)counts.size();
    DevBuf d_table, d_ctl, d_entries, d_eslot, d_rank, d_slot_rank, d_pages;
    BG_TRY(d_table.alloc(((size_t)kTableSlots + 1) * 8));
    BG_TRY(d_ctl.alloc(sizeof(PqDictCtl)));
    BG_TRY(d_entries.alloc((size_t)kDictMax * 8));
    BG_TRY(d_eslot.alloc((size_t)kDictMax * 4));
    BG_HIP(hipMemsetAsync(d_table.p, 0xFF, ((size_t)kTableSlots + 1) * 8, c->stream));
    BG_HIP(hipMemsetAsync(d_ctl.p, 0, sizeof(PqDictCtl), c->stream));
    hipLaunchKernelGGL(pq_dict_insert_kernel, dim3((unsigned)stream_grid(m, kThreads)), dim3(kThreads), 0, c->stream, dense, m, d_table.as<unsigned long long>(),
                       d_ctl.as<PqDictCtl>(), d_entries.as<uint64_t>(), d_eslot.as<uint32_t>());
    BG_HIP(hipGetLastError());
    PqDictCtl ctl;
    BG_TRY(copy_d2h(c, &ctl, d_ctl.p, sizeof ctl));
    BG_HIP(hipStreamSynchronize(c->stream));
    *fallback = ctl.overflow != 0 || ctl.count > kDictMax;
    if (*fallback) return 0;
    const uint32_t entries = ctl.count;
    if (entries == 0) return fail(BOWGPU_ERR_HIP, "parquet: the dictionary of %lld values came back empty", (long long)m);

    // ---- the order of the contract, and each entry's rank
    std::vector<uint64_t> ent(entries);
    BG_TRY(copy_d2h(c, ent.data(), d_entries.p, (size_t)entries * 8));
    BG_HIP(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> order(entries);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ent[x] < ent[y]; });
    std::vector<uint16_t> rank(entries);
    dict->resize(entries);
    for (uint32_t r = 0; r < entries; r++) {
        (*dict)[r] = ent[order[r]];
        rank[order[r]] = (uint16_t)r;
        if (r > 0 && (*dict)[r] == (*dict)[r - 1]) return fail(BOWGPU_ERR_HIP, "parquet: the dictionary holds a pattern twice");
    }
    BG_TRY(d_rank.alloc((size_t)entries * 2));
    BG_TRY(d_slot_rank.alloc(((size_t)kTableSlots + 1) * 2));
    BG_TRY(copy_h2d(c, d_rank.p, rank.data(), (size_t)entries * 2));
    hipLaunchKernelGGL(pq_dict_rank_kernel, dim3((entries + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, d_eslot.as<const uint32_t>(),
                       d_rank.as<const uint16_t>(), entries, d_slot_rank.as<uint16_t>());
    BG_HIP(hipGetLastError());

    // ---- the sections: sizes known from the counts and the width alone
    uint32_t width = 1;
    while (width < 16 && (1u << width) < entries) width++;
    std::vector<PqDictPage> pages((size_t)npages + 1);
    s->off.resize((size_t)npages);
    s->len.resize((size_t)npages);
    int64_t v0 = 0, groups = 0;
    uint64_t at = 0;
    for (int64_t p = 0; p <= npages; p++) {
        const int64_t cnt = p < npages ? counts[(size_t)p] : 0;
        pages[(size_t)p] = PqDictPage{v0, at, (int32_t)cnt, (uint32_t)groups};
        if (p == npages) break;
        const uint64_t bytes = dict_lead_bytes(cnt) + (uint64_t)((cnt + 7) >> 3) * width;
        s->off[(size_t)p] = (int64_t)at;
        s->len[(size_t)p] = (int64_t)bytes;
        s->used = (size_t)(at + bytes);   // (every section holds its width byte)
        at += (bytes + 7) & ~(uint64_t)7;
        v0 += cnt;
        groups += cnt > 0 ? (cnt + kPackValues - 1) / kPackValues : 1;
    }
    if (v0 != m) return fail(BOWGPU_ERR_HIP, "parquet: the page counts (%lld) and the dense values (%lld) disagree", (long long)v0, (long long)m);
    BG_TRY(s->own.alloc((size_t)at));
    s->image = s->own.as<const uint8_t>();
    BG_TRY(d_pages.alloc(pages.size() * sizeof(PqDictPage)));
    BG_TRY(copy_h2d(c, d_pages.p, pages.data(), pages.size() * sizeof(PqDictPage)));
    hipLaunchKernelGGL(pq_dict_pack_kernel, dim3((unsigned)groups), dim3(kThreads), 0, c->stream, dense, d_pages.as<const PqDictPage>(), npages,
                       d_table.as<const unsigned long long>(), d_slot_rank.as<const uint16_t>(), width, ctl.has_empty, d_ctl.as<PqDictCtl>(),
                       s->own.as<uint8_t>());
    BG_HIP(hipGetLastError());
    BG_TRY(copy_d2h(c, &ctl, d_ctl.p, sizeof ctl));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (ctl.status != 0) return fail(BOWGPU_ERR_HIP, "parquet: a value of the chunk is not in its dictionary");
    return 0;
}

}  // namespace bowgpu
