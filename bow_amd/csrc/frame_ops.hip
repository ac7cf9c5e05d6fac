// frame_ops.hip — Bow.DropNils (reference bow.go:188-224), Bow.Diff (bowdiff.go:8-73) and Bow.Distinct (bowgetters.go:333-358) on the
// device: the three streaming kernels in front of the layers Sort and Filter already have.  Hand-written for gfx950 (wave64); host
// orchestration in frame_ops_api.cpp.
//
//   valid_mask_kernel      reads ONLY validity bitmaps: a lane forms the 64-bit word of its 64 rows from each selected column's bitmap
//                          (a funnel shift onto row alignment) and ANDs them; a wave is one tile of 4096 rows and leaves the tile
//                          records of filter_mask_kernel - the 64 words, the count, the span - for filter_stats_kernel, the scan and
//                          filter_scatter_kernel
//   diff_kernel            out[i] = col[i] - col[i-1] for up to kMoveCols columns: the previous row comes from the neighbour lane, the
//                          row in front of a wave's first row is one extra load; validity is v & ((v << 1) | carry) per 64-row word,
//                          stored whole
//   distinct_tail_kernel   over keys in sorted order: flags the LAST row of each group of equal keys, and leaves the same tile records
//
// No workgroup waits on another and nothing is accumulated across workgroups: the bytes are a function of the input.
#include "common.h"
#include "bitmap_word.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kFilterTileRows;
constexpr int kTileWords = kTile / 64;
static_assert(kTileWords == 64, "valid_mask_kernel forms a tile's words with one wave");

// bytes [8 W, 8 W + 8) of a caller's bitmap of nb bytes, any alignment
__device__ __forceinline__ unsigned long long mask_word64(const uint8_t *p, int64_t W, int64_t nb) {
    const int64_t b0 = W * 8;
    if ((reinterpret_cast<uintptr_t>(p) & 7) == 0 && b0 + 8 <= nb) return *reinterpret_cast<const unsigned long long *>(p + b0);
    unsigned long long x = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (b0 + k < nb) x |= (unsigned long long)p[b0 + k] << (8 * k);
    return x;
}

// one wave = one tile, lane = word of the tile
__global__ __launch_bounds__(kThreads) void valid_mask_kernel(ValidMaskArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    const int64_t tile = (int64_t)blockIdx.x * kWaves + w;
    if (tile >= ntiles) return;   // (the whole wave)
    const int64_t W = tile * kTileWords + lane, row0 = W * 64;
    unsigned long long word = 0;   // rows past the end: clear bits
    if (row0 < a.n) {
        word = a.n - row0 < 64 ? (1ull << (a.n - row0)) - 1ull : ~0ull;
#pragma unroll
        for (int c = 0; c < kValidMaskCols; c++)
            if (c < a.ncols) word &= bitmap_word64(a.vbits[c], a.vbit0[c], a.vwords[c], row0);
        if (a.and_mask) word &= mask_word64(a.and_mask, W, (a.n + 7) >> 3);
        if (a.accumulate) word &= a.t.mask[W];
    }
    a.t.mask[W] = word;
    uint32_t cnt = (uint32_t)__popcll(word), lo = 0xFFFFFFFFu, hi = 0;
    if (word) {
        lo = (uint32_t)(lane * 64 + __ffsll((long long)word) - 1);
        hi = (uint32_t)(lane * 64 + 63 - __clzll((long long)word));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) {
        a.t.tile_counts[tile] = cnt;
        a.t.tile_spans[tile] = cnt ? lo | (hi << 16) : 0u;   // (tile-relative, below 4096 each)
    }
}

// A wave takes kDiffWords consecutive 64-row words of every column of the group; all loads of a column are issued before any is used.
constexpr int kDiffWords = 4;
__global__ __launch_bounds__(kThreads) void diff_kernel(DiffArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t W0 = ((int64_t)blockIdx.x * kWaves + w) * kDiffWords;
    const int64_t i0 = W0 * 64;
    if (i0 >= a.n) return;   // (the whole wave)
#pragma unroll
    for (int c = 0; c < kMoveCols; c++) {
        if (c >= a.cols.ncols) continue;
        const uint64_t *vals = a.cols.values[c];
        const uint32_t *vb = a.cols.vbits[c];
        const int64_t vb0 = a.cols.vbit0[c];
        const bool is_float = (a.float_mask >> c) & 1u;
        uint64_t x[kDiffWords];
        uint32_t vw[kDiffWords];
#pragma unroll
        for (int k = 0; k < kDiffWords; k++) {
            const int64_t i = i0 + k * 64 + lane;
            x[k] = 0;
            vw[k] = ~0u;
            if (i < a.n) {
                x[k] = vals[i];
                if (vb) vw[k] = vb[(vb0 + i) >> 5];
            }
        }
        // the row in front of the wave's first row: one extra load (row 0 of the column has none: its carry is clear)
        uint64_t px = 0;
        uint32_t pv = 0;
        if (lane == 0 && i0 > 0) {
            px = vals[i0 - 1];
            pv = 1u;
            if (vb) pv = (vb[(vb0 + i0 - 1) >> 5] >> ((vb0 + i0 - 1) & 31)) & 1u;
        }
        unsigned long long carry = (unsigned long long)__builtin_amdgcn_readfirstlane(pv);
#pragma unroll
        for (int k = 0; k < kDiffWords; k++) {
            const int64_t i = i0 + k * 64 + lane;
            const bool in = i < a.n;
            const bool ok = in && ((vw[k] >> ((vb0 + i) & 31)) & 1u);
            const unsigned long long v = __ballot(ok);
            uint64_t prev = __shfl_up(x[k], 1);
            if (k > 0) {
                const uint64_t last = __shfl(x[k - 1], 63);
                if (lane == 0) prev = last;
            } else if (lane == 0) {
                prev = px;
            }
            const unsigned long long outv = v & ((v << 1) | carry);
            carry = v >> 63;
            uint64_t d = 0;   // a null slot holds 0
            if ((outv >> lane) & 1ull) {
                if (is_float) d = (uint64_t)__double_as_longlong(__dsub_rn(__longlong_as_double((long long)x[k]), __longlong_as_double((long long)prev)));
                else d = x[k] - prev;   // wraps, as Go's int64 does
            }
            if (in) __builtin_nontemporal_store(d, &a.cols.out_values[c][i]);
            if (lane == 0 && i0 + k * 64 < a.n) a.cols.out_valid[c][W0 + k] = outv;   // (rows >= n: clear bits)
        }
    }
}

// one workgroup = one tile; a wave flags kWaveWords consecutive words of it.  The next row comes from the neighbour lane, for lane 63
// from lane 0 of the word behind; the row behind a wave's last row is one extra load.
constexpr int kWaveWords = kTileWords / kWaves;
__global__ __launch_bounds__(kThreads) void distinct_tail_kernel(const uint64_t *s, int64_t n, int is_float, TileRecords t) {
    __shared__ uint32_t wcnt[kWaves], wlo[kWaves], whi[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kTile + (int64_t)w * kWaveWords * 64;
    uint64_t x[kWaveWords + 1];
#pragma unroll
    for (int k = 0; k < kWaveWords; k++) {
        const int64_t i = r0 + k * 64 + lane;
        x[k] = i < n ? s[i] : 0;
    }
    {
        const int64_t i = r0 + (int64_t)kWaveWords * 64;
        x[kWaveWords] = (lane == 0 && i < n) ? s[i] : 0;
    }
    uint32_t cnt = 0, lo = 0xFFFFFFFFu, hi = 0;   // wave-uniform
#pragma unroll
    for (int k = 0; k < kWaveWords; k++) {
        const int wi = w * kWaveWords + k;
        const int64_t i = r0 + k * 64 + lane;
        uint64_t next = __shfl_down(x[k], 1);
        const uint64_t first_behind = __shfl(x[k + 1], 0);
        if (lane == 63) next = first_behind;
        // Go's != on the map key: integer for Int64, IEEE for Float64 (-0.0 equals +0.0; no NaN gets here)
        const bool differ = is_float ? __longlong_as_double((long long)x[k]) != __longlong_as_double((long long)next) : x[k] != next;
        const bool flag = i < n && (i == n - 1 || differ);
        const unsigned long long word = __ballot(flag);
        if (lane == 0) t.mask[(int64_t)blockIdx.x * kTileWords + wi] = word;   // (every word of the tile is stored)
        if (word) {
            cnt += (uint32_t)__popcll(word);
            const uint32_t first = (uint32_t)(wi * 64 + __ffsll((long long)word) - 1), last = (uint32_t)(wi * 64 + 63 - __clzll((long long)word));
            lo = first < lo ? first : lo;
            hi = last > hi ? last : hi;
        }
    }
    if (lane == 0) { wcnt[w] = cnt; wlo[w] = lo; whi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, l = 0xFFFFFFFFu, h = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) {
            total += wcnt[i];
            l = wlo[i] < l ? wlo[i] : l;
            h = whi[i] > h ? whi[i] : h;
        }
        t.tile_counts[blockIdx.x] = total;
        t.tile_spans[blockIdx.x] = total ? l | (h << 16) : 0u;
    }
}

}  // namespace

int launch_valid_mask(Ctx *c, const ValidMaskArgs &a) {
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(valid_mask_kernel, dim3((unsigned)((ntiles + kWaves - 1) / kWaves)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_diff(Ctx *c, const DiffArgs &a) {
    const int64_t per_block = (int64_t)kWaves * kDiffWords * 64;
    hipLaunchKernelGGL(diff_kernel, dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_distinct_tail(Ctx *c, const uint64_t *s, int64_t n, int is_float, const TileRecords &t) {
    const int64_t ntiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(distinct_tail_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, s, n, is_float, t);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
