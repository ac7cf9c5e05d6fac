// sort.hip — Bow.SortByCol on the device (reference bowsort.go:10-41): stable LSD radix argsort of one Int64 / Float64 column and the
// gather that moves the other columns.  Hand-written for gfx950 (wave64); host orchestration in sort_api.cpp.
//
//   sort_hist_kernel       ONE read of the key: the eight 8-bit digit histograms of its image, "is some key[i] < key[i-1]", NaN seen
//   per radix pass         sort_tile_hist_kernel (digit counts per 4096-row tile, digit-major) -> exclusive scan over (digit, tile)
//                          -> sort_scatter_kernel (stable: ranks by ballot matching inside a wave, waves combined in wave order in LDS,
//                          the tile staged in LDS in digit order so that global stores leave in runs per digit)
//   gather_kernel          out[j] = in[idx[j]] for up to kMoveCols columns; a wave owns its 64-bit validity word.  The one gather of the
//                          library: the sort's permutation, a caller's indices (bowgpu_take), the join's pairs with their "no row"
//
// Every count is an integer added in an order-free way (LDS / global atomics) or scanned in a fixed order; the position of a row
// after a pass is a function of the keys alone, never of scheduling.
#include <type_traits>

#include "common.h"
#include "key_image.h"
#include "wave_scan.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 16;
constexpr int kTile = kThreads * kItems;   // rows per scatter tile
constexpr int kWaveRows = kTile / kWaves;  // consecutive rows of a tile that one wave ranks
static_assert(kTile == kSortTileRows, "sort_api.cpp sizes the tile histograms with kSortTileRows");

// mode 0 / 1: src holds raw Int64 / Float64 keys; 2: images
__device__ __forceinline__ uint64_t load_image(const uint64_t *src, int64_t i, int mode) {
    const uint64_t v = src[i];
    return mode == 2 ? v : key_image(v, mode);
}

// one LDS counter bump per row - or one per wave when every row of the wave has the same digit (the high bytes of timestamps)
__device__ __forceinline__ void count_digit(uint32_t *h, uint32_t d, bool valid, int lane) {
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    const unsigned long long vm = __ballot(valid);
    if (__all(!valid || d == d0)) {
        if (lane == 0 && valid) atomicAdd(&h[d0], (uint32_t)__popcll(vm));   // (rows ascend with the lane: lane 0 is valid when any lane is)
    } else if (valid) {
        atomicAdd(&h[d], 1u);
    }
}

// exclusive scan of one value per thread over the workgroup (kThreads threads); wtot: kWaves LDS words
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wtot, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v, lane);
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) {
        const uint32_t x = wtot[i];
        if (i < w) base += x;
        t += x;
    }
    *total = t;
    __syncthreads();
    return base + incl - v;
}

// ---------------------------------------------------------------- histogram + checks: one read of the key
// hist: [8][256] digit counts of the images (digit p = bits 8p .. 8p+7); flags[0] |= 1: some key[i] < key[i-1]; flags[1] |= 1: a NaN.
// img_out (nullable): the images, for a key that is read over the host link (so that the passes do not read it there again).
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const uint64_t *key, int64_t n, int is_float, uint32_t *hist, uint32_t *flags,
                                                             uint64_t *img_out) {
    __shared__ uint32_t h[8 * 256];
    for (int j = threadIdx.x; j < 8 * 256; j += kThreads) h[j] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    bool unsorted = false, nan = false;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t rounds = (n + stride - 1) / stride;
    int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t r = 0; r < rounds; r++, i += stride) {   // (every lane runs every round: the ballots below need whole waves)
        const bool valid = i < n;
        uint64_t bits = 0;
        if (valid) bits = key[i];
        const uint64_t img = key_image(bits, is_float);
        if (is_float && valid) nan |= is_nan_bits(bits);
        uint64_t prev = __shfl_up(img, 1);   // the neighbour: the lane below, or the last row of the 64 rows before
        if (lane == 0 && valid && i > 0) prev = key_image(key[i - 1], is_float);
        if (valid && i > 0) unsorted |= img < prev;
        if (img_out && valid) img_out[i] = img;
#pragma unroll
        for (int p = 0; p < 8; p++) count_digit(h + 256 * p, (uint32_t)(img >> (8 * p)) & 255u, valid, lane);
    }
    if (__any(unsorted) && lane == 0) atomicOr(&flags[0], 1u);
    if (__any(nan) && lane == 0) atomicOr(&flags[1], 1u);
    __syncthreads();
    for (int j = threadIdx.x; j < 8 * 256; j += kThreads) {
        const uint32_t v = h[j];
        if (v) atomicAdd(&hist[j], v);
    }
}

// ---------------------------------------------------------------- one radix pass
// tile_hist[d * ntiles + tile] = rows of the tile whose digit is d: scanned in that order it is the first output position of the
// tile's rows with digit d (all smaller digits of every tile, then the same digit of the earlier tiles: a stable scatter)
__global__ __launch_bounds__(kThreads) void sort_tile_hist_kernel(const uint64_t *src, int mode, int64_t n, int shift, uint32_t *tile_hist,
                                                                  int64_t ntiles) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll 4
    for (int k = 0; k < kItems; k++) {
        const int64_t i = base + k * kThreads + threadIdx.x;
        const bool valid = i < n;
        uint32_t d = 0;
        if (valid) d = (uint32_t)(load_image(src, i, mode) >> shift) & 255u;
        count_digit(h, d, valid, lane);
    }
    __syncthreads();
    tile_hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of m 32-bit counts in place, in three launches (m = 256 * ntiles; the total is n < 2^31)
constexpr int kScanItems = 16;
constexpr int kScanBlock = kThreads * kScanItems;
__global__ __launch_bounds__(kThreads) void sort_scan_sums_kernel(const uint32_t *v, int64_t m, uint32_t *sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) if (base + k < m) s += v[base + k];
    uint32_t total;
    (void)block_exclusive_scan(s, wtot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kThreads) void sort_scan_top_kernel(uint32_t *sums, int64_t nb) {
    __shared__ uint32_t wtot[kWaves];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kThreads) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t x = b < nb ? sums[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(x, wtot, &total);
        if (b < nb) sums[b] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(kThreads) void sort_scan_apply_kernel(uint32_t *v, int64_t m, const uint32_t *sums) {
    __shared__ uint32_t wtot[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
    uint32_t x[kScanItems];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        x[k] = base + k < m ? v[base + k] : 0u;
        s += x[k];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_exclusive_scan(s, wtot, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < m) v[base + k] = run;
        run += x[k];
    }
}

// The stable scatter of one tile.  Wave w ranks rows [w * kWaveRows, (w + 1) * kWaveRows) of the tile, 64 consecutive rows at a
// time: a row's rank among the rows of its digit is (rows of that digit in the waves below) + (in this wave's earlier rounds) + (in
// the lanes below), i.e. its position in row order - stability.  tile_base: the scanned tile_hist.
__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(const uint64_t *src, int mode, const uint32_t *src_idx, int64_t n, int shift,
                                                                const uint32_t *tile_base, int64_t ntiles, uint64_t *dst, uint32_t *dst_idx) {
    __shared__ uint64_t skey[kTile];
    __shared__ uint32_t sidx[kTile];
    __shared__ uint32_t whist[kWaves * 256];   // per wave and digit: rows counted so far, then the first staged slot of that wave's rows
    __shared__ uint32_t gdelta[256];           // per digit: (first output position of the tile's rows) - (their first staged slot), mod 2^32
    __shared__ uint32_t wtot[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    for (int j = threadIdx.x; j < kWaves * 256; j += kThreads) whist[j] = 0;
    __syncthreads();

    uint64_t img[kItems];
    uint32_t idx[kItems];
    uint32_t rank[kItems];
    volatile uint32_t *my = whist + 256 * w;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const int64_t i = tile0 + w * kWaveRows + k * 64 + lane;
        const bool valid = i < n;
        img[k] = 0;
        idx[k] = 0;
        if (valid) {
            img[k] = load_image(src, i, mode);
            idx[k] = src_idx ? src_idx[i] : (uint32_t)i;
        }
        const uint32_t d = (uint32_t)(img[k] >> shift) & 255u;
        unsigned long long m = __ballot(valid);   // the lanes whose row has this lane's digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(valid && bit);
            m &= bit ? bal : ~bal;
        }
        const uint32_t lower = (uint32_t)__popcll(m & below);
        uint32_t before = 0;
        if (valid) before = my[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && lower == 0) my[d] = before + (uint32_t)__popcll(m);   // one lane per digit present; the wave's LDS accesses keep program order
        __builtin_amdgcn_wave_barrier();
        rank[k] = before + lower;
    }
    __syncthreads();
    {   // thread t = digit t: the waves' counts become slots
        const int d = threadIdx.x;
        uint32_t cnt[kWaves], total = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) { cnt[i] = whist[256 * i + d]; total += cnt[i]; }
        uint32_t all;
        uint32_t slot = block_exclusive_scan(total, wtot, &all);   // first staged slot of digit d
        gdelta[d] = tile_base[(int64_t)d * ntiles + blockIdx.x] - slot;
#pragma unroll
        for (int i = 0; i < kWaves; i++) { whist[256 * i + d] = slot; slot += cnt[i]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const int64_t i = tile0 + w * kWaveRows + k * 64 + lane;
        if (i < n) {
            const uint32_t d = (uint32_t)(img[k] >> shift) & 255u;
            const uint32_t s = whist[256 * w + d] + rank[k];
            if (s < (uint32_t)kTile) { skey[s] = img[k]; sidx[s] = idx[k]; }
        }
    }
    __syncthreads();
    const int64_t rows = n - tile0 < kTile ? n - tile0 : kTile;
    for (int j = threadIdx.x; j < rows; j += kThreads) {
        const uint64_t v = skey[j];
        const uint32_t d = (uint32_t)(v >> shift) & 255u;
        const uint32_t o = gdelta[d] + (uint32_t)j;
        if ((int64_t)o < n) { dst[o] = v; dst_idx[o] = sidx[j]; }
    }
}

// out[i] = idx[i] as 64 bits: uint32_t (the sort's row numbers) zero-extends, int32_t (the join's) sign-extends so that -1 stays -1
template <typename SrcT>
__global__ __launch_bounds__(kThreads) void widen_kernel(const SrcT *idx, int64_t n, int64_t *out) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = (int64_t)idx[i];
}

// ---------------------------------------------------------------- gather
// out[j] = col[idx[j]] for every column of the group: the index is read once.  A wave covers rows 64q .. 64q + 63 and stores their
// validity word whole (bits of rows >= n_idx: 0); null slots hold 0.  Three instantiations:
//   <uint32_t, false>  the sort's own permutation                  } an index outside [0, length) raises *bad and reads nothing
//   <int64_t, false>   a caller's indices (bowgpu_take)            }
//   <int32_t, true>    the join's: an index < 0 is "no row" and gives a null slot, every other one is in range (join_expand_kernel
//                      wrote them); on a "no row" row the column key_slot reads the second source through idx2.  Its argument block
//                      is GatherNoRowArgs; the other two take GatherArgs and hold no trace of the second source
template <typename IdxT, bool kNoRow>
__global__ __launch_bounds__(kThreads) void gather_kernel(std::conditional_t<kNoRow, GatherNoRowArgs, GatherArgs> a, const IdxT *idx) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t rounds = (a.n_idx + stride - 1) / stride;
    uint32_t nulls[kMoveCols] = {};
    bool bad = false;
    int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t r = 0; r < rounds; r++, j += stride) {   // (every lane runs every round: the ballots below need whole waves)
        bool in = j < a.n_idx;
        std::conditional_t<kNoRow, int32_t, int64_t> p = kNoRow ? -1 : 0, p2 = -1;
        if (in) {
            p = idx[j];
            if constexpr (kNoRow) {
                if (a.key_slot >= 0 && p < 0) p2 = a.idx2[j];
            } else if (p < 0 || p >= a.length) {   // (the library's own permutation never trips this: it guards the reads all the same)
                bad = true;
                p = -1;
            }
        }
#pragma unroll
        for (int c = 0; c < kMoveCols; c++) {
            if (c < a.cols.ncols) {
                const uint64_t *vals = a.cols.values[c];
                const uint32_t *vb = a.cols.vbits[c];
                int64_t vb0 = a.cols.vbit0[c], row = p;
                if constexpr (kNoRow) {
                    const bool second = c == a.key_slot && p < 0;
                    vals = second ? a.values2 : vals;
                    vb = second ? a.vbits2 : vb;
                    vb0 = second ? a.vbit02 : vb0;
                    row = second ? p2 : p;
                }
                bool valid = in && row >= 0;
                uint64_t v = 0;
                if (valid && vb) {
                    const int64_t bit = vb0 + row;
                    valid = (vb[bit >> 5] >> (bit & 31)) & 1u;
                }
                if (valid) v = vals[row];
                if (in) a.cols.out_values[c][j] = v;
                const unsigned long long word = __ballot(valid);
                const unsigned long long rows = __ballot(in);
                if (lane == 0 && rows) {
                    // whole 64-bit words, ceil(n_idx / 64) of them: at most 8 * ceil(n / 64) <= ((ceil(n / 8) + 3) & ~3) + 4 bytes, which
                    // is what devout_prepare gives every output's validity working copy (equal when n % 64 is 1 .. 32)
                    a.cols.out_valid[c][j >> 6] = word;
                    nulls[c] += (uint32_t)__popcll(rows & ~word);
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kMoveCols; c++)
            if (c < a.cols.ncols && nulls[c]) atomicAdd(&a.null_counts[c], (unsigned long long)nulls[c]);
    }
    if constexpr (!kNoRow) {
        if (__any(bad) && lane == 0) atomicOr(a.bad, 1u);
    }
}

}  // namespace

int launch_sort_hist(Ctx *c, const uint64_t *key, int64_t n, int is_float, uint32_t *d_hist, uint32_t *d_flags, uint64_t *img_out) {
    hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)stream_grid(n, kThreads)), dim3(kThreads), 0, c->stream, key, n, is_float, d_hist, d_flags, img_out);
    BG_HIP(hipGetLastError());
    return 0;
}

// the three launches of the exclusive scan, for the radix passes and for filter.hip's tile counts
int launch_scan_u32(Ctx *c, uint32_t *v, int64_t m, uint32_t *sums) {
    const int64_t nb = (m + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(sort_scan_sums_kernel, dim3((unsigned)nb), dim3(kThreads), 0, c->stream, v, m, sums);
    hipLaunchKernelGGL(sort_scan_top_kernel, dim3(1), dim3(kThreads), 0, c->stream, sums, nb);
    hipLaunchKernelGGL(sort_scan_apply_kernel, dim3((unsigned)nb), dim3(kThreads), 0, c->stream, v, m, sums);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_sort_pass(Ctx *c, const uint64_t *src, int mode, const uint32_t *src_idx, int64_t n, int shift, uint32_t *tile_hist, uint32_t *sums,
                     uint64_t *dst, uint32_t *dst_idx) {
    const int64_t ntiles = (n + kTile - 1) / kTile;
    const int64_t m = 256 * ntiles;
    hipLaunchKernelGGL(sort_tile_hist_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, src, mode, n, shift, tile_hist, ntiles);
    BG_TRY(launch_scan_u32(c, tile_hist, m, sums));
    hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, src, mode, src_idx, n, shift, tile_hist, ntiles,
                       dst, dst_idx);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_widen(Ctx *c, const uint32_t *idx32, const int32_t *idx32s, int64_t n, int64_t *out) {
    const dim3 grid((unsigned)stream_grid(n, kThreads));
    if (idx32) hipLaunchKernelGGL((widen_kernel<uint32_t>), grid, dim3(kThreads), 0, c->stream, idx32, n, out);
    else hipLaunchKernelGGL((widen_kernel<int32_t>), grid, dim3(kThreads), 0, c->stream, idx32s, n, out);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_gather(Ctx *c, const GatherNoRowArgs &a, const GatherIdx &ix) {
    const dim3 grid((unsigned)stream_grid(a.n_idx, kThreads));
    const GatherArgs &plain = a;
    if (ix.u32) hipLaunchKernelGGL((gather_kernel<uint32_t, false>), grid, dim3(kThreads), 0, c->stream, plain, ix.u32);
    else if (ix.i64) hipLaunchKernelGGL((gather_kernel<int64_t, false>), grid, dim3(kThreads), 0, c->stream, plain, ix.i64);
    else hipLaunchKernelGGL((gather_kernel<int32_t, true>), grid, dim3(kThreads), 0, c->stream, a, ix.i32);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
