// filter.hip — Bow.Filter on the device (reference bowsetters.go:58-132): value-set predicates evaluated into a row bitmap, and the
// ordered compaction of the selected rows.  Hand-written for gfx950 (wave64); host orchestration in filter_api.cpp.
//
//   filter_mask_kernel     reads ONLY the predicate columns and the caller's bitmap: a wave forms the 64-bit result word of its 64 rows
//                          with a ballot and stores it whole; per tile of 4096 rows the selected count and the lowest / highest
//                          selected row
//   filter_stats_kernel    those records summed / reduced into the call's three numbers (a handful of order-free integer atomics)
//   exclusive scan         of the tile counts (sort.hip's three launches)
//   filter_scatter_kernel  one workgroup per tile: a kept row's output slot is (tile base) + (set bits of the tile's earlier words) +
//                          (set bits below its lane); lanes load only the rows they keep, a tile that keeps nothing reads its 64 mask
//                          words and nothing else; the rows of all columns of the group are loaded together and stored straight to
//                          their slots (dense runs per store instruction); validity bits pass through LDS
//
// No workgroup waits on another: ordering comes from launch boundaries alone.  Output validity words that lie inside one tile's run are
// stored whole; the at most two words a run shares with its neighbours are combined with atomic OR into a zeroed bitmap, so the bytes
// are a function of the input, never of scheduling.
#include "common.h"
#include "wave_scan.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kFilterTileRows;
constexpr int kTileWords = kTile / 64;          // mask words per tile
constexpr int kWaveWords = kTileWords / kWaves;  // consecutive words of a tile that one wave forms / moves
static_assert(kTileWords == 64, "filter_scatter_kernel scans a tile's word counts with one wave");

// Go's == on the boxed value (bowsetters.go:124-131): exact for Int64; IEEE for Float64 (NaN equals nothing, -0.0 equals +0.0)
__device__ __forceinline__ bool in_set(uint64_t x, const FilterPredDev &p) {
    bool hit = false;
    if (p.is_float) {
        const double xd = __longlong_as_double((long long)x);
        for (int j = 0; j < p.n_values; j++) hit |= xd == __longlong_as_double((long long)p.set[j]);
    } else {
        for (int j = 0; j < p.n_values; j++) hit |= x == p.set[j];
    }
    return hit;
}

// Eight words (512 rows) of a wave at a time: the first predicate's column - and its validity words, and the caller's bitmap - are
// loaded for all eight before any is looked at, so a lane has eight independent loads in flight; the later predicates read only the
// rows that are still selected.
constexpr int kMaskBatch = 8;
__global__ __launch_bounds__(kThreads) void filter_mask_kernel(FilterMaskArgs a) {
    __shared__ uint32_t wcnt[kWaves], wlo[kWaves], whi[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    const FilterPredDev &P0 = a.preds[0];
    const bool have0 = a.npreds > 0;
    uint32_t cnt = 0, lo = 0xFFFFFFFFu, hi = 0;   // wave-uniform: rows of this wave selected so far, the lowest / highest of them (tile-relative)
    for (int k0 = 0; k0 < kWaveWords; k0 += kMaskBatch) {
        uint64_t x0[kMaskBatch];
        uint32_t v0[kMaskBatch], am[kMaskBatch];
#pragma unroll
        for (int j = 0; j < kMaskBatch; j++) {
            const int64_t i = tile0 + (int64_t)(w * kWaveWords + k0 + j) * 64 + lane;
            const bool in = i < a.n;
            x0[j] = 0;
            v0[j] = ~0u;
            am[j] = ~0u;
            if (in && have0) x0[j] = P0.values[i];
            if (in && have0 && P0.vbits) v0[j] = P0.vbits[(P0.vbit0 + i) >> 5];
            if (in && a.and_mask) am[j] = a.and_mask[i >> 3];
        }
#pragma unroll
        for (int j = 0; j < kMaskBatch; j++) {
            const int wi = w * kWaveWords + k0 + j;
            const int64_t i = tile0 + (int64_t)wi * 64 + lane;
            bool sel = i < a.n && ((am[j] >> (i & 7)) & 1u);
            if (have0) {
                const bool valid = (v0[j] >> ((P0.vbit0 + i) & 31)) & 1u;
                sel = sel && (valid ? in_set(x0[j], P0) : P0.match_null != 0);
            }
            for (int p = 1; p < a.npreds; p++) {
                const FilterPredDev &P = a.preds[p];
                if (sel) {   // (a row some earlier predicate dropped is not read again)
                    bool valid = true;
                    if (P.vbits) {
                        const int64_t bit = P.vbit0 + i;
                        valid = (P.vbits[bit >> 5] >> (bit & 31)) & 1u;
                    }
                    sel = valid ? in_set(P.values[i], P) : P.match_null != 0;
                }
            }
            const unsigned long long word = __ballot(sel);
            if (lane == 0) a.t.mask[(int64_t)blockIdx.x * kTileWords + wi] = word;   // (rows >= n: clear bits; every word of the tile is stored)
            if (word) {
                cnt += (uint32_t)__popcll(word);
                const uint32_t first = (uint32_t)(wi * 64 + __ffsll((long long)word) - 1), last = (uint32_t)(wi * 64 + 63 - __clzll((long long)word));
                lo = first < lo ? first : lo;
                hi = last > hi ? last : hi;
            }
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
        a.t.tile_counts[blockIdx.x] = total;
        a.t.tile_spans[blockIdx.x] = l | (h << 16);   // (tile-relative, below 4096 each; meaningless where total == 0)
    }
}

// The call's selected count and its lowest / highest selected row from the per-tile records: one workgroup per 4096 tiles, so the
// global atomics (integer add / max: order-free) are a handful per call, not one set per tile.  stats: [0] count, [1] 2^32 - 1 - lowest
// row (so that the preset is all zeroes), [2] highest row, [3] workgroups done.  The workgroup that finishes last - it waits for nobody:
// it is the one whose ticket says so - hands the three numbers to the host's registered block by its own stores, which spares the call a
// copy command in front of its synchronise.
constexpr int kStatItems = 16;
__global__ __launch_bounds__(kThreads) void filter_stats_kernel(const uint32_t *counts, const uint32_t *spans, int64_t ntiles, uint32_t *stats,
                                                                uint32_t *host_out) {
    __shared__ uint32_t acc[3];
    if (threadIdx.x == 0) { acc[0] = 0; acc[1] = 0; acc[2] = 0; }
    __syncthreads();
    uint32_t total = 0, lo = 0xFFFFFFFFu, hi = 0;
    const int64_t t0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kStatItems;
#pragma unroll
    for (int k = 0; k < kStatItems; k++) {
        const int64_t t = t0 + k;
        if (t < ntiles) {
            const uint32_t cnt = counts[t];
            if (cnt) {   // (n < 2^31: rows and counts fit 32 bits)
                const uint32_t sp = spans[t], row0 = (uint32_t)t * (uint32_t)kTile;
                total += cnt;
                lo = min(lo, row0 + (sp & 0xFFFFu));
                hi = max(hi, row0 + (sp >> 16));
            }
        }
    }
    if (total) {
        atomicAdd(&acc[0], total);
        atomicMax(&acc[1], 0xFFFFFFFFu - lo);
        atomicMax(&acc[2], hi);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (acc[0]) {
            atomicAdd(&stats[0], acc[0]);
            atomicMax(&stats[1], acc[1]);
            atomicMax(&stats[2], acc[2]);
        }
        __threadfence();
        if (atomicAdd(&stats[3], 1u) == gridDim.x - 1) {
            __threadfence();
            host_out[0] = atomicAdd(&stats[0], 0u);
            host_out[1] = 0xFFFFFFFFu - atomicAdd(&stats[1], 0u);
            host_out[2] = atomicAdd(&stats[2], 0u);
        }
    }
}

// A tile's time is a chain of memory latencies, not bytes (measured: the same 1.4 ms at selectivity 0.5 and 0.99, whatever the staging),
// so the chain is kept short: the rows of ALL columns of the group are loaded together, half a tile at a time, and stored straight to
// their slots - the kept rows of 64 consecutive rows go to consecutive slots, so a wave's store instruction writes one dense run.
// Only the validity bits pass through LDS, behind the one barrier of the tile.  Nulls are not counted here: one atomic per wave on
// one address cost more than everything else in the kernel (measured); the host popcounts the finished bitmaps instead.
constexpr int kHalfWords = kWaveWords / 2;
__global__ __launch_bounds__(kThreads) void filter_scatter_kernel(FilterScatterArgs a) {
    __shared__ uint8_t sok[kMoveCols][kTile];   // validity of the tile's kept rows, per column, in output order
    __shared__ unsigned long long sword[kTileWords];
    __shared__ uint32_t sbase[kTileWords + 1];    // kept rows in the tile's earlier words; [kTileWords]: in the whole tile
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    if (w == 0) {
        const uint32_t incl = tile_word_bases(a.mask + (int64_t)blockIdx.x * kTileWords, lane, sword, sbase);
        if (lane == 63) sbase[kTileWords] = incl;
    }
    __syncthreads();
    const uint32_t total = sbase[kTileWords];
    if (total == 0) return;   // (the same in every thread of the workgroup)
    const int64_t base = (int64_t)a.tile_base[blockIdx.x];
    const int64_t end = base + total;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint64_t v[kMoveCols][kHalfWords];
        uint32_t okm[kMoveCols];
#pragma unroll
        for (int c = 0; c < kMoveCols; c++) {
            okm[c] = 0;
            if (c < a.cols.ncols) {
                const uint64_t *vals = a.cols.values[c];
                const uint32_t *vb = a.cols.vbits[c];
                const int64_t vb0 = a.cols.vbit0[c];
#pragma unroll
                for (int k = 0; k < kHalfWords; k++) {
                    const int wi = w * kWaveWords + h * kHalfWords + k;
                    const int64_t i = tile0 + (int64_t)wi * 64 + lane;
                    bool ok = (sword[wi] >> lane) & 1ull;   // lanes load only the rows they keep
                    if (ok && vb) {
                        const int64_t bit = vb0 + i;
                        ok = (vb[bit >> 5] >> (bit & 31)) & 1u;
                    }
                    v[c][k] = 0;   // a null slot holds 0
                    if (ok) v[c][k] = vals[i];
                    okm[c] |= (uint32_t)ok << k;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kHalfWords; k++) {
            const int wi = w * kWaveWords + h * kHalfWords + k;
            const unsigned long long word = sword[wi];
            if ((word >> lane) & 1ull) {
                const uint32_t slot = sbase[wi] + (uint32_t)__popcll(word & below);
#pragma unroll
                for (int c = 0; c < kMoveCols; c++) {
                    if (c < a.cols.ncols) {
                        a.cols.out_values[c][base + slot] = v[c][k];
                        sok[c][slot] = (uint8_t)((okm[c] >> k) & 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    // output validity, by the output's own 64-row words: one inside the tile's run is stored whole, the at most two shared with the
    // neighbouring tiles' runs are ORed into the zeroed bitmap
#pragma unroll
    for (int c = 0; c < kMoveCols; c++) {
        if (c < a.cols.ncols) {
            unsigned long long *ob = a.cols.out_valid[c];
            for (int64_t W = (base >> 6) + w; W <= ((end - 1) >> 6); W += kWaves) {
                const int64_t o = W * 64 + lane;
                const bool in = o >= base && o < end;
                const bool ok = in && sok[c][o - base] != 0;
                const unsigned long long bits = __ballot(ok), rows = __ballot(in);
                if (lane == 0) {
                    if (rows == ~0ull) ob[W] = bits;
                    else if (bits) atomicOr(&ob[W], bits);
                }
            }
        }
    }
}

}  // namespace

int launch_filter_stats(Ctx *c, const TileRecords &t, int64_t ntiles) {
    const int64_t per_block = (int64_t)kThreads * kStatItems;
    hipLaunchKernelGGL(filter_stats_kernel, dim3((unsigned)((ntiles + per_block - 1) / per_block)), dim3(kThreads), 0, c->stream, t.tile_counts,
                       t.tile_spans, ntiles, t.stats, t.host_stats);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_filter_mask(Ctx *c, const FilterMaskArgs &a) {
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    return launch_filter_stats(c, a.t, ntiles);
}

int launch_filter_scatter(Ctx *c, const FilterScatterArgs &a) {
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(filter_scatter_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
