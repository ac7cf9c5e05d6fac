// append.hip — AppendBows (reference bowappend.go:11-103) and Bow.Find / FindNext / Contains (bowfind.go:3-32) on the device.
// Hand-written for gfx950 (wave64); host orchestration in append_api.cpp.
//
//   append_kernel       work is divided over OUTPUT rows: a workgroup is one tile of 4096 rows, a wave takes 1024 consecutive rows of it,
//                       64 at a time.  The piece of a row is the last start <= the row in the prefix array of the call's piece table
//                       (which is also what steps over empty pieces); the wave looks its first and its last row up once, with scalar
//                       loads, and when both lie in one piece - the common case - every load of the wave is a plain coalesced 8-byte load
//                       from one base.  Otherwise a lane searches between the two.  The search is done once per row, for up to kMoveCols
//                       columns.  The wave ballots the validity of its 64 rows and stores the word whole: one owner per word however many
//                       pieces meet in it, no atomics, no preset or finish launch.  Null rows store 0.
//   find_kernel         a wave ballots the matches of 64 rows, takes the lowest set lane and lowers one device word with an integer
//                       atomic min.  Before it loads, a wave reads that word and leaves when its first row lies above it: a stale read
//                       costs work, never the answer - the answer is a minimum over all matches.
//   find_null_kernel    the same over validity bitmaps alone: a lane forms the word of 64 rows, a wave is one tile.
//   find_result_kernel  the word into the context's registered host block.
#include "common.h"
#include "bitmap_word.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kFilterTileRows;
constexpr int kWaveRows = kTile / kWaves;   // consecutive rows of a tile that one wave takes
constexpr int kBatch = 4;                   // 64-row words whose loads are issued together
constexpr int kBatches = kWaveRows / (64 * kBatch);
static_assert(kBatches * kBatch * 64 * kWaves == kTile, "a tile is split evenly");

// the last p in [lo, hi] with starts[p] <= row (starts[lo] <= row is known)
__device__ __forceinline__ uint32_t piece_of(const uint32_t *__restrict__ starts, uint32_t lo, uint32_t hi, uint32_t row) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// kUniform: every row of the wave lies in piece plo
template <bool kUniform>
__device__ __forceinline__ void append_wave(const AppendArgs &a, uint32_t r0, uint32_t rlast, uint32_t plo, uint32_t phi, int lane) {
#pragma unroll 1
    for (int b = 0; b < kBatches; b++) {
        const uint32_t base = r0 + (uint32_t)b * (kBatch * 64);
        if (base >= (uint32_t)a.n) return;   // (the whole wave)
        uint32_t row[kBatch], p[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const uint32_t r = base + k * 64 + lane;
            row[k] = r < rlast ? r : rlast;   // rows past the end read the last row: no load is conditional
            p[k] = kUniform ? plo : piece_of(a.starts, plo, phi, row[k]);
        }
#pragma unroll
        for (int c = 0; c < kMoveCols; c++) {
            if (c >= a.cols.ncols) continue;
            const AppendPiece *__restrict__ pieces = a.pieces[c];
            const bool bitmaps = (a.bitmap_mask >> c) & 1u;
            uint64_t x[kBatch];
            uint32_t vw[kBatch];
            int64_t bit[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const AppendPiece pc = pieces[p[k]];
                x[k] = pc.values[row[k]];
                vw[k] = ~0u;
                bit[k] = pc.vadj + row[k];
                if (bitmaps && pc.vbits) vw[k] = pc.vbits[bit[k] >> 5];
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const uint32_t r = base + k * 64 + lane;
                const bool in = r < (uint32_t)a.n;
                const bool ok = in && ((vw[k] >> (bit[k] & 31)) & 1u);
                const unsigned long long word = __ballot(ok);
                if (in) __builtin_nontemporal_store(ok ? x[k] : 0ull, &a.cols.out_values[c][r]);   // a null slot holds 0
                if (lane == 0 && in) a.cols.out_valid[c][r >> 6] = word;                           // (rows >= n: clear bits)
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void append_kernel(AppendArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)w * kWaveRows;
    if (first >= a.n) return;   // (the whole wave)
    const uint32_t r0 = (uint32_t)first;
    const uint32_t rlast = first + kWaveRows <= a.n ? r0 + kWaveRows - 1 : (uint32_t)(a.n - 1);
    // wave-uniform: scalar loads of the prefix array
    const uint32_t plo = piece_of(a.starts, 0, (uint32_t)a.npieces - 1, r0);
    const uint32_t phi = piece_of(a.starts, plo, (uint32_t)a.npieces - 1, rlast);
    if (plo == phi) append_wave<true>(a, r0, rlast, plo, phi, lane);
    else append_wave<false>(a, r0, rlast, plo, phi, lane);
}

// Go's == on the boxed value: integer for Int64, IEEE for Float64 (a NaN equals nothing, -0.0 equals +0.0)
__device__ __forceinline__ bool same_value(uint64_t x, uint64_t v, bool is_float) {
    return is_float ? __longlong_as_double((long long)x) == __longlong_as_double((long long)v) : x == v;
}

// workgroup = one tile from the tile of row_start on, in ascending order; wave = kWaveRows consecutive rows of it
__global__ __launch_bounds__(kThreads) void find_kernel(FindArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t first = (a.row_start / kTile + (int64_t)blockIdx.x) * kTile + (int64_t)w * kWaveRows;
    if (first >= a.n) return;   // (the whole wave)
    const bool is_float = a.is_float != 0;
    const uint32_t last = (uint32_t)(a.n - 1);
#pragma unroll 1
    for (int b = 0; b < kBatches; b++) {
        const uint32_t base = (uint32_t)first + (uint32_t)b * (kBatch * 64);
        if (base > last) return;
        // an ordinary load of the word the matches lower: rows above it cannot be the answer
        if (base > __atomic_load_n(a.result, __ATOMIC_RELAXED)) return;
        uint64_t x[kBatch];
        uint32_t vw[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const uint32_t r = base + k * 64 + lane;
            const uint32_t rc = r < last ? r : last;
            x[k] = a.values[rc];
            vw[k] = ~0u;
            if (a.vbits) vw[k] = a.vbits[(a.vbit0 + rc) >> 5];
        }
#pragma unroll
        for (int k = 0; k < kBatch; k++) {
            const uint32_t r = base + k * 64 + lane;
            const bool hit = r <= last && (int64_t)r >= a.row_start && ((vw[k] >> ((a.vbit0 + r) & 31)) & 1u) && same_value(x[k], a.value, is_float);
            const unsigned long long m = __ballot(hit);
            if (m) {   // (wave-uniform) the lowest set lane is the wave's answer: every later row of the wave lies above it
                if (lane == 0) atomicMin(a.result, base + k * 64 + (uint32_t)__ffsll((long long)m) - 1u);
                return;
            }
        }
    }
}

// the first null of the column: one wave = one tile, lane = word of the tile
__global__ __launch_bounds__(kThreads) void find_null_kernel(FindArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t tile = (int64_t)blockIdx.x * kWaves + w;
    if (tile * kTile >= a.n) return;   // (the whole wave)
    if ((uint32_t)(tile * kTile) > __atomic_load_n(a.result, __ATOMIC_RELAXED)) return;
    const int64_t row0 = tile * kTile + (int64_t)lane * 64;
    unsigned long long nulls = 0;
    if (row0 < a.n) {
        const unsigned long long rows = a.n - row0 < 64 ? (1ull << (a.n - row0)) - 1ull : ~0ull;
        nulls = ~bitmap_word64(a.vbits, a.vbit0, a.vwords, row0) & rows;
    }
    const unsigned long long m = __ballot(nulls != 0);
    if (m && lane == __ffsll((long long)m) - 1) atomicMin(a.result, (uint32_t)row0 + (uint32_t)__ffsll((long long)nulls) - 1u);
}

__global__ void find_result_kernel(const uint32_t *result, uint32_t *host_result) { *host_result = *result; }

}  // namespace

size_t append_table_bytes(int32_t npieces) {
    const size_t starts = (((size_t)npieces + 1) * 4 + 15) & ~(size_t)15;
    return starts + (size_t)kMoveCols * (size_t)npieces * sizeof(AppendPiece);
}

int launch_append(Ctx *c, const AppendArgs &a) {
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(append_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_find(Ctx *c, const FindArgs &a) {
    BG_HIP(hipMemsetAsync(a.result, 0xFF, 4, c->stream));
    if (a.values) {
        const int64_t ntiles = (a.n + kTile - 1) / kTile - a.row_start / kTile;
        hipLaunchKernelGGL(find_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    } else {
        const int64_t ntiles = (a.n + kTile - 1) / kTile;
        hipLaunchKernelGGL(find_null_kernel, dim3((unsigned)((ntiles + kWaves - 1) / kWaves)), dim3(kThreads), 0, c->stream, a);
    }
    BG_HIP(hipGetLastError());
    hipLaunchKernelGGL(find_result_kernel, dim3(1), dim3(1), 0, c->stream, (const uint32_t *)a.result, a.host_result);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
