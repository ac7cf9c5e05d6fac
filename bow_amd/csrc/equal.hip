// equal.hip — the per-row half of Bow.Equal (reference bow.go:227-275) and the search behind GetPrevRowIndex / GetNextRowIndex /
// GetPrevValue(s) / GetNextValue(s) (bowgetters.go:65-151) on the device.  Hand-written for gfx950 (wave64), in the shape of
// find_kernel / find_null_kernel of append.hip; host orchestration in equal_api.cpp.
//
//   equal_kernel        a workgroup is one tile of 4096 rows in ascending order, a wave takes 1024 consecutive rows of it, four 64-row
//                       words at a time, for up to kMoveCols column pairs.  The values of both sides are plain coalesced 8-byte loads.
//                       The validity words of both sides - and a Boolean column's value words - are formed by the first four lanes, one
//                       64-row word each, funnel-shifted onto row alignment (bitmap_word64: each side and each buffer has its own bit
//                       offset), and read by the wave as scalars.  "Differs" is then one wave-uniform word:
//                           (lvalid ^ rvalid) | (lvalid & rvalid & ballot(values differ))        rows >= n masked out
//                       so a null slot's payload is loaded but never compared.  The lowest set bit over the group's columns lowers ONE
//                       device word by an unsigned 64-bit atomic min of (row << 32) | column: that minimum is (first_row, first_col).
//                       Before it loads, a wave reads the word and leaves when its first row lies above it; a stale read costs work,
//                       never the answer.  The word is preset once per CALL, so the waves of a later launch group leave early too.
//   valid_row_kernel    over bitmaps alone: a wave is one tile, a lane forms the ANDed 64-row word of all columns.  Wave 0 takes the tile
//                       of row_start, later waves move away from it in the search direction; bits on the wrong side of row_start and bits
//                       at or past n are masked before the ballot.  Direction +1 lowers the word by an atomic min, direction -1 raises it
//                       (as a signed row, preset to -1) by an atomic max, with the same early leave.  Waves 2 and later first look at
//                       the 64 rows from row_start on and leave when the answer is there (it then belongs to wave 0 or 1).
//   equal_result_kernel / row_result_kernel   the word into the context's registered host block.
// Nothing is stored but those words, with vector stores and atomics only.  The same call gives the same answer: a minimum (maximum) over
// all candidates does not depend on who arrives first.
#include "common.h"
#include "bitmap_word.h"
#include "wave_ops.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kFilterTileRows;
constexpr int kWaveRows = kTile / kWaves;   // consecutive rows of a tile that one wave takes
constexpr int kBatch = 4;                   // 64-row words whose loads are issued together
constexpr int kBatches = kWaveRows / (64 * kBatch);
static_assert(kBatches * kBatch * 64 * kWaves == kTile, "a tile is split evenly");

// rows [row0, row0 + 64) of b as one word; all ones where there is nothing to read
__device__ __forceinline__ unsigned long long word_of(const BitsAt &b, int64_t row0) {
    return b.words ? bitmap_word64(b.words, b.bit0, b.nwords, row0) : ~0ull;
}

// valid rows under the mode: Go's == on the boxed value (IEEE for Float64: a NaN differs from everything, -0.0 equals +0.0), or the 64 bits
__device__ __forceinline__ bool differs(uint64_t x, uint64_t y, bool ieee) {
    return ieee ? !(__longlong_as_double((long long)x) == __longlong_as_double((long long)y)) : x != y;
}

__global__ __launch_bounds__(kThreads) void equal_kernel(EqualArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)w * kWaveRows;
    if (first >= a.n) return;   // (the whole wave)
    const uint32_t last = (uint32_t)(a.n - 1);
#pragma unroll 1
    for (int b = 0; b < kBatches; b++) {
        const uint32_t base = (uint32_t)first + (uint32_t)b * (kBatch * 64);
        if (base > last) return;
        // an ordinary load of the word the differences lower: rows above it cannot be the answer (its own row still can: a lower column)
        if (((unsigned long long)base << 32) > __atomic_load_n(a.result, __ATOMIC_RELAXED)) return;
        unsigned long long best = kEqualNone;   // (wave-uniform)
#pragma unroll
        for (int c = 0; c < kMoveCols; c++) {
            if (c >= a.ncols) continue;
            const EqualCol &col = a.col[c];
            const bool is_bool = col.kind == kEqualBool;
            // lane k < kBatch: the words of rows [base + 64 k, + 64)
            unsigned long long lv = ~0ull, rv = ~0ull, lt = 0, rt = 0;
            if (lane < kBatch) {
                const int64_t row0 = (int64_t)base + lane * 64;
                lv = word_of(col.valid[0], row0);
                rv = word_of(col.valid[1], row0);
                if (is_bool) {
                    lt = word_of(col.truth[0], row0);
                    rt = word_of(col.truth[1], row0);
                }
            }
            uint64_t x[kBatch], y[kBatch];
            if (!is_bool) {
#pragma unroll
                for (int k = 0; k < kBatch; k++) {
                    const uint32_t r = base + k * 64 + lane;
                    const uint32_t rc = r < last ? r : last;   // rows past the end read the last row: no load is conditional
                    x[k] = col.values[0][rc];
                    y[k] = col.values[1][rc];
                }
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const uint32_t r0 = base + k * 64;
                if (r0 > last) continue;
                const unsigned long long rows = last - r0 >= 63 ? ~0ull : (1ull << (last - r0 + 1)) - 1ull;
                const unsigned long long lvk = readlane_u64(lv, k), rvk = readlane_u64(rv, k);
                const unsigned long long neq = is_bool ? readlane_u64(lt, k) ^ readlane_u64(rt, k) : __ballot(differs(x[k], y[k], col.kind == kEqualIeee));
                const unsigned long long d = ((lvk ^ rvk) | (lvk & rvk & neq)) & rows;
                if (d) {
                    const unsigned long long key = ((unsigned long long)(r0 + (uint32_t)__ffsll((long long)d) - 1u) << 32) | (uint32_t)col.col;
                    best = key < best ? key : best;
                }
            }
        }
        if (best != kEqualNone) {   // every later row of the wave lies above it
            if (lane == 0) atomicMin(a.result, best);
            return;
        }
    }
}

// one wave = one tile, lane = word of the tile; wave g takes tile (row_start / kTile) + g * direction
__global__ __launch_bounds__(kThreads) void valid_row_kernel(ValidRowArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t g = (int64_t)blockIdx.x * kWaves + w;
    const bool up = a.direction > 0;
    const int64_t tile = a.row_start / kTile + (up ? g : -g);
    if (tile < 0 || tile * kTile >= a.n) return;   // (the whole wave)
    int32_t *result = reinterpret_cast<int32_t *>(a.result);
    const int32_t seen = __atomic_load_n(result, __ATOMIC_RELAXED);
    if (up ? (uint32_t)(tile * kTile) > (uint32_t)seen : tile * kTile + kTile - 1 < (int64_t)seen) return;   // (the last tile may end past 2^31)
    if (g >= 2) {
        // The 64 rows from row_start on, in the search direction (wave-uniform; they lie in the tiles of waves 0 and 1): when the
        // answer is there - with nulls spread over a column it nearly always is - every other wave leaves, instead of lowering the
        // word with a candidate of its own: thousands of atomics on one address cost more than the search.
        const int64_t near0 = up ? a.row_start : (a.row_start >= 63 ? a.row_start - 63 : 0);
        const int64_t nrows = up ? a.n - near0 : a.row_start - near0 + 1;
        unsigned long long near = nrows < 64 ? (1ull << nrows) - 1ull : ~0ull;
#pragma unroll
        for (int c = 0; c < BOWGPU_VALID_ROW_MAX_COLS; c++)
            if (c < a.ncols) near &= bitmap_word64(a.valid[c].words, a.valid[c].bit0, a.valid[c].nwords, near0);
        if (near) return;
    }
    const int64_t row0 = tile * kTile + (int64_t)lane * 64;
    unsigned long long m = 0;
    if (row0 < a.n) {
        m = a.n - row0 < 64 ? (1ull << (a.n - row0)) - 1ull : ~0ull;
        // the side of row_start the search looks at, inside its own word
        if (up) {
            if (a.row_start >= row0 + 64) m = 0;
            else if (a.row_start > row0) m &= ~0ull << (a.row_start - row0);
        } else {
            if (a.row_start < row0) m = 0;
            else if (a.row_start < row0 + 63) m &= (2ull << (a.row_start - row0)) - 1ull;
        }
#pragma unroll
        for (int c = 0; c < BOWGPU_VALID_ROW_MAX_COLS; c++)
            if (c < a.ncols && m) m &= bitmap_word64(a.valid[c].words, a.valid[c].bit0, a.valid[c].nwords, row0);
    }
    const unsigned long long lanes = __ballot(m != 0);
    if (!lanes) return;
    if (up) {
        if (lane == __ffsll((long long)lanes) - 1) atomicMin(a.result, (uint32_t)row0 + (uint32_t)__ffsll((long long)m) - 1u);
    } else {
        if (lane == 63 - __clzll((long long)lanes)) atomicMax(result, (int32_t)(row0 + 63 - __clzll((long long)m)));
    }
}

__global__ void equal_result_kernel(const unsigned long long *result, unsigned long long *host_result) { *host_result = *result; }
__global__ void row_result_kernel(const uint32_t *result, uint32_t *host_result) { *host_result = *result; }

}  // namespace

int launch_equal_preset(Ctx *c, unsigned long long *result) {
    BG_HIP(hipMemsetAsync(result, 0xFF, 8, c->stream));
    return 0;
}

int launch_equal(Ctx *c, const EqualArgs &a) {
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    hipLaunchKernelGGL(equal_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_equal_result(Ctx *c, const unsigned long long *result, unsigned long long *host_result) {
    hipLaunchKernelGGL(equal_result_kernel, dim3(1), dim3(1), 0, c->stream, result, host_result);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_valid_row(Ctx *c, const ValidRowArgs &a) {
    BG_HIP(hipMemsetAsync(a.result, 0xFF, 4, c->stream));
    const int64_t t0 = a.row_start / kTile;
    const int64_t ntiles = a.direction > 0 ? (a.n + kTile - 1) / kTile - t0 : t0 + 1;
    hipLaunchKernelGGL(valid_row_kernel, dim3((unsigned)((ntiles + kWaves - 1) / kWaves)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    hipLaunchKernelGGL(row_result_kernel, dim3(1), dim3(1), 0, c->stream, (const uint32_t *)a.result, a.host_result);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
