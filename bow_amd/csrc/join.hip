// join.hip — Bow.InnerJoin / OuterJoin on the device (reference bowjoin.go:12-125, getCommonRows :161-186, the fills :188-574): the
// left-ordered lookup join on one key.  Hand-written for gfx950 (wave64); host orchestration in join_api.cpp.
//
// The output keeps the LEFT frame's row order, so only the right key is sorted (sort.hip's radix argsort); the kernels here are what
// lies around it:
//
//   join_split_rows_kernel    a row bitmap (the mask pass and the scanned tile counts of Bow.Filter) as 32-bit ROW NUMBERS in row order:
//                             set bits to one list, clear bits to another.  Bow.Filter's scatter moves 64-bit column payloads; row
//                             numbers have no source column, and their slot is the same arithmetic (tile base + set bits of the
//                             earlier words + set bits below the lane).  Serves the right key's null / valid rows and the right-only rows.
//   join_right_index_kernel   the one index array [right rows with a null key, row order | right rows with a value, key order, ties in
//                             row order] from the sort's permutation, and the sorted key images where the sort did not run
//   join_probe_kernel         one lane per left row: lower and upper bound of the key's image in the sorted images (neighbouring lanes
//                             of a sorted left key walk the same cache lines); a null key takes the range of the first part; stores
//                             (first, count) and the rows the left row becomes, flags the head of the matched group with a plain
//                             store of 1 (every writer stores the same byte), sums pairs and matched left rows with integer atomics
//   join_unmatched_kernel     a right row is right-only when the head of its group of equals is not flagged; one bit per right ROW
//                             (integer atomic OR into a zeroed bitmap), so the rows come out in row order through the mask pass
//   join_expand_kernel        work divided over OUTPUT rows in tiles of 4096, as append_kernel's: a row finds its left row as the last
//                             scanned start <= the row; the wave looks its first and last row up with scalar loads and searches
//                             nothing when both fall into one left row or into a run of count-1 rows; the pair is two 32-bit words
//
// The rows themselves are moved by sort.hip's gather_kernel, in its <int32_t, true> form: an index of -1 is "no row" and gives a null
// slot, and the key column reads the other frame's key where its own index says so.
//
// Every count is an integer added in an order-free way or scanned in a fixed order; every output byte has one writer or receives the
// same value from all of them: the same call gives the same bytes.
#include "common.h"
#include "key_image.h"
#include "wave_scan.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = kFilterTileRows;
constexpr int kTileWords = kTile / 64;
constexpr int kWaveWords = kTileWords / kWaves;
constexpr int kWaveRows = kTile / kWaves;
static_assert(kTileWords == 64, "tile_word_bases scans a tile's word counts with one wave");

// first position in s[0, n) whose image is >= x (lo given: the search starts there)
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *__restrict__ s, uint32_t lo, uint32_t n, uint64_t x) {
    uint32_t hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound(const uint64_t *__restrict__ s, uint32_t lo, uint32_t n, uint64_t x) {
    uint32_t hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one workgroup per tile of the mask
__global__ __launch_bounds__(kThreads) void join_split_rows_kernel(const unsigned long long *mask, const uint32_t *tile_base, int64_t n,
                                                                   const uint64_t *values, uint32_t *set_rows, uint64_t *set_values,
                                                                   uint32_t *clear_rows) {
    __shared__ unsigned long long sword[kTileWords];
    __shared__ uint32_t sbase[kTileWords];   // set bits in the tile's earlier words
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kTile;
    if (w == 0) tile_word_bases(mask + (int64_t)blockIdx.x * kTileWords, lane, sword, sbase);   // (filter_scatter_kernel's prologue)
    __syncthreads();
    const int64_t base = (int64_t)tile_base[blockIdx.x];   // set bits of the earlier tiles; tile0 - base: their clear bits
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 4
    for (int k = 0; k < kWaveWords; k++) {
        const int wi = w * kWaveWords + k;
        const int64_t row = tile0 + (int64_t)wi * 64 + lane;
        if (row >= n) continue;   // (rows >= n: clear bits that are no rows)
        const unsigned long long word = sword[wi];
        if ((word >> lane) & 1ull) {
            const int64_t pos = base + sbase[wi] + (uint32_t)__popcll(word & below);
            if (set_rows) set_rows[pos] = (uint32_t)row;
            if (set_values) set_values[pos] = values[row];
        } else if (clear_rows) {
            const int64_t pos = (tile0 - base) + ((uint32_t)wi * 64u - sbase[wi]) + (uint32_t)__popcll(~word & below);
            clear_rows[pos] = (uint32_t)row;
        }
    }
}

__global__ __launch_bounds__(kThreads) void join_right_index_kernel(JoinRightArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < a.rv; j += stride) {
        const uint32_t p = a.perm ? a.perm[j] : (uint32_t)j;
        a.index[a.rn + j] = a.vrows ? a.vrows[p] : p;
        if (a.img_out) a.img_out[j] = key_image(a.keys[j], a.is_float);
    }
}

__global__ __launch_bounds__(kThreads) void join_probe_kernel(JoinProbeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    unsigned long long pairs = 0, matched = 0;
    bool nan = false, null_seen = false;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
        bool valid = true;
        if (a.vbits) {
            const int64_t bit = a.vbit0 + i;
            valid = (a.vbits[bit >> 5] >> (bit & 31)) & 1u;
        }
        uint32_t first = 0, count = 0;
        if (!valid) {   // nil == nil: the right rows with a null key
            null_seen = true;
            count = (uint32_t)a.rn;
        } else {
            const uint64_t bits = a.keys[i];
            if (a.is_float && is_nan_bits(bits)) {
                nan = true;   // (the call is declined: nothing of this row is used)
            } else if (a.rv > 0) {
                const uint64_t img = key_image(bits, a.is_float);
                const uint32_t lb = lower_bound(a.simg, 0, (uint32_t)a.rv, img);
                const uint32_t ub = upper_bound(a.simg, lb, (uint32_t)a.rv, img);
                count = ub - lb;
                first = (uint32_t)a.rn + lb;
                if (count) a.head[lb] = 1;   // every writer of this byte stores 1
            }
        }
        a.first[i] = first;
        a.count[i] = count;
        a.out_count[i] = a.outer && count == 0 ? 1u : count;
        pairs += count;
        matched += count != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pairs += __shfl_down(pairs, o);
        matched += __shfl_down(matched, o);
    }
    if (lane == 0) {
        if (pairs) atomicAdd(&a.stats->pairs, pairs);
        if (matched) atomicAdd(&a.stats->matched_left, matched);
    }
    if (__any(nan) && lane == 0) atomicOr(&a.stats->nan, 1u);
    if (__any(null_seen) && lane == 0) atomicOr(&a.stats->left_null, 1u);
}

__global__ __launch_bounds__(kThreads) void join_unmatched_kernel(const uint32_t *index, const uint64_t *simg, const uint8_t *head,
                                                                  const JoinStats *stats, int64_t rn, int64_t rv, uint32_t *bits) {
    const int64_t stride = (int64_t)gridDim.x * kThreads, r = rn + rv;
    const bool left_null = stats->left_null != 0;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < r; p += stride) {
        bool matched;
        if (p < rn) {
            matched = left_null;   // the first part is matched exactly when some left key is null
        } else {
            const uint32_t j = (uint32_t)(p - rn);
            matched = head[lower_bound(simg, 0, j, simg[j])] != 0;   // (the head of j's group lies at or below j)
        }
        if (!matched) {
            const uint32_t row = index[p];
            atomicOr(&bits[row >> 5], 1u << (row & 31));
        }
    }
}

// the last i in [lo, hi] with starts[i] <= row (starts[lo] <= row is known)
__device__ __forceinline__ uint32_t left_row_of(const uint32_t *__restrict__ starts, uint32_t lo, uint32_t hi, uint32_t row) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (starts[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void join_expand_kernel(JoinExpandArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)w * kWaveRows;
    if (first >= a.rows) return;   // (the whole wave)
    const uint32_t r0 = (uint32_t)first;
    const uint32_t rlast = first + kWaveRows <= a.rows ? r0 + kWaveRows - 1 : (uint32_t)(a.rows - 1);
    const uint32_t nleft = (uint32_t)a.rows_left;
    // wave-uniform: scalar loads of the scanned starts
    uint32_t ilo = 0, ihi = 0;
    bool one = false, run = false;
    if (a.starts && r0 < nleft) {
        const uint32_t llast = rlast < nleft ? rlast : nleft - 1;
        ilo = left_row_of(a.starts, 0, (uint32_t)a.n_left - 1, r0);
        ihi = left_row_of(a.starts, ilo, (uint32_t)a.n_left - 1, llast);
        one = ilo == ihi;
        // outer: every left row becomes at least one row, so starts ascend strictly; a span as long as its rows is a run of count-1 rows
        run = a.outer && a.starts[ilo] == r0 && ihi - ilo == llast - r0;
    }
    for (uint32_t o = r0 + (uint32_t)lane; o <= rlast; o += 64) {
        int32_t l, r;
        if (o >= nleft) {
            l = -1;
            r = a.tail_rows ? (int32_t)a.tail_rows[o - nleft] : (int32_t)(o - nleft);
        } else if (!a.starts) {
            l = (int32_t)o;
            r = -1;
        } else {
            const uint32_t i = one ? ilo : run ? ilo + (o - r0) : left_row_of(a.starts, ilo, ihi, o);
            const uint32_t j = o - a.starts[i];
            l = (int32_t)i;
            r = j < a.count[i] ? (int32_t)a.index[a.first[i] + j] : -1;
        }
        a.out_l[o] = l;
        a.out_r[o] = r;
    }
}

}  // namespace

int launch_join_split_rows(Ctx *c, const unsigned long long *mask, const uint32_t *tile_base, int64_t n, const uint64_t *values, uint32_t *set_rows,
                           uint64_t *set_values, uint32_t *clear_rows) {
    const int64_t ntiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(join_split_rows_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, mask, tile_base, n, values, set_rows, set_values,
                       clear_rows);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_right_index(Ctx *c, const JoinRightArgs &a) {
    hipLaunchKernelGGL(join_right_index_kernel, dim3((unsigned)stream_grid(a.rv, kThreads)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_probe(Ctx *c, const JoinProbeArgs &a) {
    hipLaunchKernelGGL(join_probe_kernel, dim3((unsigned)stream_grid(a.n, kThreads)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_unmatched(Ctx *c, const uint32_t *index, const uint64_t *simg, const uint8_t *head, const JoinStats *stats, int64_t rn, int64_t rv,
                          uint32_t *bits) {
    hipLaunchKernelGGL(join_unmatched_kernel, dim3((unsigned)stream_grid(rn + rv, kThreads)), dim3(kThreads), 0, c->stream, index, simg, head, stats, rn, rv, bits);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_expand(Ctx *c, const JoinExpandArgs &a) {
    const int64_t ntiles = (a.rows + kTile - 1) / kTile;
    hipLaunchKernelGGL(join_expand_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
