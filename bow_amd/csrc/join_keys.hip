// join_keys.hip — the join on SEVERAL common columns (reference getCommonCols bowjoin.go:128-155, getCommonRows :161-186): the kernels that
// reduce a tuple of keys to one exact surrogate key per row, so that the one-key join of join.hip runs on it as it stands.  Hand-written
// for gfx950 (wave64); host orchestration in join_keys_api.cpp.
//
// Nothing is hashed.  Per key pair the left and the right key are ranked TOGETHER: equal keys of either side get the same dense rank, a
// null key gets rank 0, and two ranks packed into one 64-bit word are equal exactly when both keys are.  More than two keys rank the
// packed word again and pack it with the next key's rank.
//
//   join_keys_concat_kernel   the left then the right key as one column of L + R slots: raw bits of a valid row, 0 under a null (no
//                             payload under a null reaches the sort); raises one flag bit per side for a NaN among the valid rows
//   (sort.hip's radix argsort over that column, or its "already in order" answer)
//   join_keys_marks_kernel    over SORTED positions: 1 where the key image differs from its predecessor's; one extra slot takes the
//                             scan's total, so that after the exclusive scan slot j + 1 holds the dense rank of position j
//   (sort.hip's scan)
//   join_keys_rank_kernel     over sorted positions: scatters 1 + dense rank to the ORIGINAL row, 0 where the row's key is null (the
//                             null rows sorted into the group of a real 0: the override makes that harmless)
//   join_keys_pack_kernel     rank_a << 32 | rank_b per row
//
// Every kernel is a grid-stride loop over rows; every output word has one owner; the only atomic is the OR into the NaN flag word.
// Every value is an integer count: the same call gives the same bytes.
#include "join_host.h"
#include "key_image.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ bool row_valid(const uint32_t *__restrict__ vbits, int64_t vbit0, int64_t row) {
    if (!vbits) return true;
    const int64_t bit = vbit0 + row;
    return (vbits[bit >> 5] >> (bit & 31)) & 1u;
}

__global__ __launch_bounds__(kThreads) void join_keys_concat_kernel(JoinKeysConcatArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    uint32_t nan = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
        const int side = i >= a.n_left;
        const int64_t row = side ? i - a.n_left : i;
        uint64_t bits = 0;
        if (row_valid(a.vbits[side], a.vbit0[side], row)) {
            bits = a.keys[side][row];
            if (a.is_float && is_nan_bits(bits)) nan |= 1u << side;   // (the call is declined: nothing of this column is used)
        }
        a.out[i] = bits;
    }
    const bool l = __any(nan & 1u), r = __any(nan & 2u);
    if ((l || r) && lane == 0) atomicOr(a.nan, (l ? 1u : 0u) | (r ? 2u : 0u));
}

__device__ __forceinline__ uint64_t image_of(uint64_t v, int mode) { return mode == 2 ? v : key_image(v, mode); }

__global__ __launch_bounds__(kThreads) void join_keys_marks_kernel(const uint64_t *__restrict__ src, int mode, int64_t n, uint32_t *__restrict__ marks) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j <= n; j += stride) {
        uint32_t m = 0;
        if (j > 0 && j < n) m = image_of(src[j], mode) != image_of(src[j - 1], mode);
        marks[j] = m;
    }
}

__global__ __launch_bounds__(kThreads) void join_keys_rank_kernel(JoinKeysRankArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < a.n; j += stride) {
        const int64_t p = a.perm ? (int64_t)a.perm[j] : j;   // (a permutation of [0, n): every slot of rank has one writer)
        const int side = p >= a.n_left;
        const bool valid = row_valid(a.vbits[side], a.vbit0[side], side ? p - a.n_left : p);
        a.rank[p] = valid ? 1u + a.scanned[j + 1] : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void join_keys_pack_kernel(const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, int64_t n,
                                                                  uint64_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) out[i] = (uint64_t)hi[i] << 32 | lo[i];
}

}  // namespace

int launch_join_keys_concat(Ctx *c, const JoinKeysConcatArgs &a) {
    hipLaunchKernelGGL(join_keys_concat_kernel, dim3((unsigned)stream_grid(a.n, kThreads)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_keys_marks(Ctx *c, const uint64_t *src, int mode, int64_t n, uint32_t *marks) {
    hipLaunchKernelGGL(join_keys_marks_kernel, dim3((unsigned)stream_grid(n + 1, kThreads)), dim3(kThreads), 0, c->stream, src, mode, n, marks);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_keys_rank(Ctx *c, const JoinKeysRankArgs &a) {
    hipLaunchKernelGGL(join_keys_rank_kernel, dim3((unsigned)stream_grid(a.n, kThreads)), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_join_keys_pack(Ctx *c, const uint32_t *hi, const uint32_t *lo, int64_t n, uint64_t *out) {
    hipLaunchKernelGGL(join_keys_pack_kernel, dim3((unsigned)stream_grid(n, kThreads)), dim3(kThreads), 0, c->stream, hi, lo, n, out);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
