// sort_shard.hip — Bow.SortByCol over a frame held as row-range shards on several devices: the kernels of the steps that are not a
// local sort, a gather or an append.  Hand-written for gfx950 (wave64); host orchestration in sort_shard_api.cpp.
//
//   split_bounds_kernel     one workgroup, two lanes per candidate image: lower and upper bound of the candidate in the rank's sorted
//                           key by binary search.  The host bisects the 64-bit image range with it, one launch per rank and round.
//   image_at_kernel         the images at a handful of rows (a rank's first and last key, the two ends of its pieces).
//   merge_init_kernel       (image, row) pairs of a staging frame's key column: the runs before their first merge round.
//   merge_partition_kernel  merge path: per output tile of kMergeTileRows rows of a pair of adjacent runs, how many of the outputs in
//                           front of the tile come from the LEFT run - a binary search along the tile's diagonal.  On equal images the
//                           left run's rows come first.
//   merge_runs_kernel       one workgroup per tile: the tile's two slices of images into LDS (16 KB), every element ranked in the
//                           other slice by binary search there (a left element counts the right elements BELOW it, a right element
//                           the left elements NOT ABOVE it: left wins ties, the merge is stable), image and row stored at tile base +
//                           own position + rank.  Every output position has exactly one owner: no atomics, no workgroup waits for
//                           another, the result is a function of the inputs alone.
#include "common.h"
#include "key_image.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kMergeTileRows;
constexpr int kItems = kTile / kThreads;   // elements a thread of merge_runs_kernel carries in registers
static_assert(kItems * kThreads == kTile, "a tile is split evenly");

__device__ __forceinline__ uint64_t image_of(uint64_t bits, int mode) { return mode == kKeyImages ? bits : key_image(bits, mode); }

__global__ __launch_bounds__(2 * kShardMaxWorld) void split_bounds_kernel(SplitBoundsArgs a) {
    const int j = threadIdx.x >> 1, upper = threadIdx.x & 1;
    if (j >= a.ncand) return;
    const uint64_t x = a.cand[j];
    int64_t lo = 0, hi = a.n;   // rows [0, lo) are below (upper: not above) x, rows [hi, n) are not
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t v = image_of(a.keys[mid], a.mode);
        if (upper ? v <= x : v < x) lo = mid + 1;
        else hi = mid;
    }
    a.out[threadIdx.x] = (uint32_t)lo;
}

__global__ __launch_bounds__(kThreads) void image_at_kernel(ImageAtArgs a) {
    if ((int)threadIdx.x < a.npos) a.out[threadIdx.x] = image_of(a.keys[a.pos[threadIdx.x]], a.mode);
}

__global__ __launch_bounds__(kThreads) void merge_init_kernel(const uint64_t *keys, int64_t n, int is_float, uint64_t *img, uint32_t *idx) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        img[i] = key_image(keys[i], is_float);
        idx[i] = (uint32_t)i;
    }
}

// the pair of runs tile g belongs to
__device__ __forceinline__ int pair_of(const MergeRoundArgs &a, uint32_t g) {
    int j = 0;
    while (j + 1 < a.npairs && a.tile0[j + 1] <= g) j++;
    return j;
}

__global__ __launch_bounds__(kThreads) void merge_partition_kernel(MergeRoundArgs a) {
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= (uint32_t)a.ntiles) return;
    const int j = pair_of(a, g);
    const uint32_t a0 = a.start[2 * j], b0 = a.start[2 * j + 1], e = a.start[2 * j + 2];
    const uint32_t la = b0 - a0, lb = e - b0;
    const uint32_t diag = (g - a.tile0[j]) * (uint32_t)kTile;   // outputs of the pair in front of the tile (< la + lb)
    const uint64_t *__restrict__ A = a.img_in + a0, *__restrict__ B = a.img_in + b0;
    uint32_t lo = diag > lb ? diag - lb : 0, hi = diag < la ? diag : la;
    while (lo < hi) {   // the left run gives lo .. hi of the first diag outputs
        const uint32_t mid = lo + ((hi - lo) >> 1);
        // A[mid] <= B[diag - mid - 1]: with mid from the left, that right element is taken and A[mid], which comes before it, is not
        if (A[mid] <= B[diag - mid - 1]) lo = mid + 1;
        else hi = mid;
    }
    a.part[g] = lo;
}

__global__ __launch_bounds__(kThreads) void merge_runs_kernel(MergeRoundArgs a) {
    __shared__ uint64_t s_img[kTile];
    const uint32_t g = blockIdx.x;
    const int j = pair_of(a, g);
    const uint32_t a0 = a.start[2 * j], b0 = a.start[2 * j + 1], e = a.start[2 * j + 2];
    const uint32_t la = b0 - a0, lb = e - b0;
    const uint32_t diag = (g - a.tile0[j]) * (uint32_t)kTile;
    const uint32_t rows = la + lb - diag < (uint32_t)kTile ? la + lb - diag : (uint32_t)kTile;
    const uint32_t ab = a.part[g], ae = g + 1 < a.tile0[j + 1] ? a.part[g + 1] : la;   // the tile's slice of the left run
    const uint32_t na = ae - ab, bb = diag - ab;                                      // ... and of the right run: [bb, bb + rows - na)
    uint64_t img[kItems];
    uint32_t idx[kItems];
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t p = (uint32_t)k * kThreads + threadIdx.x;
        if (p < rows) {
            const uint32_t src = p < na ? a0 + ab + p : b0 + bb + (p - na);
            img[k] = a.img_in[src];
            idx[k] = a.idx_in[src];
            s_img[p] = img[k];
        }
    }
    __syncthreads();
    const uint32_t out0 = a0 + diag;
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t p = (uint32_t)k * kThreads + threadIdx.x;
        if (p >= rows) continue;
        const bool left = p < na;
        // left element: right elements below it; right element: left elements not above it
        uint32_t lo = left ? na : 0, hi = left ? rows : na;
        const uint32_t base = lo;
        const uint64_t x = img[k];
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const uint64_t v = s_img[mid];
            if (left ? v < x : v <= x) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t out = out0 + (left ? p : p - na) + (lo - base);
        a.img_out[out] = x;
        a.idx_out[out] = idx[k];
    }
}

}  // namespace

int launch_split_bounds(Ctx *c, const SplitBoundsArgs &a) {
    hipLaunchKernelGGL(split_bounds_kernel, dim3(1), dim3(2 * kShardMaxWorld), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_image_at(Ctx *c, const ImageAtArgs &a) {
    hipLaunchKernelGGL(image_at_kernel, dim3(1), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_merge_init(Ctx *c, const uint64_t *keys, int64_t n, int is_float, uint64_t *img, uint32_t *idx) {
    hipLaunchKernelGGL(merge_init_kernel, dim3((unsigned)stream_grid(n, kThreads)), dim3(kThreads), 0, c->stream, keys, n, is_float, img, idx);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_merge_round(Ctx *c, MergeRoundArgs *a, int nruns) {
    a->npairs = nruns / 2;
    uint32_t t = 0;
    for (int j = 0; j < a->npairs; j++) {
        a->tile0[j] = t;
        t += (uint32_t)(((int64_t)(a->start[2 * j + 2] - a->start[2 * j]) + kTile - 1) / kTile);
    }
    a->tile0[a->npairs] = t;
    a->ntiles = (int32_t)t;
    if (t > 0) {
        hipLaunchKernelGGL(merge_partition_kernel, dim3((t + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, *a);
        hipLaunchKernelGGL(merge_runs_kernel, dim3(t), dim3(kThreads), 0, c->stream, *a);
        BG_HIP(hipGetLastError());
    }
    if (nruns & 1) {   // the unpaired last run is carried over as it is
        const uint32_t r0 = a->start[nruns - 1], rows = a->start[nruns] - r0;
        BG_HIP(hipMemcpyAsync(a->img_out + r0, a->img_in + r0, (size_t)rows * 8, hipMemcpyDeviceToDevice, c->stream));
        BG_HIP(hipMemcpyAsync(a->idx_out + r0, a->idx_in + r0, (size_t)rows * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}

}  // namespace bowgpu
