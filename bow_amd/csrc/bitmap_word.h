// bitmap_word.h — 64 rows of an Arrow validity bitmap as one word per lane (valid_mask_kernel of frame_ops.hip, find_null_kernel of
// append.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bowgpu {

// rows [row0, row0 + 64) of a bitmap as one word: three 32-bit words funnel-shifted onto row alignment (words at or past vwords - they
// hold no row of the column - read as 0)
__device__ __forceinline__ unsigned long long bitmap_word64(const uint32_t *vb, int64_t vbit0, int64_t vwords, int64_t row0) {
    const int64_t bit = vbit0 + row0;
    const int64_t i = bit >> 5;
    const uint32_t sh = (uint32_t)(bit & 31);
    const uint32_t w0 = i < vwords ? vb[i] : 0u, w1 = i + 1 < vwords ? vb[i + 1] : 0u, w2 = (sh && i + 2 < vwords) ? vb[i + 2] : 0u;
    const uint32_t lo = __funnelshift_r(w0, w1, sh), hi = __funnelshift_r(w1, w2, sh);
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

}  // namespace bowgpu
