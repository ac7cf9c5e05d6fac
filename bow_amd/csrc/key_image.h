// The order of Buffer.Less (bowbuffer.go:126-139) as an unsigned 64-bit image, shared by the radix sort (sort.hip) and the join's
// probe (join.hip): equal images <=> Go's == on the boxed value, for keys without a NaN.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bowgpu {

// x ^ 2^63 for Int64; for Float64 the sign-flip map with -0.0 folded onto +0.0 (equal under Less: they keep their input order).
__device__ __forceinline__ uint64_t key_image(uint64_t bits, int is_float) {
    if (is_float) {
        if ((bits << 1) == 0) bits = 0;
        return (bits >> 63) ? ~bits : bits ^ 0x8000000000000000ull;
    }
    return bits ^ 0x8000000000000000ull;
}
__device__ __forceinline__ bool is_nan_bits(uint64_t bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

}  // namespace bowgpu
