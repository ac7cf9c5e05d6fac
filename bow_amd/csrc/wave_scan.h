// Wave64 scans shared by the radix sort (sort.hip), the filter's compaction (filter.hip) and the join's row lists (join.hip).
// (The DPP scan and reductions of the Aggregate / Interpolate kernels - other instructions - live in wave_ops.h.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bowgpu {

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// The prologue of a pass over one 64-word tile of a row bitmap, run by ONE wave (the caller's barrier follows): the tile's words into
// sword[64], the set bits of the tile's earlier words into sbase[64].  Returns the inclusive count at the lane (lane 63: the tile's).
// A set bit `lane` of word wi then has the slot sbase[wi] + popcount(word & ((1 << lane) - 1)) among the tile's set bits.
__device__ __forceinline__ uint32_t tile_word_bases(const unsigned long long *tile_words, int lane, unsigned long long *sword, uint32_t *sbase) {
    const unsigned long long word = tile_words[lane];
    const uint32_t pc = (uint32_t)__popcll(word);
    const uint32_t incl = wave_inclusive_scan(pc, lane);
    sword[lane] = word;
    sbase[lane] = incl - pc;
    return incl;
}

}  // namespace bowgpu
