// join_host.h — the surrogate key of a tuple of keys: what join_api.cpp (the join's entry points and its one host path), join_surrogate.cpp
// (the host side of the reduction) and join_keys.hip (its kernels) hand each other.
#pragma once

#include "common.h"

namespace bowgpu {

// one key pair's two columns on the device
struct KeyPair {
    const DevCol *l, *r;
};
// The surrogate keys of n_keys >= 2 key pairs of n_left / n_right rows: packed[0, n_left) the left rows', packed[n_left, n_left + n_right)
// the right rows', Int64.  Equal exactly when the tuples are (a null equals a null per column), no nulls, no NaN.  Synchronises
int surrogate_keys(Ctx *c, const KeyPair *keys, int32_t n_keys, int64_t n_left, int64_t n_right, DevBuf *packed);

// join_keys.hip
struct JoinKeysConcatArgs {
    const uint64_t *keys[2];     // left, right
    const uint32_t *vbits[2];    // nullptr: no nulls
    int64_t vbit0[2];
    int64_t n_left, n;           // n = n_left + n_right
    uint64_t *out;               // [n] raw bits of the valid rows, 0 under a null
    uint32_t *nan;               // one word, zeroed by the host: bit 0 / 1 - a NaN among the valid rows of the left / right key
    int32_t is_float, _pad;
};
int launch_join_keys_concat(Ctx *c, const JoinKeysConcatArgs &a);
// marks[j] = 1 where sorted position j >= 1 differs from j - 1, else 0, j in [0, n]; marks[n] = 0 (the scan's total lands there).
// mode 0 / 1: src holds raw Int64 / Float64 keys (a column found in order), 2: images
int launch_join_keys_marks(Ctx *c, const uint64_t *src, int mode, int64_t n, uint32_t *marks);
struct JoinKeysRankArgs {
    const uint32_t *scanned;     // [n + 1] the marks after the exclusive scan: scanned[j + 1] is the dense rank of sorted position j
    const uint32_t *perm;        // nullptr: the column was in order
    const uint32_t *vbits[2];    // the two inputs' validity; nullptr: no nulls (always so for a packed pair)
    int64_t vbit0[2];
    int64_t n_left, n;
    uint32_t *rank;              // [n] by ORIGINAL row: 0 for a null key, else 1 + dense rank
};
int launch_join_keys_rank(Ctx *c, const JoinKeysRankArgs &a);
// out[i] = hi[i] << 32 | lo[i]
int launch_join_keys_pack(Ctx *c, const uint32_t *hi, const uint32_t *lo, int64_t n, uint64_t *out);

}  // namespace bowgpu
