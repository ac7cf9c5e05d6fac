// join_host.h — what the host files of the join hand each other: join_api.cpp (one key per side) owns the checks, the count and the
// expand; join_keys_api.cpp (several keys per side) reduces its key tuples to one surrogate key per side and calls them as they stand.
#pragma once

#include "common.h"

namespace bowgpu {

constexpr int64_t kJoinMaxRows = (int64_t)1 << 31;   // rows inside the kernels are 32 bits wide

// everything a call keeps on the device between its count and its gather
struct JoinWork {
    DevCol rk;                 // the right key
    StagedCols left;           // the left key, by left frame column (moved with its group)
    const DevCol *lk = nullptr;
    MaskWork vw, uw;           // the right key's validity; the right-only rows
    SortWork sw;
    DevBuf vrows, ckeys, index, simg, first, count, starts, sums, head, stats, ubits, urows, out_l, out_r;
    int64_t n_left = 0, n_right = 0, rn = 0, rv = 0, rows_left = 0, tail = 0;
    bool probed = false;       // false: no pair list (an empty side, no common column) - identity rows
};

// the checks of the entry points, in the words every join entry point reports them with
int join_side_limit(int64_t n, const char *side);
int join_key_checks(const bowgpu_col *k, const char *side);
int join_kind_check(int32_t kind);
int join_types_check(const bowgpu_col *l, const bowgpu_col *r);   // bowjoin.go:135-139, up to the column name
int join_rows_limit(int64_t rows);

// the count: the right side, the probe, the right-only rows.  *rows / *pairs; nothing of the caller's is written.  Synchronises.
// lkey_col: the left frame column the key is (the gather then finds it staged in w->left); -1: the key is no frame column
int join_count_device(Ctx *c, const bowgpu_col *lkey, int32_t lkey_col, const bowgpu_col *rkey, int32_t kind, JoinWork *w, int64_t *rows, int64_t *pairs);
// the index pairs of the `rows` output rows, as 32-bit rows in the workspace (no synchronise)
int join_expand_device(Ctx *c, int32_t kind, JoinWork *w, int64_t rows);

// join_keys.hip: the surrogate key of a tuple of keys (host side: join_keys_api.cpp)
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
