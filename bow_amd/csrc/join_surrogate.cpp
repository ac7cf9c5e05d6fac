// join_surrogate.cpp — the host side of the join on SEVERAL common columns (reference getCommonRows bowjoin.go:161-186: a row pair is
// common when it agrees on every common column): the kernels of join_keys.hip around the argsort and the scan of Bow.SortByCol reduce the
// key tuples of both sides to one Int64 surrogate column per side, the probe keys join_api.cpp counts on.  No key is compared on the CPU.
#include <string.h>

#include "common.h"
#include "join_host.h"

using namespace bowgpu;

namespace {

// the dense ranks of one column of n rows (already the concatenation of both sides) by ORIGINAL row.  vl / vr: the validity of the two
// inputs it was concatenated from - a null row takes rank 0; nullptr for a column without nulls.  Synchronises (the argsort does)
int rank_column(Ctx *c, const uint64_t *col, int32_t type, int64_t n_left, int64_t n, const DevCol *vl, const DevCol *vr, uint32_t *rank) {
    SortWork sw;
    DevBuf marks, sums;
    int32_t sorted = 0;
    BG_TRY(argsort_device(c, DeviceKey(col, n, type), &sw, &sorted));
    BG_TRY(marks.alloc((size_t)(n + 1) * 4));
    BG_TRY(sums.alloc((size_t)((n + 1 + 4095) / 4096) * 4));
    if (sorted) BG_TRY(launch_join_keys_marks(c, col, type == BOWGPU_FLOAT64, n, marks.as<uint32_t>()));
    else BG_TRY(launch_join_keys_marks(c, sw.keys[sw.cur].as<const uint64_t>(), 2, n, marks.as<uint32_t>()));
    BG_TRY(launch_scan_u32(c, marks.as<uint32_t>(), n + 1, sums.as<uint32_t>()));
    JoinKeysRankArgs a;
    memset(&a, 0, sizeof a);
    a.scanned = marks.as<const uint32_t>();
    a.perm = sorted ? nullptr : sw.perm();
    if (vl) { a.vbits[0] = vl->vbits; a.vbit0[0] = vl->vbit0; }
    if (vr) { a.vbits[1] = vr->vbits; a.vbit0[1] = vr->vbit0; }
    a.n_left = n_left;
    a.n = n;
    a.rank = rank;
    BG_TRY(launch_join_keys_rank(c, a));
    BG_HIP(hipStreamSynchronize(c->stream));   // the sort's and the scan's buffers go back with this scope
    return 0;
}

}  // namespace

namespace bowgpu {

// the buffers of one key pair go back before the next one's are taken
int surrogate_keys(Ctx *c, const KeyPair *keys, int32_t n_keys, int64_t n_left, int64_t n_right, DevBuf *packed) {
    const int64_t n = n_left + n_right;
    DevBuf rank_a, rank_b, flag;
    BG_TRY(rank_a.alloc((size_t)n * 4));
    BG_TRY(rank_b.alloc((size_t)n * 4));
    BG_TRY(packed->alloc(temp_values_bytes(n)));
    BG_TRY(flag.alloc(4));
    for (int32_t k = 0; k < n_keys; k++) {
        {
            const int32_t type = keys[k].l->type;
            DevBuf cat;
            BG_TRY(cat.alloc(temp_values_bytes(n)));
            BG_HIP(hipMemsetAsync(flag.p, 0, 4, c->stream));
            JoinKeysConcatArgs a;
            memset(&a, 0, sizeof a);
            a.keys[0] = reinterpret_cast<const uint64_t *>(keys[k].l->values);
            a.keys[1] = reinterpret_cast<const uint64_t *>(keys[k].r->values);
            a.vbits[0] = keys[k].l->vbits;
            a.vbits[1] = keys[k].r->vbits;
            a.vbit0[0] = keys[k].l->vbit0;
            a.vbit0[1] = keys[k].r->vbit0;
            a.n_left = n_left;
            a.n = n;
            a.out = cat.as<uint64_t>();
            a.nan = flag.as<uint32_t>();
            a.is_float = type == BOWGPU_FLOAT64;
            BG_TRY(launch_join_keys_concat(c, a));
            uint32_t nan = 0;
            BG_HIP(hipMemcpyAsync(&nan, flag.p, 4, hipMemcpyDeviceToHost, c->stream));
            BG_HIP(hipStreamSynchronize(c->stream));
            if (nan)
                return fail(BOWGPU_ERR_UNSUPPORTED, "%s join column of key pair %d holds a NaN among its valid rows: it equals nothing in the reference "
                                                    "(the caller keeps the reference path)", (nan & 1u) ? "left" : "right", k);
            BG_TRY(rank_column(c, cat.as<const uint64_t>(), type, n_left, n, keys[k].l, keys[k].r, (k == 0 ? rank_a : rank_b).as<uint32_t>()));
        }
        if (k == 0) continue;
        BG_TRY(launch_join_keys_pack(c, rank_a.as<const uint32_t>(), rank_b.as<const uint32_t>(), n, packed->as<uint64_t>()));
        if (k < n_keys - 1)   // more keys to come: the pair as ONE key, ranked again (it has no nulls)
            BG_TRY(rank_column(c, packed->as<const uint64_t>(), BOWGPU_INT64, n_left, n, nullptr, nullptr, rank_a.as<uint32_t>()));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace bowgpu
