// join_keys_api.cpp — C-ABI entry points of Bow.InnerJoin / OuterJoin on SEVERAL common columns (reference getCommonCols bowjoin.go:128-155,
// getCommonRows :161-186, the per-column fills :383-400): bowgpu_join_keys_rows, bowgpu_join_keys.  No key and one key are
// bowgpu_join_rows / bowgpu_join themselves.  Two keys and more: the kernels of join_keys.hip around the argsort and the scan of
// Bow.SortByCol reduce the key tuples of both sides to one Int64 surrogate column per side, and the one-key join's count, expand and
// gather (join_api.cpp, sort_api.cpp) run on those as they stand; no key is compared and no row is moved on the CPU.
#include <string.h>

#include <vector>

#include "common.h"
#include "join_host.h"

using namespace bowgpu;

namespace {

int n_keys_check(int32_t n_keys) {
    if (n_keys < 0) return fail(BOWGPU_ERR_ARG, "negative key count");
    if (n_keys > BOWGPU_JOIN_MAX_KEYS)
        return fail(BOWGPU_ERR_UNSUPPORTED, "%d join columns: the device join serves at most BOWGPU_JOIN_MAX_KEYS = %d", n_keys, BOWGPU_JOIN_MAX_KEYS);
    return 0;
}

int both_sides_limit(int64_t n_left, int64_t n_right) {   // the surrogate pass sorts both sides as one column, and the argsort is 31-bit
    if (n_left + n_right >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the frames have %lld + %lld rows: the device join on several columns serves fewer than 2^31 = 2147483648 "
                                            "rows on both sides together", (long long)n_left, (long long)n_right);
    return 0;
}

// one key pair's two columns on the device
struct KeyPair {
    const DevCol *l, *r;
    int32_t type;
};

// the dense ranks of one column of n rows (already the concatenation of both sides) by ORIGINAL row.  vl / vr: the validity of the two
// inputs it was concatenated from - a null row takes rank 0; nullptr for a column without nulls.  Synchronises (the argsort does)
int rank_column(Ctx *c, const uint64_t *col, int32_t type, int64_t n_left, int64_t n, const DevCol *vl, const DevCol *vr, uint32_t *rank) {
    SortWork sw;
    DevBuf marks, sums;
    int32_t sorted = 0;
    const bowgpu_col ck = device_col(col, n, type);
    DevCol dk;
    dk.values = col;
    dk.length = n;
    dk.type = type;
    BG_TRY(argsort_device(c, &ck, dk, &sw, &sorted));
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

// The surrogate keys of n_keys >= 2 key pairs: packed[0, L) the left rows', packed[L, L + R) the right rows'.  Equal exactly when the
// tuples are (a null equals a null per column), no nulls, no NaN.  The buffers of one key pair go back before the next one's are taken
int surrogate_keys(Ctx *c, const KeyPair *keys, int32_t n_keys, int64_t n_left, int64_t n_right, DevBuf *packed) {
    const int64_t n = n_left + n_right;
    DevBuf rank_a, rank_b, flag;
    BG_TRY(rank_a.alloc((size_t)n * 4));
    BG_TRY(rank_b.alloc((size_t)n * 4));
    BG_TRY(packed->alloc(temp_values_bytes(n)));
    BG_TRY(flag.alloc(4));
    for (int32_t k = 0; k < n_keys; k++) {
        {
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
            a.is_float = keys[k].type == BOWGPU_FLOAT64;
            BG_TRY(launch_join_keys_concat(c, a));
            uint32_t nan = 0;
            BG_HIP(hipMemcpyAsync(&nan, flag.p, 4, hipMemcpyDeviceToHost, c->stream));
            BG_HIP(hipStreamSynchronize(c->stream));
            if (nan)
                return fail(BOWGPU_ERR_UNSUPPORTED, "%s join column of key pair %d holds a NaN among its valid rows: it equals nothing in the reference "
                                                    "(the caller keeps the reference path)", (nan & 1u) ? "left" : "right", k);
            BG_TRY(rank_column(c, cat.as<const uint64_t>(), keys[k].type, n_left, n, keys[k].l, keys[k].r, (k == 0 ? rank_a : rank_b).as<uint32_t>()));
        }
        if (k == 0) continue;
        BG_TRY(launch_join_keys_pack(c, rank_a.as<const uint32_t>(), rank_b.as<const uint32_t>(), n, packed->as<uint64_t>()));
        if (k < n_keys - 1)   // more keys to come: the pair as ONE key, ranked again (it has no nulls)
            BG_TRY(rank_column(c, packed->as<const uint64_t>(), BOWGPU_INT64, n_left, n, nullptr, nullptr, rank_a.as<uint32_t>()));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// the key columns of both sides staged (where they are host-resident) for the whole call
struct StagedKeys {
    StagedCols left[BOWGPU_JOIN_MAX_KEYS];   // left key k alone, as column 0 of the one-column piece the gather moves it in
    DevCol right[BOWGPU_JOIN_MAX_KEYS];
    KeyPair pairs[BOWGPU_JOIN_MAX_KEYS];
};

int stage_key(Ctx *c, const bowgpu_col *col, DevCol *out) {
    const bowgpu_col k = uncounted(*col);
    return devcol_prepare(c, &k, out, true, true);
}

int stage_keys(Ctx *c, const bowgpu_col *const *lk, const bowgpu_col *const *rk, int32_t n_keys, StagedKeys *s) {
    for (int32_t k = 0; k < n_keys; k++) {
        DevCol *l = s->left[k].add(0);
        BG_TRY(stage_key(c, lk[k], l));
        BG_TRY(stage_key(c, rk[k], &s->right[k]));
        s->pairs[k].l = l;
        s->pairs[k].r = &s->right[k];
        s->pairs[k].type = lk[k]->type;
    }
    return 0;
}

}  // namespace

extern "C" {

int bowgpu_join_keys_rows(const bowgpu_col *left_keys, const bowgpu_col *right_keys, int32_t n_keys, int32_t kind, int64_t *l_idx, int64_t *r_idx,
                          int64_t idx_capacity, int32_t idx_residency, int64_t *rows, int64_t *pairs) {
    if (!rows || !pairs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(n_keys_check(n_keys));
    if (n_keys == 0) return bowgpu_join_rows(nullptr, nullptr, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
    if (!left_keys || !right_keys) return fail(BOWGPU_ERR_ARG, "null argument");
    if (n_keys == 1) return bowgpu_join_rows(left_keys, right_keys, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
    BG_TRY(join_kind_check(kind));
    const int64_t n_left = left_keys[0].length, n_right = right_keys[0].length;
    const bowgpu_col *lk[BOWGPU_JOIN_MAX_KEYS], *rk[BOWGPU_JOIN_MAX_KEYS];
    for (int32_t k = 0; k < n_keys; k++) {
        lk[k] = &left_keys[k];
        rk[k] = &right_keys[k];
        BG_TRY(join_key_checks(lk[k], "left"));
        BG_TRY(join_key_checks(rk[k], "right"));
        if (lk[k]->length != n_left || rk[k]->length != n_right) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        BG_TRY(join_types_check(lk[k], rk[k]));
    }
    BG_TRY(both_sides_limit(n_left, n_right));
    if (n_left == 0 || n_right == 0)   // no pair list whatever the keys are: the one-key call's answer
        return bowgpu_join_rows(lk[0], rk[0], kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
    if (l_idx != nullptr || r_idx != nullptr) {   // (before the device is touched; bowgpu_join_rows says the same)
        if (!l_idx || !r_idx) return fail(BOWGPU_ERR_ARG, "null argument");
        if (!residency_ok(idx_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", idx_residency);
        if (idx_capacity < 0) return fail(BOWGPU_ERR_ARG, "negative index capacity");
    }
    Ctx *c = nullptr;
    BG_TRY(ctx_get(&c));
    DevBuf packed;
    {
        StagedKeys s;   // the staged keys go back before the join proper takes its workspace
        BG_TRY(synced(c, stage_keys(c, lk, rk, n_keys, &s)));
        BG_TRY(synced(c, surrogate_keys(c, s.pairs, n_keys, n_left, n_right, &packed)));
    }
    const bowgpu_col ls = device_col(packed.p, n_left, BOWGPU_INT64), rs = device_col(packed.as<uint64_t>() + n_left, n_right, BOWGPU_INT64);
    return bowgpu_join_rows(&ls, &rs, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
}

int bowgpu_join_keys(const bowgpu_col *left_cols, int32_t n_left_cols, const int32_t *left_keys, const bowgpu_col *right_cols, int32_t n_right_cols,
                     const int32_t *right_keys, int32_t n_keys, int32_t kind, bowgpu_out *outs, int64_t *rows) {
    if (!rows) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(n_keys_check(n_keys));
    if (n_keys == 0) return bowgpu_join(left_cols, n_left_cols, -1, right_cols, n_right_cols, -1, kind, outs, rows);
    if (!left_keys || !right_keys) return fail(BOWGPU_ERR_ARG, "null argument");
    if (n_left_cols < 0 || n_right_cols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if ((n_left_cols > 0 && !left_cols) || (n_right_cols > 0 && !right_cols)) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(join_kind_check(kind));
    const int64_t n_left = n_left_cols > 0 ? left_cols[0].length : 0, n_right = n_right_cols > 0 ? right_cols[0].length : 0;
    BG_TRY(frame_cols_checks(left_cols, n_left_cols, n_left, true));
    BG_TRY(frame_cols_checks(right_cols, n_right_cols, n_right, true));
    const bowgpu_col *lk[BOWGPU_JOIN_MAX_KEYS], *rk[BOWGPU_JOIN_MAX_KEYS];
    for (int32_t k = 0; k < n_keys; k++) {
        if (left_keys[k] < 0 || left_keys[k] > n_left_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the left frame", left_keys[k]);
        if (right_keys[k] < 0 || right_keys[k] > n_right_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the right frame", right_keys[k]);
        for (int32_t j = 0; j < k; j++) {
            if (left_keys[j] == left_keys[k]) return fail(BOWGPU_ERR_ARG, "left column %d is listed twice among the join columns", left_keys[k]);
            if (right_keys[j] == right_keys[k]) return fail(BOWGPU_ERR_ARG, "right column %d is listed twice among the join columns", right_keys[k]);
        }
        lk[k] = &left_cols[left_keys[k]];
        rk[k] = &right_cols[right_keys[k]];
    }
    for (int32_t k = 0; k < n_keys; k++) BG_TRY(join_types_check(lk[k], rk[k]));
    if (n_keys == 1) return bowgpu_join(left_cols, n_left_cols, left_keys[0], right_cols, n_right_cols, right_keys[0], kind, outs, rows);
    BG_TRY(join_side_limit(n_left, "left"));
    BG_TRY(join_side_limit(n_right, "right"));
    BG_TRY(both_sides_limit(n_left, n_right));
    // which key pair a column belongs to (-1: none), and the right columns without the keys, as the frame the outputs behind the left
    // columns come from
    std::vector<int32_t> lkey_of((size_t)n_left_cols, -1), rkey_of((size_t)n_right_cols, -1);
    for (int32_t k = 0; k < n_keys; k++) {
        lkey_of[(size_t)left_keys[k]] = k;
        rkey_of[(size_t)right_keys[k]] = k;
    }
    std::vector<bowgpu_col> rcols;
    for (int i = 0; i < n_right_cols; i++)
        if (rkey_of[(size_t)i] < 0) rcols.push_back(right_cols[i]);
    const int32_t n_rest = (int32_t)rcols.size(), n_outs = n_left_cols + n_rest;
    if (!outs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(outs_checks(outs, n_outs, -1));
    const bool outer = kind == BOWGPU_JOIN_OUTER;
    const bool probe = n_left > 0 && n_right > 0;
    JoinWork w;
    StagedKeys s;
    DevBuf packed;
    Ctx *c = nullptr;
    int64_t total = 0, npairs = 0;
    if (!probe) {   // no pair list: the row count is known without the device
        total = outer ? n_left + n_right : 0;
        BG_TRY(join_rows_limit(total));
    } else {
        BG_TRY(ctx_get(&c));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        BG_TRY(synced(c, stage_keys(c, lk, rk, n_keys, &s)));
        BG_TRY(synced(c, surrogate_keys(c, s.pairs, n_keys, n_left, n_right, &packed)));
        // the surrogates are no frame columns (-1): the gather below never takes one for a column it has to move
        const bowgpu_col ls = device_col(packed.p, n_left, BOWGPU_INT64), rs = device_col(packed.as<uint64_t>() + n_left, n_right, BOWGPU_INT64);
        BG_TRY(synced(c, join_count_device(c, &ls, -1, &rs, kind, &w, &total, &npairs)));
    }
    for (int i = 0; i < n_outs; i++)
        if (outs[i].length < total)
            return fail(BOWGPU_ERR_ARG, "output column %d has %lld slots, %lld needed", i, (long long)outs[i].length, (long long)total);
    BG_TRY(outs_checks(outs, n_outs, total));
    *rows = total;
    if (total == 0) {
        for (int i = 0; i < n_left_cols; i++) out_empty(&outs[i], left_cols[i].type);
        for (int i = 0; i < n_rest; i++) out_empty(&outs[n_left_cols + i], rcols[(size_t)i].type);
        return 0;
    }
    if (!probe) {   // an OuterJoin with an empty side: the other side's rows padded with nulls - the gather's work
        BG_TRY(ctx_get(&c));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        w.n_left = w.rows_left = n_left;
        w.n_right = w.tail = n_right;
        BG_TRY(synced(c, stage_keys(c, lk, rk, n_keys, &s)));
    }
    BG_TRY(synced(c, join_expand_device(c, kind, &w, total)));
    const bool device_out = any_device_out(outs, n_outs);
    // The left frame in pieces: EVERY key column takes the left row's value and, on a right-only row, the value and validity of ITS OWN
    // right key (bowjoin.go:383-400 runs per common column); the gather knows one such column a call, so each key column is a piece of
    // its own and the runs of other columns between them are pieces without one
    StagedCols none;
    bool bad;   // (never raised: the pairs are -1 or in range)
    int32_t run0 = 0;
    for (int32_t i = 0; i <= n_left_cols; i++) {
        const int32_t k = i < n_left_cols ? lkey_of[(size_t)i] : -1;
        if (i < n_left_cols && k < 0) continue;
        GatherIdx il;
        il.i32 = w.out_l.as<const int32_t>();
        il.i32_2 = w.out_r.as<const int32_t>();
        if (i > run0) BG_TRY(synced(c, gather_frame(c, left_cols + run0, i - run0, none, il, total, outs + run0, &bad)));
        if (i == n_left_cols) break;
        il.key_col = 0;
        il.key2 = &s.right[k];
        BG_TRY(synced(c, gather_frame(c, left_cols + i, 1, s.left[k], il, total, outs + i, &bad)));
        run0 = i + 1;
    }
    GatherIdx ir;
    ir.i32 = w.out_r.as<const int32_t>();
    BG_TRY(synced(c, gather_frame(c, rcols.data(), n_rest, none, ir, total, outs + n_left_cols, &bad)));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "gather_kernel");
    return 0;
}

}  // extern "C"
