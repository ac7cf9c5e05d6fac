// join_api.cpp — C-ABI entry points of Bow.InnerJoin / OuterJoin (reference bowjoin.go:12-125; getCommonRows :161-186; the fills
// :188-574): bowgpu_join_rows, bowgpu_join.  Host code validates, prepares residency and puts the kernels of join.hip around the argsort
// of Bow.SortByCol and the mask pass and scan of Bow.Filter; no key is compared and no row is moved on the CPU.
#include <string.h>

#include <vector>

#include "common.h"
#include "join_host.h"

using namespace bowgpu;

namespace bowgpu {

int join_side_limit(int64_t n, const char *side) {
    if (n >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the %s frame has %lld rows: the device join serves fewer than 2^31 = 2147483648 rows", side, (long long)n);
    return 0;
}

int join_key_checks(const bowgpu_col *k, const char *side) {
    if (!movable_type(k->type)) return fail(BOWGPU_ERR_UNSUPPORTED, "%s join column is of unsupported type (Int64 / Float64 only)", side);
    if (k->length < 0 || k->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (!residency_ok(k->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", k->residency);
    return join_side_limit(k->length, side);
}

int join_kind_check(int32_t kind) {
    if (kind != BOWGPU_JOIN_INNER && kind != BOWGPU_JOIN_OUTER) return fail(BOWGPU_ERR_ARG, "unknown join kind %d", kind);
    return 0;
}

int join_types_check(const bowgpu_col *l, const bowgpu_col *r) {   // bowjoin.go:135-139, up to the column name
    if (l->type != r->type) return fail(BOWGPU_ERR_TYPE, "left and right bow on join columns are of incompatible types");
    return 0;
}

int join_rows_limit(int64_t rows) {
    if (rows >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the join has %lld rows: the device join serves fewer than 2^31 = 2147483648 rows", (long long)rows);
    return 0;
}

}  // namespace bowgpu

namespace {

// the right side: [rows with a null key, row order | rows with a value, key order, ties in row order] and the sorted images
int right_side(Ctx *c, const bowgpu_col *rkey, JoinWork *w) {
    const int64_t r = rkey->length;
    BG_TRY(devcol_prepare(c, rkey, &w->rk, true, true));   // (counts the nulls where the caller said -1)
    w->rn = w->rk.null_count;
    w->rv = r - w->rn;
    BG_TRY(w->index.alloc((size_t)r * 4));
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(w->rk.values);
    const uint32_t *vrows = nullptr;
    if (w->rn > 0) {   // the validity mask, its scan, and the rows of both kinds with the values of the valid ones
        TileRecords t;
        BG_TRY(valid_rows_scanned(c, w->rk, &w->vw, &t));
        if (w->vw.selected != w->rv) return fail(BOWGPU_ERR_ARG, "right join column states %lld nulls, its bitmap has %lld", (long long)w->rn, (long long)(r - w->vw.selected));
        BG_TRY(w->vrows.alloc((size_t)(w->rv > 0 ? w->rv : 1) * 4));
        BG_TRY(w->ckeys.alloc((size_t)(w->rv > 0 ? w->rv : 1) * 8));
        BG_TRY(launch_join_split_rows(c, t.mask, t.tile_counts, r, keys, w->vrows.as<uint32_t>(), w->ckeys.as<uint64_t>(), w->index.as<uint32_t>()));
        keys = w->ckeys.as<const uint64_t>();
        vrows = w->vrows.as<const uint32_t>();
    }
    if (w->rv == 0) return 0;
    int32_t sorted = 0;
    int rc;
    if (w->rn > 0) {
        const bowgpu_col ck = device_col(keys, w->rv, rkey->type);
        DevCol dk;
        dk.values = keys;
        dk.length = w->rv;
        dk.type = rkey->type;
        rc = argsort_device(c, &ck, dk, &w->sw, &sorted);
    } else {
        rc = argsort_device(c, rkey, w->rk, &w->sw, &sorted);
    }
    if (rc == BOWGPU_ERR_UNSUPPORTED)
        return fail(BOWGPU_ERR_UNSUPPORTED, "right join column holds a NaN among its valid rows: it equals nothing in the reference and Less is no order "
                                            "there (the caller keeps the reference path)");
    BG_TRY(rc);
    JoinRightArgs a;
    memset(&a, 0, sizeof a);
    a.vrows = vrows;
    a.keys = keys;
    a.index = w->index.as<uint32_t>();
    a.rn = w->rn;
    a.rv = w->rv;
    a.is_float = rkey->type == BOWGPU_FLOAT64;
    if (sorted) {   // a key already in order cost the one read that found it so: the images are made here
        BG_TRY(w->simg.alloc((size_t)w->rv * 8));
        a.img_out = w->simg.as<uint64_t>();
    } else {
        a.perm = w->sw.perm();
    }
    return launch_join_right_index(c, a);
}

const uint64_t *sorted_images(const JoinWork &w) {
    return w.simg.p ? w.simg.as<const uint64_t>() : w.sw.keys[w.sw.cur].as<const uint64_t>();
}

}  // namespace

namespace bowgpu {

// the count: the right side, the probe, the right-only rows.  *rows / *pairs; nothing of the caller's is written.  Synchronises
int join_count_device(Ctx *c, const bowgpu_col *lkey, int32_t lkey_col, const bowgpu_col *rkey, int32_t kind, JoinWork *w, int64_t *rows, int64_t *pairs) {
    const int64_t n_left = lkey->length, n_right = rkey->length;
    const bool outer = kind == BOWGPU_JOIN_OUTER;
    w->n_left = n_left;
    w->n_right = n_right;
    w->probed = true;
    BG_TRY(right_side(c, rkey, w));
    DevCol *lk = w->left.add(lkey_col);
    const bowgpu_col lcol = uncounted(*lkey);
    BG_TRY(devcol_prepare(c, &lcol, lk, true, true));
    w->lk = lk;
    BG_TRY(w->first.alloc((size_t)n_left * 4));
    BG_TRY(w->count.alloc((size_t)n_left * 4));
    BG_TRY(w->starts.alloc((size_t)n_left * 4));
    BG_TRY(w->head.alloc((size_t)(w->rv > 0 ? w->rv : 1)));
    BG_TRY(w->stats.alloc(sizeof(JoinStats)));
    BG_HIP(hipMemsetAsync(w->head.p, 0, w->head.bytes, c->stream));
    BG_HIP(hipMemsetAsync(w->stats.p, 0, sizeof(JoinStats), c->stream));
    JoinProbeArgs p;
    memset(&p, 0, sizeof p);
    p.keys = reinterpret_cast<const uint64_t *>(lk->values);
    p.vbits = lk->vbits;
    p.vbit0 = lk->vbit0;
    p.n = n_left;
    p.simg = w->rv > 0 ? sorted_images(*w) : nullptr;
    p.rn = w->rn;
    p.rv = w->rv;
    p.first = w->first.as<uint32_t>();
    p.count = w->count.as<uint32_t>();
    p.out_count = w->starts.as<uint32_t>();
    p.head = w->head.as<uint8_t>();
    p.stats = w->stats.as<JoinStats>();
    p.is_float = lkey->type == BOWGPU_FLOAT64;
    p.outer = outer;
    BG_TRY(launch_join_probe(c, p));
    JoinStats st;
    BG_HIP(hipMemcpyAsync(&st, w->stats.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (st.nan)
        return fail(BOWGPU_ERR_UNSUPPORTED, "left join column holds a NaN among its valid rows: it equals nothing in the reference (the caller keeps the "
                                            "reference path)");
    *pairs = (int64_t)st.pairs;
    w->rows_left = outer ? (int64_t)(st.pairs + ((unsigned long long)n_left - st.matched_left)) : (int64_t)st.pairs;
    BG_TRY(join_rows_limit(w->rows_left));
    w->tail = 0;
    if (outer) {   // one bit per right ROW that occurs in no pair, then the mask pass that counts them per tile
        BG_TRY(w->ubits.alloc((size_t)((n_right + 31) >> 5) * 4 + 8));
        BG_HIP(hipMemsetAsync(w->ubits.p, 0, w->ubits.bytes, c->stream));
        BG_TRY(launch_join_unmatched(c, w->index.as<const uint32_t>(), p.simg, p.head, p.stats, w->rn, w->rv, w->ubits.as<uint32_t>()));
        FilterMaskArgs m;
        memset(&m, 0, sizeof m);
        m.n = n_right;
        m.and_mask = w->ubits.as<const uint8_t>();
        BG_TRY(mask_work_prepare(c, n_right, &w->uw, &m.t));
        BG_TRY(launch_filter_mask(c, m));
        BG_TRY(mask_work_collect(c, &w->uw));
        w->tail = w->uw.selected;
    }
    *rows = w->rows_left + w->tail;
    return join_rows_limit(*rows);
}

// the index pairs of the `rows` output rows, as 32-bit rows in the workspace (no synchronise)
int join_expand_device(Ctx *c, int32_t kind, JoinWork *w, int64_t rows) {
    BG_TRY(w->out_l.alloc((size_t)rows * 4));
    BG_TRY(w->out_r.alloc((size_t)rows * 4));
    JoinExpandArgs e;
    memset(&e, 0, sizeof e);
    e.n_left = w->n_left;
    e.rows_left = w->rows_left;
    e.rows = rows;
    e.out_l = w->out_l.as<int32_t>();
    e.out_r = w->out_r.as<int32_t>();
    e.outer = kind == BOWGPU_JOIN_OUTER;
    if (w->probed) {
        BG_TRY(w->sums.alloc((size_t)((w->n_left + 4095) / 4096) * 4));
        BG_TRY(launch_scan_u32(c, w->starts.as<uint32_t>(), w->n_left, w->sums.as<uint32_t>()));
        e.starts = w->starts.as<const uint32_t>();
        e.first = w->first.as<const uint32_t>();
        e.count = w->count.as<const uint32_t>();
        e.index = w->index.as<const uint32_t>();
        if (w->tail > 0) {   // the right-only rows in row order: the scan of the tile counts and the rows of the set bits
            const int64_t ntiles = (w->n_right + kFilterTileRows - 1) / kFilterTileRows;
            BG_TRY(w->uw.sums.alloc((size_t)((ntiles + 4095) / 4096) * 4));
            BG_TRY(launch_scan_u32(c, w->uw.tiles.as<uint32_t>(), ntiles, w->uw.sums.as<uint32_t>()));
            BG_TRY(w->urows.alloc((size_t)w->tail * 4));
            BG_TRY(launch_join_split_rows(c, w->uw.mask.as<const unsigned long long>(), w->uw.tiles.as<const uint32_t>(), w->n_right, nullptr,
                                          w->urows.as<uint32_t>(), nullptr, nullptr));
            e.tail_rows = w->urows.as<const uint32_t>();
        }
    }
    return launch_join_expand(c, e);
}

}  // namespace bowgpu

extern "C" {

int bowgpu_join_rows(const bowgpu_col *left_key, const bowgpu_col *right_key, int32_t kind, int64_t *l_idx, int64_t *r_idx, int64_t idx_capacity,
                     int32_t idx_residency, int64_t *rows, int64_t *pairs) {
    if (!rows || !pairs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(join_kind_check(kind));
    if ((left_key == nullptr) != (right_key == nullptr))   // the other frame's length cannot be known: no partial answer
        return fail(BOWGPU_ERR_ARG, "one join column is NULL: give both, or neither for frames without a common column");
    if (left_key) {
        BG_TRY(join_key_checks(left_key, "left"));
        BG_TRY(join_key_checks(right_key, "right"));
        BG_TRY(join_types_check(left_key, right_key));
    }
    const bool fill = l_idx != nullptr || r_idx != nullptr;
    if (fill) {
        if (!l_idx || !r_idx) return fail(BOWGPU_ERR_ARG, "null argument");
        if (!residency_ok(idx_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", idx_residency);
        if (idx_capacity < 0) return fail(BOWGPU_ERR_ARG, "negative index capacity");
    }
    const int64_t n_left = left_key ? left_key->length : 0, n_right = right_key ? right_key->length : 0;
    const bool outer = kind == BOWGPU_JOIN_OUTER;
    const bool probe = left_key && right_key && n_left > 0 && n_right > 0;
    *pairs = 0;
    *rows = 0;
    JoinWork w;
    Ctx *c = nullptr;
    if (!probe) {   // no pair list: known without the device
        const int64_t total = outer ? n_left + n_right : 0;
        BG_TRY(join_rows_limit(total));
        *rows = total;
        if (!fill || total == 0) return 0;
        if (idx_capacity < total) return fail(BOWGPU_ERR_ARG, "index buffers have %lld slots, %lld needed", (long long)idx_capacity, (long long)total);
        BG_TRY(ctx_get(&c));
        w.n_left = w.rows_left = n_left;
        w.n_right = w.tail = n_right;
        BG_HIP(hipEventRecord(c->ev0, c->stream));
    } else {
        BG_TRY(ctx_get(&c));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        int64_t nrows = 0, npairs = 0;
        BG_TRY(synced(c, join_count_device(c, left_key, 0, right_key, kind, &w, &nrows, &npairs)));
        if (fill && idx_capacity < nrows)
            return fail(BOWGPU_ERR_ARG, "index buffers have %lld slots, %lld needed", (long long)idx_capacity, (long long)nrows);
        *rows = nrows;
        *pairs = npairs;
        if (!fill || nrows == 0) {
            BG_HIP(hipEventRecord(c->ev1, c->stream));
            BG_HIP(hipStreamSynchronize(c->stream));
            kernel_done(c, "join_probe_kernel");
            return 0;
        }
    }
    const int64_t n = *rows;
    DevBuf wide_l, wide_r;
    int64_t *dl = l_idx, *dr = r_idx;
    if (idx_residency != BOWGPU_DEVICE) {
        BG_TRY(wide_l.alloc((size_t)n * 8));
        BG_TRY(wide_r.alloc((size_t)n * 8));
        dl = wide_l.as<int64_t>();
        dr = wide_r.as<int64_t>();
    } else if ((reinterpret_cast<uintptr_t>(l_idx) | reinterpret_cast<uintptr_t>(r_idx)) & 7) {
        return fail(BOWGPU_ERR_ARG, "index buffer must be 8-byte aligned");
    }
    BG_TRY(synced(c, join_expand_device(c, kind, &w, n)));
    BG_TRY(synced(c, launch_widen(c, nullptr, w.out_l.as<const int32_t>(), n, dl)));
    BG_TRY(synced(c, launch_widen(c, nullptr, w.out_r.as<const int32_t>(), n, dr)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_TRY(synced(c, aux_out(c, l_idx, dl, (size_t)n * 8, idx_residency)));
    BG_TRY(synced(c, aux_out(c, r_idx, dr, (size_t)n * 8, idx_residency)));
    BG_HIP(hipStreamSynchronize(c->stream));
    kernel_done(c, "join_expand_kernel");
    return 0;
}

int bowgpu_join(const bowgpu_col *left_cols, int32_t n_left_cols, int32_t left_key, const bowgpu_col *right_cols, int32_t n_right_cols,
                int32_t right_key, int32_t kind, bowgpu_out *outs, int64_t *rows) {
    if (!rows) return fail(BOWGPU_ERR_ARG, "null argument");
    if (n_left_cols < 0 || n_right_cols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if ((n_left_cols > 0 && !left_cols) || (n_right_cols > 0 && !right_cols)) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(join_kind_check(kind));
    const int64_t n_left = n_left_cols > 0 ? left_cols[0].length : 0, n_right = n_right_cols > 0 ? right_cols[0].length : 0;
    BG_TRY(frame_cols_checks(left_cols, n_left_cols, n_left, true));
    BG_TRY(frame_cols_checks(right_cols, n_right_cols, n_right, true));
    const bool keyed = !(left_key == -1 && right_key == -1);   // -1 / -1: the frames have no common column
    if (keyed) {
        if (left_key < 0 || left_key > n_left_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the left frame", left_key);
        if (right_key < 0 || right_key > n_right_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the right frame", right_key);
        BG_TRY(join_types_check(&left_cols[left_key], &right_cols[right_key]));
    }
    BG_TRY(join_side_limit(n_left, "left"));
    BG_TRY(join_side_limit(n_right, "right"));
    // the right columns without the key, as the frame the outputs behind the left columns come from
    std::vector<bowgpu_col> rcols;
    for (int i = 0; i < n_right_cols; i++)
        if (!keyed || i != right_key) rcols.push_back(right_cols[i]);
    const int32_t n_rest = (int32_t)rcols.size(), n_outs = n_left_cols + n_rest;
    if (n_outs > 0 && !outs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(outs_checks(outs, n_outs, -1));
    const bool outer = kind == BOWGPU_JOIN_OUTER;
    const bool probe = keyed && n_left > 0 && n_right > 0;
    JoinWork w;
    Ctx *c = nullptr;
    int64_t total = 0, npairs = 0;
    if (!probe) {   // no pair list: the row count is known without the device
        total = outer ? n_left + n_right : 0;
        BG_TRY(join_rows_limit(total));
    } else {
        BG_TRY(ctx_get(&c));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        BG_TRY(synced(c, join_count_device(c, &left_cols[left_key], left_key, &right_cols[right_key], kind, &w, &total, &npairs)));
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
    if (n_outs == 0) return 0;
    if (!probe) {   // an OuterJoin with an empty side or without a common column: the other rows padded with nulls - the gather's work
        BG_TRY(ctx_get(&c));
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        w.n_left = w.rows_left = n_left;
        w.n_right = w.tail = n_right;
        if (keyed) BG_TRY(devcol_prepare(c, &right_cols[right_key], &w.rk, true, true));
    }
    BG_TRY(synced(c, join_expand_device(c, kind, &w, total)));
    const bool device_out = any_device_out(outs, n_outs);
    // the key column takes the left row's value, and the RIGHT key's value and validity on a right-only row (bowjoin.go:397)
    GatherIdx il, ir;
    il.i32 = w.out_l.as<const int32_t>();
    ir.i32 = il.i32_2 = w.out_r.as<const int32_t>();
    il.key_col = keyed ? left_key : -1;
    il.key2 = &w.rk;
    bool bad;   // (never raised: the pairs are -1 or in range)
    BG_TRY(synced(c, gather_frame(c, left_cols, n_left_cols, w.left, il, total, outs, &bad)));
    StagedCols none;
    BG_TRY(synced(c, gather_frame(c, rcols.data(), n_rest, none, ir, total, outs + n_left_cols, &bad)));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "gather_kernel");
    return 0;
}

}  // extern "C"
