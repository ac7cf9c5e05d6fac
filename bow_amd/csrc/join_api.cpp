// join_api.cpp — C-ABI entry points of Bow.InnerJoin / OuterJoin (reference bowjoin.go:12-125; getCommonCols :128-155; getCommonRows
// :161-186; the fills :188-574): bowgpu_join_rows, bowgpu_join, bowgpu_join_keys_rows, bowgpu_join_keys.  The four are argument adaptors
// of two drivers - the rows of a join, the joined frame - that take the call's keys as a list of 0 .. BOWGPU_JOIN_MAX_KEYS pairs.  One
// probe key per side: the staged pair itself, or the surrogates of several (join_surrogate.cpp).  Host code validates, prepares residency
// and puts the kernels of join.hip around the argsort of Bow.SortByCol and the mask pass and scan of Bow.Filter; no key is compared and no
// row is moved on the CPU.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "join_host.h"

using namespace bowgpu;

namespace {

constexpr int64_t kJoinMaxRows = (int64_t)1 << 31;   // rows inside the kernels are 32 bits wide

// one key pair of a call: the two columns, and the frame columns they are (-1: the call has no frames)
struct JoinKey {
    const bowgpu_col *l, *r;
    int32_t lcol, rcol;
};

// ---------------------------------------------------------------- the checks
int join_side_limit(int64_t n, const char *side) {
    if (n >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the %s frame has %lld rows: the device join serves fewer than 2^31 = 2147483648 rows", side, (long long)n);
    return 0;
}

int both_sides_limit(int64_t n_left, int64_t n_right) {   // the surrogate pass sorts both sides as one column, and the argsort is 31-bit
    if (n_left + n_right >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the frames have %lld + %lld rows: the device join on several columns serves fewer than 2^31 = 2147483648 "
                                            "rows on both sides together", (long long)n_left, (long long)n_right);
    return 0;
}

int join_rows_limit(int64_t rows) {
    if (rows >= kJoinMaxRows)
        return fail(BOWGPU_ERR_UNSUPPORTED, "the join has %lld rows: the device join serves fewer than 2^31 = 2147483648 rows", (long long)rows);
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

// the key arrays of the several-keys entry points, before an adaptor reads them
int key_arrays_check(int32_t n_keys, const void *left_keys, const void *right_keys) {
    if (n_keys < 0) return fail(BOWGPU_ERR_ARG, "negative key count");
    if (n_keys > BOWGPU_JOIN_MAX_KEYS)
        return fail(BOWGPU_ERR_UNSUPPORTED, "%d join columns: the device join serves at most BOWGPU_JOIN_MAX_KEYS = %d", n_keys, BOWGPU_JOIN_MAX_KEYS);
    if (n_keys > 0 && (!left_keys || !right_keys)) return fail(BOWGPU_ERR_ARG, "null argument");
    return 0;
}

// the rows driver's: the key columns are the call's only columns
int join_rows_checks(const JoinKey *keys, int32_t n_keys, int32_t kind, const int64_t *l_idx, const int64_t *r_idx, int64_t idx_capacity,
                     int32_t idx_residency, const int64_t *rows, const int64_t *pairs) {
    if (!rows || !pairs) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(join_kind_check(kind));
    for (int32_t k = 0; k < n_keys; k++) {
        BG_TRY(join_key_checks(keys[k].l, "left"));
        BG_TRY(join_key_checks(keys[k].r, "right"));
        if (keys[k].l->length != keys[0].l->length || keys[k].r->length != keys[0].r->length) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        BG_TRY(join_types_check(keys[k].l, keys[k].r));
    }
    if (n_keys >= 2) BG_TRY(both_sides_limit(keys[0].l->length, keys[0].r->length));
    if (l_idx != nullptr || r_idx != nullptr) {
        if (!l_idx || !r_idx) return fail(BOWGPU_ERR_ARG, "null argument");
        if (!residency_ok(idx_residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", idx_residency);
        if (idx_capacity < 0) return fail(BOWGPU_ERR_ARG, "negative index capacity");
    }
    return 0;
}

// the frame driver's; keys[k].l / .r: filled in from the frame columns once those are known to exist
int join_frame_checks(const bowgpu_col *left_cols, int32_t n_left_cols, const bowgpu_col *right_cols, int32_t n_right_cols, JoinKey *keys, int32_t n_keys,
                      int32_t kind, const bowgpu_out *outs, const int64_t *rows) {
    if (!rows) return fail(BOWGPU_ERR_ARG, "null argument");
    if (n_left_cols < 0 || n_right_cols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if ((n_left_cols > 0 && !left_cols) || (n_right_cols > 0 && !right_cols)) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(join_kind_check(kind));
    const int64_t n_left = n_left_cols > 0 ? left_cols[0].length : 0, n_right = n_right_cols > 0 ? right_cols[0].length : 0;
    BG_TRY(frame_cols_checks(left_cols, n_left_cols, n_left, true));
    BG_TRY(frame_cols_checks(right_cols, n_right_cols, n_right, true));
    for (int32_t k = 0; k < n_keys; k++) {
        if (keys[k].lcol < 0 || keys[k].lcol > n_left_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the left frame", keys[k].lcol);
        if (keys[k].rcol < 0 || keys[k].rcol > n_right_cols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d' in the right frame", keys[k].rcol);
        for (int32_t j = 0; j < k; j++) {
            if (keys[j].lcol == keys[k].lcol) return fail(BOWGPU_ERR_ARG, "left column %d is listed twice among the join columns", keys[k].lcol);
            if (keys[j].rcol == keys[k].rcol) return fail(BOWGPU_ERR_ARG, "right column %d is listed twice among the join columns", keys[k].rcol);
        }
        keys[k].l = &left_cols[keys[k].lcol];
        keys[k].r = &right_cols[keys[k].rcol];
    }
    for (int32_t k = 0; k < n_keys; k++) BG_TRY(join_types_check(keys[k].l, keys[k].r));
    BG_TRY(join_side_limit(n_left, "left"));
    BG_TRY(join_side_limit(n_right, "right"));
    if (n_keys >= 2) BG_TRY(both_sides_limit(n_left, n_right));
    const int32_t n_outs = n_left_cols + n_right_cols - n_keys;
    if (n_outs > 0 && !outs) return fail(BOWGPU_ERR_ARG, "null argument");
    return outs_checks(outs, n_outs, -1);
}

// ---------------------------------------------------------------- the call's keys on the device
// The left frame is gathered in pieces that hold at most one key column each: cut after every key column but the last one in frame
// order.  Piece p is the columns [start[p], start[p + 1]) with key pair key[p]'s column (-1: the one piece of a call without keys);
// rel[k]: the index of key pair k's column within its piece
struct LeftPieces {
    int32_t n = 1, start[BOWGPU_JOIN_MAX_KEYS + 1] = {0}, key[BOWGPU_JOIN_MAX_KEYS] = {-1}, rel[BOWGPU_JOIN_MAX_KEYS] = {0};
};

LeftPieces left_pieces(const JoinKey *keys, int32_t n_keys, int32_t n_left_cols) {
    LeftPieces p;
    for (int32_t k = 0; k < n_keys; k++) p.key[k] = k;
    std::sort(p.key, p.key + n_keys, [keys](int32_t a, int32_t b) { return keys[a].lcol < keys[b].lcol; });
    p.n = n_keys > 1 ? n_keys : 1;
    for (int32_t i = 1; i < p.n; i++) p.start[i] = keys[p.key[i - 1]].lcol + 1;
    p.start[p.n] = n_left_cols;
    for (int32_t i = 0; i < n_keys; i++) p.rel[p.key[i]] = keys[p.key[i]].lcol - p.start[i];
    return p;
}

// The key columns of both sides staged (where they are host-resident) once a call: what the probe keys are or are made from, what the
// gather finds a left key column under (left[k]: it alone, by its index within its piece) and reads a right-only row's key from
struct StagedKeys {
    StagedCols left[BOWGPU_JOIN_MAX_KEYS];
    DevCol right[BOWGPU_JOIN_MAX_KEYS];
    KeyPair pairs[BOWGPU_JOIN_MAX_KEYS];
};

// lrel: LeftPieces::rel; nullptr: the call has no frames.  The kernels read the bitmaps anyway, so no null count is taken first - but
// for the right key of a call on one key: the right side splits on its nulls (counted here where the caller said -1)
int stage_keys(Ctx *c, const JoinKey *keys, int32_t n_keys, const int32_t *lrel, StagedKeys *s) {
    for (int32_t k = 0; k < n_keys; k++) {
        DevCol *l = s->left[k].add(lrel ? lrel[k] : 0);
        const bowgpu_col lcol = uncounted(*keys[k].l), rcol = n_keys == 1 ? *keys[k].r : uncounted(*keys[k].r);
        BG_TRY(devcol_prepare(c, &lcol, l, true, true));
        BG_TRY(devcol_prepare(c, &rcol, &s->right[k], true, true));
        s->pairs[k] = {l, &s->right[k]};
    }
    return 0;
}

// ---------------------------------------------------------------- the join on one probe key per side
// everything a call keeps on the device between its count and its gather
struct JoinWork {
    MaskWork vw, uw;           // the right key's validity; the right-only rows
    SortWork sw;
    DevBuf vrows, ckeys, index, simg, first, count, starts, sums, head, stats, ubits, urows, out_l, out_r;
    int64_t n_left = 0, n_right = 0, rn = 0, rv = 0, rows_left = 0, tail = 0;
    bool probed = false;       // false: no pair list (an empty side, no common column) - identity rows
};

// the right side: [rows with a null key, row order | rows with a value, key order, ties in row order] and the sorted images.
// rcol: the key as the call states it (the argsort reads a registered column in place)
int right_side(Ctx *c, const bowgpu_col *rcol, const DevCol &rk, JoinWork *w) {
    const int64_t r = rk.length;
    w->rn = rk.null_count;
    w->rv = r - w->rn;
    BG_TRY(w->index.alloc((size_t)r * 4));
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(rk.values);
    const uint32_t *vrows = nullptr;
    if (w->rn > 0) {   // the validity mask, its scan, and the rows of both kinds with the values of the valid ones
        TileRecords t;
        BG_TRY(valid_rows_scanned(c, rk, &w->vw, &t));
        if (w->vw.selected != w->rv) return fail(BOWGPU_ERR_ARG, "right join column states %lld nulls, its bitmap has %lld", (long long)w->rn, (long long)(r - w->vw.selected));
        BG_TRY(w->vrows.alloc((size_t)(w->rv > 0 ? w->rv : 1) * 4));
        BG_TRY(w->ckeys.alloc((size_t)(w->rv > 0 ? w->rv : 1) * 8));
        BG_TRY(launch_join_split_rows(c, t.mask, t.tile_counts, r, keys, w->vrows.as<uint32_t>(), w->ckeys.as<uint64_t>(), w->index.as<uint32_t>()));
        keys = w->ckeys.as<const uint64_t>();
        vrows = w->vrows.as<const uint32_t>();
    }
    if (w->rv == 0) return 0;
    int32_t sorted = 0;
    const int rc = w->rn > 0 ? argsort_device(c, DeviceKey(keys, w->rv, rk.type), &w->sw, &sorted) : argsort_device(c, rcol, rk, &w->sw, &sorted);
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
    a.is_float = rk.type == BOWGPU_FLOAT64;
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

// the count on the prepared keys lk / rk: the right side, the probe, the right-only rows.  *rows / *pairs; nothing of the caller's is
// written.  Synchronises: neither key is read after it
int join_count_device(Ctx *c, const DevCol &lk, const bowgpu_col *rcol, const DevCol &rk, int32_t kind, JoinWork *w, int64_t *rows, int64_t *pairs) {
    const int64_t n_left = lk.length, n_right = rk.length;
    const bool outer = kind == BOWGPU_JOIN_OUTER;
    w->n_left = n_left;
    w->n_right = n_right;
    w->probed = true;
    BG_TRY(right_side(c, rcol, rk, w));
    BG_TRY(w->first.alloc((size_t)n_left * 4));
    BG_TRY(w->count.alloc((size_t)n_left * 4));
    BG_TRY(w->starts.alloc((size_t)n_left * 4));
    BG_TRY(w->head.alloc((size_t)(w->rv > 0 ? w->rv : 1)));
    BG_TRY(w->stats.alloc(sizeof(JoinStats)));
    BG_HIP(hipMemsetAsync(w->head.p, 0, w->head.bytes, c->stream));
    BG_HIP(hipMemsetAsync(w->stats.p, 0, sizeof(JoinStats), c->stream));
    JoinProbeArgs p;
    memset(&p, 0, sizeof p);
    p.keys = reinterpret_cast<const uint64_t *>(lk.values);
    p.vbits = lk.vbits;
    p.vbit0 = lk.vbit0;
    p.n = n_left;
    p.simg = w->rv > 0 ? sorted_images(*w) : nullptr;
    p.rn = w->rn;
    p.rv = w->rv;
    p.first = w->first.as<uint32_t>();
    p.count = w->count.as<uint32_t>();
    p.out_count = w->starts.as<uint32_t>();
    p.head = w->head.as<uint8_t>();
    p.stats = w->stats.as<JoinStats>();
    p.is_float = lk.type == BOWGPU_FLOAT64;
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

// ---------------------------------------------------------------- the steps of the two drivers
// a call from its count on
struct JoinCall {
    Ctx *c = nullptr;
    JoinWork w;
    StagedKeys s;
    DevBuf packed;             // the surrogate column of several key pairs
    bool probe = false;        // there is a pair list to make: keys, and rows on both sides
    int64_t total = 0, pairs = 0;
};

// The keys staged, the probe keys and the count on them.  One key pair: the staged pair itself.  Several: the two halves of their
// surrogate column.  keep_keys: the gather will read the staged keys; else those of several pairs go back before the join proper
// takes its workspace
int probe_count(const JoinKey *keys, int32_t n_keys, const int32_t *lrel, int32_t kind, bool keep_keys, JoinCall *j) {
    Ctx *c = j->c;
    BG_TRY(synced(c, stage_keys(c, keys, n_keys, lrel, &j->s)));
    if (n_keys == 1) return synced(c, join_count_device(c, *j->s.pairs[0].l, keys[0].r, *j->s.pairs[0].r, kind, &j->w, &j->total, &j->pairs));
    const int64_t n_left = keys[0].l->length, n_right = keys[0].r->length;
    BG_TRY(synced(c, surrogate_keys(c, j->s.pairs, n_keys, n_left, n_right, &j->packed)));
    if (!keep_keys) j->s = StagedKeys();
    const DeviceKey ls(j->packed.p, n_left, BOWGPU_INT64), rs(j->packed.as<uint64_t>() + n_left, n_right, BOWGPU_INT64);
    return synced(c, join_count_device(c, ls.dev, &rs.col, rs.dev, kind, &j->w, &j->total, &j->pairs));
}

// j->total.  Without a pair list it is known without the device; else the device is taken, the call's event bracket opened and the count run
int join_total(const JoinKey *keys, int32_t n_keys, const int32_t *lrel, int64_t n_left, int64_t n_right, int32_t kind, bool keep_keys, JoinCall *j) {
    j->probe = n_keys > 0 && n_left > 0 && n_right > 0;
    if (!j->probe) {
        j->total = kind == BOWGPU_JOIN_OUTER ? n_left + n_right : 0;
        return join_rows_limit(j->total);
    }
    BG_TRY(ctx_get(&j->c));
    BG_HIP(hipEventRecord(j->c->ev0, j->c->stream));
    return probe_count(keys, n_keys, lrel, kind, keep_keys, j);
}

// an OuterJoin without a pair list has rows all the same - all left rows, then all right rows: the device is taken for them here
int identity_rows(int64_t n_left, int64_t n_right, JoinCall *j) {
    BG_TRY(ctx_get(&j->c));
    j->w.n_left = j->w.rows_left = n_left;
    j->w.n_right = j->w.tail = n_right;
    BG_HIP(hipEventRecord(j->c->ev0, j->c->stream));
    return 0;
}

// The left frame, piece by piece.  EVERY key column takes the left row's value and, on a right-only row, the value and validity of ITS
// OWN right key (bowjoin.go:383-400 runs per common column); the gather knows one such column a call
int gather_left(const bowgpu_col *left_cols, const LeftPieces &p, const JoinCall &j, bowgpu_out *outs) {
    StagedCols none;
    bool bad;   // (never raised: the pairs are -1 or in range)
    for (int32_t i = 0; i < p.n; i++) {
        const int32_t k = p.key[i], c0 = p.start[i];
        GatherIdx il;
        il.i32 = j.w.out_l.as<const int32_t>();
        il.i32_2 = j.w.out_r.as<const int32_t>();
        if (k >= 0) {
            il.key_col = p.rel[k];
            il.key2 = j.s.pairs[k].r;
        }
        const StagedCols &have = k >= 0 ? j.s.left[k] : none;
        BG_TRY(synced(j.c, gather_frame(j.c, left_cols + c0, p.start[i + 1] - c0, have, il, j.total, outs + c0, &bad)));
    }
    return 0;
}

// ---------------------------------------------------------------- the two drivers
int join_rows(const JoinKey *keys, int32_t n_keys, int32_t kind, int64_t *l_idx, int64_t *r_idx, int64_t idx_capacity, int32_t idx_residency,
              int64_t *rows, int64_t *pairs) {
    BG_TRY(join_rows_checks(keys, n_keys, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs));
    const bool fill = l_idx != nullptr || r_idx != nullptr;
    const int64_t n_left = n_keys > 0 ? keys[0].l->length : 0, n_right = n_keys > 0 ? keys[0].r->length : 0;
    *pairs = 0;
    *rows = 0;
    JoinCall j;
    BG_TRY(join_total(keys, n_keys, nullptr, n_left, n_right, kind, false, &j));
    const int64_t n = j.total;
    if (fill && idx_capacity < n) return fail(BOWGPU_ERR_ARG, "index buffers have %lld slots, %lld needed", (long long)idx_capacity, (long long)n);
    *rows = n;
    *pairs = j.pairs;
    if (!fill || n == 0) {
        if (!j.probe) return 0;
        BG_HIP(hipEventRecord(j.c->ev1, j.c->stream));
        BG_HIP(hipStreamSynchronize(j.c->stream));
        kernel_done(j.c, "join_probe_kernel");
        return 0;
    }
    if (!j.probe) BG_TRY(identity_rows(n_left, n_right, &j));
    Ctx *c = j.c;
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
    BG_TRY(synced(c, join_expand_device(c, kind, &j.w, n)));
    BG_TRY(synced(c, launch_widen(c, nullptr, j.w.out_l.as<const int32_t>(), n, dl)));
    BG_TRY(synced(c, launch_widen(c, nullptr, j.w.out_r.as<const int32_t>(), n, dr)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_TRY(synced(c, aux_out(c, l_idx, dl, (size_t)n * 8, idx_residency)));
    BG_TRY(synced(c, aux_out(c, r_idx, dr, (size_t)n * 8, idx_residency)));
    BG_HIP(hipStreamSynchronize(c->stream));
    kernel_done(c, "join_expand_kernel");
    return 0;
}

int join_frame(const bowgpu_col *left_cols, int32_t n_left_cols, const bowgpu_col *right_cols, int32_t n_right_cols, JoinKey *keys, int32_t n_keys,
               int32_t kind, bowgpu_out *outs, int64_t *rows) {
    BG_TRY(join_frame_checks(left_cols, n_left_cols, right_cols, n_right_cols, keys, n_keys, kind, outs, rows));
    const int64_t n_left = n_left_cols > 0 ? left_cols[0].length : 0, n_right = n_right_cols > 0 ? right_cols[0].length : 0;
    // the right columns without the keys, as the frame the outputs behind the left columns come from
    std::vector<bowgpu_col> rcols;
    for (int32_t i = 0; i < n_right_cols; i++)
        if (std::none_of(keys, keys + n_keys, [i](const JoinKey &k) { return k.rcol == i; })) rcols.push_back(right_cols[i]);
    const int32_t n_rest = (int32_t)rcols.size(), n_outs = n_left_cols + n_rest;
    const LeftPieces pieces = left_pieces(keys, n_keys, n_left_cols);
    JoinCall j;
    BG_TRY(join_total(keys, n_keys, pieces.rel, n_left, n_right, kind, true, &j));
    const int64_t total = j.total;
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
    if (!j.probe) {   // the other rows padded with nulls - the gather's work; a key column's right partner is read all the same
        BG_TRY(identity_rows(n_left, n_right, &j));
        BG_TRY(synced(j.c, stage_keys(j.c, keys, n_keys, pieces.rel, &j.s)));
    }
    Ctx *c = j.c;
    BG_TRY(synced(c, join_expand_device(c, kind, &j.w, total)));
    const bool device_out = any_device_out(outs, n_outs);
    BG_TRY(gather_left(left_cols, pieces, j, outs));
    StagedCols none;
    GatherIdx ir;
    ir.i32 = j.w.out_r.as<const int32_t>();
    bool bad;
    BG_TRY(synced(c, gather_frame(c, rcols.data(), n_rest, none, ir, total, outs + n_left_cols, &bad)));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (device_out) device_write_epoch_bump();
    kernel_done(c, "gather_kernel");
    return 0;
}

}  // namespace

extern "C" {

int bowgpu_join_rows(const bowgpu_col *left_key, const bowgpu_col *right_key, int32_t kind, int64_t *l_idx, int64_t *r_idx, int64_t idx_capacity,
                     int32_t idx_residency, int64_t *rows, int64_t *pairs) {
    if ((left_key == nullptr) != (right_key == nullptr))   // the other frame's length cannot be known: no partial answer
        return fail(BOWGPU_ERR_ARG, "one join column is NULL: give both, or neither for frames without a common column");
    const JoinKey key = {left_key, right_key, -1, -1};
    return join_rows(&key, left_key ? 1 : 0, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
}

int bowgpu_join(const bowgpu_col *left_cols, int32_t n_left_cols, int32_t left_key, const bowgpu_col *right_cols, int32_t n_right_cols,
                int32_t right_key, int32_t kind, bowgpu_out *outs, int64_t *rows) {
    JoinKey key = {nullptr, nullptr, left_key, right_key};
    const int32_t n_keys = left_key == -1 && right_key == -1 ? 0 : 1;   // -1 / -1: the frames have no common column
    return join_frame(left_cols, n_left_cols, right_cols, n_right_cols, &key, n_keys, kind, outs, rows);
}

int bowgpu_join_keys_rows(const bowgpu_col *left_keys, const bowgpu_col *right_keys, int32_t n_keys, int32_t kind, int64_t *l_idx, int64_t *r_idx,
                          int64_t idx_capacity, int32_t idx_residency, int64_t *rows, int64_t *pairs) {
    BG_TRY(key_arrays_check(n_keys, left_keys, right_keys));
    JoinKey keys[BOWGPU_JOIN_MAX_KEYS];
    for (int32_t k = 0; k < n_keys; k++) keys[k] = {&left_keys[k], &right_keys[k], -1, -1};
    return join_rows(keys, n_keys, kind, l_idx, r_idx, idx_capacity, idx_residency, rows, pairs);
}

int bowgpu_join_keys(const bowgpu_col *left_cols, int32_t n_left_cols, const int32_t *left_keys, const bowgpu_col *right_cols, int32_t n_right_cols,
                     const int32_t *right_keys, int32_t n_keys, int32_t kind, bowgpu_out *outs, int64_t *rows) {
    BG_TRY(key_arrays_check(n_keys, left_keys, right_keys));
    JoinKey keys[BOWGPU_JOIN_MAX_KEYS];
    for (int32_t k = 0; k < n_keys; k++) keys[k] = {nullptr, nullptr, left_keys[k], right_keys[k]};
    return join_frame(left_cols, n_left_cols, right_cols, n_right_cols, keys, n_keys, kind, outs, rows);
}

}  // extern "C"
