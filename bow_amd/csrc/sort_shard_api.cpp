// sort_shard_api.cpp — bowgpu_sort_by_col_sharded: Bow.SortByCol (reference bowsort.go:10-41) over a frame the caller holds as
// row-range shards, one per device.  One library thread per rank (the workers of fanout.cpp) runs: the local sort of the rank's key
// (argsort_device), the exact splitter search across ranks (split_bounds_kernel, bisected by the host), the rank's rows into sorted
// order (the gather), the exchange (every destination pulls its pieces), their concatenation (the append kernel) and, where the
// pulled runs interleave, their stable merge (sort_shard.hip) and one more gather.  No key is compared and no row is moved on the CPU.
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "common.h"
#include "fanout.h"

using namespace bowgpu;

namespace {

constexpr int64_t kSortMaxRows = (int64_t)1 << 31;   // row indices inside a rank are 32 bits wide
// a three-way bisection of at most 2^64 images: 64 probes for a range below 2^64 values, 65 when the keys span all of it
constexpr int kSplitMaxRounds = 65;

thread_local bowgpu_sort_shard_info g_info;          // of the calling thread's last call (bowgpu_sort_by_col_sharded_info)

struct Piece { int src; int64_t a, b; };             // rows [a, b) of rank src's sorted order

struct RankState {
    int64_t n = 0;
    int64_t nulls = 0;               // of the rank's key
    StagedCols have;                 // the key on the rank's device
    const DevCol *dk = nullptr;
    bowgpu_col key;                  // ... as it was staged (without a bitmap that holds no null)
    SortWork w;
    int32_t sorted = 1;
    const uint64_t *skeys = nullptr; // the key in sorted order as the splitter kernels read it
    int32_t smode = kKeyImages;
    uint64_t first_img = 0, last_img = 0;
    DevFrame tmp;                               // the rank's columns in sorted order (a rank that was not in order)
    std::vector<bowgpu_col> src;                // what the destinations pull from: the temporaries, or the input as it lies
    std::vector<int64_t> cut;                   // [world][world + 1], the same on every rank
    std::vector<uint64_t> ends;                 // [world][2]: first / last image of piece (this rank -> d)
    double sort_ms = 0, split_ms = 0, merge_ms = 0;   // kernels of the local sort (device events); wall time of the splitter search; kernels of the merge
    int merge_rounds = 0, sort_passes = 0;
    int rc = 0;
    std::string err;
    void release() {   // on the rank's own thread: the blocks go back to THAT thread's (device's) cache
        tmp.clear();
        w = SortWork();
        have = StagedCols();
        dk = nullptr;
    }
};

struct ShardSort {
    const bowgpu_col *const *cols_by_rank;
    const int32_t *ids;
    int world;
    int32_t ncols, key_col;
    bowgpu_out *const *outs_by_rank;
    uint32_t route;
    int64_t total = 0;
    std::vector<int64_t> T;                  // [world + 1]: T[d] = rows of the ranks below d
    std::vector<RankState> ranks;
    std::vector<uint32_t> bounds[2];         // the splitter exchange, by round parity: [rank][2 * kShardMaxWorld]
    Barrier barrier;
    bool unchanged = false;
    int split_rounds = 0;
};

int read_images(Ctx *c, const RankState &me, const uint32_t *pos, int npos, uint64_t *out) {
    ImageAtArgs a;
    memset(&a, 0, sizeof a);
    a.keys = me.skeys; a.mode = me.smode; a.npos = npos;
    memcpy(a.pos, pos, sizeof(uint32_t) * (size_t)npos);
    static_assert(sizeof(uint64_t) * (sizeof a.pos / sizeof a.pos[0]) == kScrImages.size, "an image per position");
    BG_TRY(scratch_at(c, kScrImages, &a.out));
    BG_TRY(launch_image_at(c, a));
    BG_HIP(hipMemcpyAsync(out, a.out, sizeof(uint64_t) * (size_t)npos, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// step 1a: the key on the rank's device, its nulls
int rank_key(Ctx *c, ShardSort *ss, int r) {
    RankState &me = ss->ranks[r];
    const bowgpu_col *key = &ss->cols_by_rank[r][ss->key_col];
    me.n = key->length;
    if (me.n == 0) return 0;
    me.key = *key;
    const int64_t known = host_count_nulls(key);
    if (known == 0) { me.key.validity = nullptr; me.key.null_count = 0; }
    DevCol *dk = me.have.add(ss->key_col);
    me.dk = dk;
    BG_TRY(synced(c, devcol_prepare(c, &me.key, dk, true, true)));
    me.nulls = dk->null_count > 0 ? dk->null_count : 0;
    if (me.nulls > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %lld nil values", (long long)me.nulls);
    return 0;
}

// step 1b: the local sort - sorted images and a row index, or "already in order" - and the rank's first and last image
int rank_sort(Ctx *c, ShardSort *ss, int r) {
    RankState &me = ss->ranks[r];
    if (me.n == 0) return 0;
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, argsort_device(c, &me.key, *me.dk, &me.w, &me.sorted)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    if (me.sorted) {
        me.skeys = reinterpret_cast<const uint64_t *>(me.dk->values);
        me.smode = me.key.type == BOWGPU_FLOAT64 ? kKeyRawFloat : kKeyRawInt;
    } else {
        me.skeys = me.w.keys[me.w.cur].as<const uint64_t>();
        me.smode = kKeyImages;
    }
    const uint32_t pos[2] = {0u, (uint32_t)(me.n - 1)};
    uint64_t img[2];
    BG_TRY(read_images(c, me, pos, 2, img));
    me.first_img = img[0];
    me.last_img = img[1];
    me.sort_passes = me.w.passes;
    float ms = 0;   // (read_images has synchronised)
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) (void)hipGetLastError();
    me.sort_ms = ms;
    return 0;
}

// step 2, collective: the cut positions of every rank's sorted order, from a bisection of the image range that every rank runs on
// the same numbers.  Every rank reaches every round's barrier; false: some rank failed (its status says how)
bool splitters(Ctx *c, ShardSort *ss, int r, int *rc_out) {
    RankState &me = ss->ranks[r];
    const int world = ss->world;
    me.cut.assign((size_t)world * (world + 1), 0);
    auto cut = [&](int s, int d) -> int64_t & { return me.cut[(size_t)s * (world + 1) + d]; };
    for (int s = 0; s < world; s++) cut(s, world) = ss->ranks[s].n;
    struct Search { int d; uint64_t lo, hi; };
    std::vector<Search> open;
    uint64_t lo0 = ~0ull, hi0 = 0;
    for (int s = 0; s < world; s++)
        if (ss->ranks[s].n > 0) {
            if (ss->ranks[s].first_img < lo0) lo0 = ss->ranks[s].first_img;
            if (ss->ranks[s].last_img > hi0) hi0 = ss->ranks[s].last_img;
        }
    for (int d = 1; d < world; d++) {
        if (ss->T[d] >= ss->total) { for (int s = 0; s < world; s++) cut(s, d) = ss->ranks[s].n; }   // trailing empty ranks: everything lies below
        else if (ss->T[d] > 0) open.push_back({d, lo0, hi0});                                           // (T[d] = 0: nothing does)
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int round = 0; !open.empty(); round++) {
        int rc = 0;
        uint32_t *mine = ss->bounds[round & 1].data() + (size_t)r * 2 * kShardMaxWorld;
        const int ncand = (int)open.size();
        if (round >= kSplitMaxRounds) rc = fail(BOWGPU_ERR_HIP, "internal: the splitter search did not settle in %d rounds", kSplitMaxRounds);
        if (r == 0) ss->split_rounds = round + 1;
        if (rc == 0 && me.n > 0) {
            SplitBoundsArgs a;
            memset(&a, 0, sizeof a);
            a.keys = me.skeys; a.n = me.n; a.mode = me.smode; a.ncand = ncand;
            for (int j = 0; j < ncand; j++) a.cand[j] = open[j].lo + ((open[j].hi - open[j].lo) >> 1);
            static_assert(sizeof(uint32_t) * 2 * (sizeof a.cand / sizeof a.cand[0]) == kScrSplitBounds.size, "two counts per candidate");
            rc = scratch_at(c, kScrSplitBounds, &a.out);
            if (rc == 0) rc = launch_split_bounds(c, a);
            if (rc == 0 && hipMemcpyAsync(mine, a.out, sizeof(uint32_t) * 2 * (size_t)ncand, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                rc = hip_fail(hipGetLastError(), "hipMemcpyAsync (splitter bounds)");
            if (rc == 0 && hipStreamSynchronize(c->stream) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipStreamSynchronize");
        } else if (rc == 0) {
            memset(mine, 0, sizeof(uint32_t) * 2 * (size_t)ncand);
        }
        if (rc != 0) *rc_out = rc;
        if (!ss->barrier.vote(rc == 0)) return false;
        const uint32_t *all = ss->bounds[round & 1].data();
        std::vector<Search> next;
        for (int j = 0; j < ncand; j++) {
            const Search &q = open[j];
            const uint64_t mid = q.lo + ((q.hi - q.lo) >> 1);
            const int64_t t = ss->T[q.d];
            int64_t below = 0, upto = 0;
            for (int s = 0; s < world; s++) {
                below += all[(size_t)s * 2 * kShardMaxWorld + 2 * j];
                upto += all[(size_t)s * 2 * kShardMaxWorld + 2 * j + 1];
            }
            if (upto <= t) next.push_back({q.d, mid + 1, q.hi});         // the row at position t has a larger image
            else if (below > t) next.push_back({q.d, q.lo, mid - 1});    // ... a smaller one
            else {
                // mid IS the image of the row at global position t: its ties are cut in rank order
                int64_t left = t - below;
                for (int s = 0; s < world; s++) {
                    const int64_t lw = all[(size_t)s * 2 * kShardMaxWorld + 2 * j], up = all[(size_t)s * 2 * kShardMaxWorld + 2 * j + 1];
                    const int64_t take = up - lw < left ? up - lw : left;
                    cut(s, q.d) = lw + take;
                    left -= take;
                }
            }
        }
        open.swap(next);
    }
    me.split_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // what every destination receives is what it gave
    for (int d = 0; d < world; d++) {
        int64_t rows = 0;
        for (int s = 0; s < world; s++) {
            if (cut(s, d + 1) < cut(s, d)) { *rc_out = fail(BOWGPU_ERR_HIP, "internal: the cuts of rank %d are not monotone", s); return false; }
            rows += cut(s, d + 1) - cut(s, d);
        }
        if (rows != ss->ranks[d].n) {
            *rc_out = fail(BOWGPU_ERR_HIP, "internal: rank %d would receive %lld rows, it holds %lld", d, (long long)rows, (long long)ss->ranks[d].n);
            return false;
        }
    }
    return true;
}

// step 3: the rank's columns in sorted order (temporaries on its own device, or its input as it lies) and the ends of its pieces
int rank_source(Ctx *c, ShardSort *ss, int r) {
    RankState &me = ss->ranks[r];
    const int world = ss->world, nc = ss->ncols;
    const bowgpu_col *cols = ss->cols_by_rank[r];
    me.src.assign(cols, cols + nc);
    me.ends.assign((size_t)2 * world, 0);
    if (me.n == 0) return 0;
    if (!me.sorted) {
        BG_TRY(me.tmp.alloc(c, nc, me.n, true));
        GatherIdx ix;
        ix.u32 = me.w.perm();
        bool bad = false;
        BG_TRY(gather_frame(c, cols, nc, me.have, ix, me.n, me.tmp.outs.data(), &bad));
        if (bad) return fail(BOWGPU_ERR_HIP, "internal: the sort produced a row index outside the frame");
        me.tmp.as_cols(cols, me.n, me.src.data());
    }
    uint32_t pos[2 * kShardMaxWorld];
    int at[kShardMaxWorld], np = 0;
    for (int d = 0; d < world; d++) {
        const int64_t a = me.cut[(size_t)r * (world + 1) + d], b = me.cut[(size_t)r * (world + 1) + d + 1];
        at[d] = -1;
        if (b > a) { at[d] = np; pos[np++] = (uint32_t)a; pos[np++] = (uint32_t)(b - 1); }
    }
    uint64_t img[2 * kShardMaxWorld];
    if (np > 0) BG_TRY(read_images(c, me, pos, np, img));
    for (int d = 0; d < world; d++)
        if (at[d] >= 0) { me.ends[2 * d] = img[at[d]]; me.ends[2 * d + 1] = img[at[d] + 1]; }
    return 0;   // (the gather's groups and read_images have synchronised: the pieces are complete)
}

// the k sorted runs of a staging frame's key into one permutation: ceil(log2 k) rounds of pairwise stable merges
int merge_runs(Ctx *c, const uint64_t *key, int is_float, const std::vector<uint32_t> &starts, DevBuf img[2], DevBuf idx[2], DevBuf *part, int *cur,
               int *rounds) {
    const int64_t n = starts.back();
    int nruns = (int)starts.size() - 1;
    for (int b = 0; b < 2; b++) {
        BG_TRY(img[b].alloc((size_t)n * 8));
        BG_TRY(idx[b].alloc((size_t)n * 4));
    }
    MergeRoundArgs a;
    memset(&a, 0, sizeof a);
    memcpy(a.start, starts.data(), sizeof(uint32_t) * starts.size());
    BG_TRY(part->alloc((size_t)(n / kMergeTileRows + nruns + 1) * 4));   // (a round's tiles: every pair rounds up once)
    BG_TRY(launch_merge_init(c, key, n, is_float, img[0].as<uint64_t>(), idx[0].as<uint32_t>()));
    *cur = 0;
    while (nruns > 1) {
        a.img_in = img[*cur].as<const uint64_t>(); a.idx_in = idx[*cur].as<const uint32_t>();
        a.img_out = img[*cur ^ 1].as<uint64_t>(); a.idx_out = idx[*cur ^ 1].as<uint32_t>();
        a.part = part->as<uint32_t>();
        BG_TRY(launch_merge_round(c, &a, nruns));
        const int merged = (nruns + 1) / 2;
        for (int j = 0; j < merged; j++) a.start[j] = a.start[2 * j];
        a.start[merged] = (uint32_t)n;
        nruns = merged;
        *cur ^= 1;
        ++*rounds;
    }
    return 0;
}

// steps 4 - 6 on destination d: its pieces pulled in source-rank order and put together by the append kernel - straight into the
// caller's outputs, or into a staging frame that is merged and gathered
int rank_dest(Ctx *c, ShardSort *ss, int d) {
    const int world = ss->world, nc = ss->ncols;
    const int64_t nd = ss->ranks[d].n;
    bowgpu_out *outs = ss->outs_by_rank[d];
    const bowgpu_col *schema = ss->cols_by_rank[0];
    if (nd == 0) {
        for (int i = 0; i < nc; i++) out_empty(&outs[i], schema[i].type);
        return 0;
    }
    std::vector<Piece> pieces;
    const std::vector<int64_t> &cut = ss->ranks[d].cut;
    for (int s = 0; s < world; s++) {
        const int64_t a = cut[(size_t)s * (world + 1) + d], b = cut[(size_t)s * (world + 1) + d + 1];
        if (b > a) pieces.push_back({s, a, b});
    }
    const int np = (int)pieces.size();
    bool interleave = false;
    for (int j = 0; j + 1 < np; j++)
        interleave |= ss->ranks[pieces[j].src].ends[2 * d + 1] > ss->ranks[pieces[j + 1].src].ends[2 * d];
    // a staging frame when the runs have to be merged
    DevFrame stage;
    if (interleave) BG_TRY(stage.alloc(c, nc, nd, true));
    bowgpu_out *target = interleave ? stage.outs.data() : outs;
    std::vector<std::vector<bowgpu_col>> frames(np, std::vector<bowgpu_col>(nc));
    std::vector<const bowgpu_col *> fptr(np);
    for (int f = 0; f < np; f++) fptr[f] = frames[f].data();
    PieceTable table(np);
    for (int g0 = 0; g0 < nc; g0 += kMoveCols) {
        const int gc = nc - g0 < kMoveCols ? nc - g0 : kMoveCols;
        std::vector<DevBuf> lv((size_t)np * gc), lb((size_t)np * gc);   // the pulled pieces of this group
        int64_t nulls[kMoveCols] = {};
        bool count_on_device[kMoveCols] = {};
        for (int f = 0; f < np; f++) {
            const Piece &p = pieces[f];
            for (int i = 0; i < gc; i++) {
                // step 4, the exchange (queued on this rank's stream behind one another; lv / lb live until the group is done, so only a
                // failure synchronises)
                BG_TRY(synced(c, stage_rows(c, ss->ids[d], ss->ids[p.src], ss->ranks[p.src].src[g0 + i], p.a, p.b, &lv[(size_t)f * gc + i],
                                            &lb[(size_t)f * gc + i], &frames[f][g0 + i])));
                if (frames[f][g0 + i].validity) count_on_device[i] = true;
            }
        }
        std::vector<DevCol> staged;
        MoveGroup g;
        g.cols = MoveCols();
        BG_TRY(move_group_outputs(c, nc, g0, target, nd, &g));
        unsigned long long valid[kMoveCols] = {};
        BG_TRY(synced(c, append_launch(c, fptr.data(), np, g0, nd, g, &staged, &table, count_on_device, valid)));
        BG_TRY(move_group_finish(c, &g, schema, g0, nd, nulls));
        for (int i = 0; i < gc; i++)
            if (count_on_device[i]) target[g0 + i].null_count = nd - (int64_t)valid[i];
    }
    if (interleave) {
        std::vector<uint32_t> starts(np + 1);
        int64_t at = 0;
        for (int f = 0; f < np; f++) { starts[f] = (uint32_t)at; at += pieces[f].b - pieces[f].a; }
        starts[np] = (uint32_t)at;
        DevBuf img[2], idx[2], part;
        int cur = 0;
        RankState &me = ss->ranks[d];
        BG_HIP(hipEventRecord(c->ev0, c->stream));
        BG_TRY(synced(c, merge_runs(c, reinterpret_cast<const uint64_t *>(stage.outs[ss->key_col].values), schema[ss->key_col].type == BOWGPU_FLOAT64,
                                    starts, img, idx, &part, &cur, &me.merge_rounds)));
        BG_HIP(hipEventRecord(c->ev1, c->stream));
        BG_HIP(hipEventSynchronize(c->ev1));   // (the gather below records ev1 again)
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) (void)hipGetLastError();
        me.merge_ms = ms;
        std::vector<bowgpu_col> scols(nc);
        stage.as_cols(schema, nd, scols.data());
        GatherIdx ix;
        ix.u32 = idx[cur].as<const uint32_t>();
        bool bad = false;
        StagedCols none;
        BG_TRY(gather_frame(c, scols.data(), nc, none, ix, nd, outs, &bad));
        if (bad) return fail(BOWGPU_ERR_HIP, "internal: the merge produced a row index outside the staging frame");
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    if (any_device_out(outs, nc)) device_write_epoch_bump();
    return 0;
}

// rank r's whole part of the call inside one dispatch.  Every rank reaches every barrier, whatever its status: a rank that has failed
// still stands at the barrier behind which nobody reads its buffers
void shard_rank(Worker *w, ShardSort *ss, int r) {
    RankState &me = ss->ranks[r];
    Ctx *c = nullptr;
    auto step = [&](int rc) {
        if (rc != 0 && me.rc == 0) { me.rc = rc; me.err = bowgpu_last_error(); }
        return rc == 0;
    };
    bool ok = step(sharded_enter(w, ss->ids[r], ss->route, &c)) && step(rank_key(c, ss, r));
    ok = ss->barrier.vote(ok);
    if (ok) ok = step(rank_sort(c, ss, r));
    ok = ss->barrier.vote(ok);
    if (ok) {   // the whole frame in order: every rank is, and no rank starts below the end of the one before it (every rank decides alike)
        bool in_order = true, any = false;
        uint64_t last = 0;
        for (int s = 0; s < ss->world; s++) {
            const RankState &q = ss->ranks[s];
            if (q.n == 0) continue;
            in_order &= q.sorted && !(any && q.first_img < last);
            last = q.last_img;
            any = true;
        }
        if (r == 0) ss->unchanged = in_order;
        if (in_order) ok = false;   // (nothing more to do, on any rank)
    }
    if (ok) {
        int rc = 0;
        ok = splitters(c, ss, r, &rc);
        if (rc != 0) step(rc);
    }
    if (ok) ok = step(rank_source(c, ss, r));
    ok = ss->barrier.vote(ok);                       // the pieces are there
    if (ok) ok = step(rank_dest(c, ss, r));
    if (c) (void)hipStreamSynchronize(c->stream);
    (void)ss->barrier.vote(ok);                      // nobody reads this rank's temporaries any more
    me.release();
}

}  // namespace

extern "C" {

int bowgpu_sort_by_col_sharded(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world, int32_t ncols, int32_t key_col,
                               bowgpu_out *const *outs_by_rank, int32_t *unchanged) {
    if (!cols_by_rank || !device_ids || !outs_by_rank || !unchanged) return fail(BOWGPU_ERR_ARG, "null argument");
    *unchanged = 0;   // (1 only where the call has found the frame in order)
    g_info = bowgpu_sort_shard_info();
    if (world <= 0 || world > kShardMaxWorld) return fail(BOWGPU_ERR_ARG, "world %d: 1 .. 64 ranks", world);
    for (int r = 0; r < world; r++) {
        if (!cols_by_rank[r]) return fail(BOWGPU_ERR_ARG, "rank %d: null column array", r);
        if (!outs_by_rank[r]) return fail(BOWGPU_ERR_ARG, "rank %d: null output array", r);
    }
    if (key_col < 0 || key_col > ncols - 1) return fail(BOWGPU_ERR_BAD_COL, "no column '%d'", key_col);
    if (!movable_type(cols_by_rank[0][key_col].type)) return fail(BOWGPU_ERR_TYPE, "column to sort by is of unsupported type (Int64 / Float64 only)");
    // one schema: rank 0's types everywhere; within a rank, columns of one length
    for (int r = 0; r < world; r++) {
        for (int i = 0; i < ncols; i++)
            if (cols_by_rank[r][i].type != cols_by_rank[0][i].type)
                return fail(BOWGPU_ERR_ARG, "rank %d: column %d has type %d, rank 0's has type %d (every rank has the same schema)", r, i,
                            cols_by_rank[r][i].type, cols_by_rank[0][i].type);
        for (int i = 0; i < ncols; i++)
            if (cols_by_rank[r][i].length != cols_by_rank[r][key_col].length)
                return fail(BOWGPU_ERR_ARG, "rank %d: column %d has %lld rows, the column to sort by has %lld", r, i,
                            (long long)cols_by_rank[r][i].length, (long long)cols_by_rank[r][key_col].length);
    }
    for (int r = 0; r < world; r++) BG_TRY(frame_cols_checks(cols_by_rank[r], ncols, cols_by_rank[r][key_col].length, true));
    // the key's nulls where they are known without a device: summed over the ranks, like the rows of one frame
    int64_t nulls = 0;
    bool nulls_known = true;
    for (int r = 0; r < world; r++) {
        const int64_t k = host_count_nulls(&cols_by_rank[r][key_col]);
        if (k < 0) nulls_known = false;
        else nulls += k;
    }
    if (nulls_known && nulls > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %lld nil values", (long long)nulls);
    ShardSort ss;
    ss.T.assign(world + 1, 0);
    for (int r = 0; r < world; r++) {
        const int64_t n = cols_by_rank[r][key_col].length;
        if (n >= kSortMaxRows)
            return fail(BOWGPU_ERR_UNSUPPORTED, "rank %d: column to sort by has %lld rows: the device sort serves fewer than 2^31 = 2147483648 rows a rank",
                        r, (long long)n);
        ss.T[r + 1] = ss.T[r] + n;
    }
    ss.total = ss.T[world];
    for (int r = 0; r < world; r++) {
        const int64_t n = cols_by_rank[r][key_col].length;
        for (int i = 0; i < ncols; i++) {
            const bowgpu_out &u = outs_by_rank[r][i];
            if (!residency_ok(u.residency)) return fail(BOWGPU_ERR_ARG, "rank %d: output %d: unknown residency %d", r, i, u.residency);
            if (u.length < n)
                return fail(BOWGPU_ERR_ARG, "rank %d: output %d has %lld slots, %lld needed", r, i, (long long)u.length, (long long)n);
            if (n > 0 && (!u.values || !u.validity)) return fail(BOWGPU_ERR_ARG, "rank %d: output %d lacks a values or validity buffer", r, i);
        }
    }
    if (ss.total < 2) {   // sort.IsSorted of 0 or 1 rows: the reference returns the receiver
        *unchanged = 1;
        return 0;
    }

    int count = 0;
    if (bowgpu_device_count(&count) != 0 || count <= 0)
        return fail(BOWGPU_ERR_NO_DEVICE, "no HIP device available; the bowgpu path has no CPU fallback");
    for (int r = 0; r < world; r++)
        if (device_ids[r] < 0 || device_ids[r] >= count)
            return fail(BOWGPU_ERR_NO_DEVICE, "rank %d: device %d out of range (%d devices)", r, device_ids[r], count);
    // device-resident buffers of rank r live on device_ids[r]
    for (int r = 0; r < world; r++) {
        auto on_device = [&](const void *p, const char *what, int i) -> int {
            if (!p) return 0;
            int dev = -1;
            BG_TRY(device_of(p, &dev));
            if (dev != device_ids[r])
                return fail(BOWGPU_ERR_ARG, "rank %d: a device-resident buffer of %s %d lives on device %d, not on device_ids[%d] = %d", r, what, i, dev,
                            r, device_ids[r]);
            return 0;
        };
        for (int i = 0; i < ncols; i++) {
            const bowgpu_col &cl = cols_by_rank[r][i];
            if (cl.residency == BOWGPU_DEVICE && cl.length > 0) {
                BG_TRY(on_device(cl.values, "column", i));
                if (cl.null_count != 0) BG_TRY(on_device(cl.validity, "column", i));
            }
            const bowgpu_out &u = outs_by_rank[r][i];
            if (u.residency == BOWGPU_DEVICE && cl.length > 0) {
                BG_TRY(on_device(u.values, "output", i));
                BG_TRY(on_device(u.validity, "output", i));
            }
        }
    }
    {   // the ranks work on streams of their own: what the calling thread's stream still has in flight is done first
        Ctx *c;
        BG_TRY(ctx_get(&c));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    ss.cols_by_rank = cols_by_rank; ss.ids = device_ids; ss.world = world; ss.ncols = ncols; ss.key_col = key_col;
    ss.outs_by_rank = outs_by_rank; ss.route = route_mask();
    ss.ranks.resize(world);
    ss.bounds[0].assign((size_t)world * 2 * kShardMaxWorld, 0);
    ss.bounds[1].assign((size_t)world * 2 * kShardMaxWorld, 0);
    ss.barrier.n = world;
    Fanout *f = sharded_pool();
    {
        std::lock_guard<std::mutex> call_lock(f->call_mu);
        sharded_grow_locked(f, world);
        fan_run(f, world, [&](int r) { shard_rank(f->workers[r], &ss, r); });   // the one dispatch, the one join
    }
    int64_t dev_nulls = 0;
    for (int r = 0; r < world; r++) dev_nulls += ss.ranks[r].nulls;
    if (dev_nulls > 0) return fail(BOWGPU_ERR_SORT_NULLS, "column to sort by has %lld nil values", (long long)dev_nulls);
    for (int r = 0; r < world; r++)
        if (ss.ranks[r].rc != 0) return fail(ss.ranks[r].rc, "%s", ss.ranks[r].err.c_str());
    *unchanged = ss.unchanged ? 1 : 0;
    g_info.splitter_rounds = ss.split_rounds;
    for (int r = 0; r < world; r++) {
        const RankState &q = ss.ranks[r];
        if (q.merge_rounds > g_info.merge_rounds) g_info.merge_rounds = q.merge_rounds;
        if (q.sort_passes > g_info.sort_passes) g_info.sort_passes = q.sort_passes;
        g_info.merged_ranks += q.merge_rounds > 0;
        if (q.sort_ms > g_info.local_sort_ms) g_info.local_sort_ms = q.sort_ms;
        if (q.split_ms > g_info.splitter_ms) g_info.splitter_ms = q.split_ms;
        if (q.merge_ms > g_info.merge_ms) g_info.merge_ms = q.merge_ms;
    }
    return 0;
}

int bowgpu_sort_by_col_sharded_info(bowgpu_sort_shard_info *info) {
    if (!info) return fail(BOWGPU_ERR_ARG, "null argument");
    *info = g_info;
    return 0;
}

}  // extern "C"
