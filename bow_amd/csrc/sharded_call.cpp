// sharded_call.cpp — bowgpu_rolling_aggregate_sharded: ONE Rolling.Aggregate call over the frame the CALLER already holds as row
// ranges, one per device (the pool of fanout.cpp's sharded_pool, not the fan-out's).  Each rank runs its whole part inside ONE dispatch -
// record, pass in flight, record published, a barrier among the workers, finish straight into the caller's buffers of that rank, the
// tail of a window it does not own (shard.hip shard_tail_kernel) - and the calling thread joins once.  No device temporaries for the
// outputs, no bitmaps through the host.
#include <string.h>

#include <string>

#include "fan_host.h"
#include "fanout.h"

namespace bowgpu {
namespace {

struct ShardedCall {
    const bowgpu_col *const *cols_by_rank;
    const int32_t *ids;
    int world;
    int32_t ncols, ts_col;
    int64_t interval;
    bowgpu_options opts;
    const bowgpu_agg *aggs;
    int32_t naggs;
    bowgpu_out *const *outs_by_rank;
    uint32_t route;
    std::vector<RankRows> ranks;                   // rank r's columns as the protocol sees them, with their staged copies
    std::vector<bowgpu_shard_record> records[2];   // the exchange: first round, second round (rows below s0 split across ranks)
    std::vector<bowgpu_shard_decision> decisions;
    std::vector<bowgpu_agg_info> infos;
    Barrier barrier;
    std::mutex err_mu;
    int rc = 0;
    std::string err;
    void fail_rank(int code) {   // on the failing worker: its thread-local message
        {
            std::lock_guard<std::mutex> g(err_mu);
            if (rc == 0) { rc = code; err = bowgpu_last_error(); }
        }
        barrier.abort();
    }
};

// a rank that wrote a window it does not own (drops_last): the slot out of its outputs.  Device-resident outputs: shard_tail_kernel and
// the one synchronisation of the rank's stream it needs anyway; host-resident ones are on the host already (the finish has synchronised)
int sharded_tail(Ctx *c, ShardedCall *sc, int r, const bowgpu_shard_decision &d) {
    bowgpu_out *outs = sc->outs_by_rank[r];
    const int na = sc->naggs;
    if (!d.drops_last || d.windows_local <= 0) return 0;
    const int64_t s = d.windows_owned;   // = windows_local - 1: the last slot written
    uint8_t was_valid[BOWGPU_CARRY_MAX_AGGS] = {};
    ShardTailArgs a;
    memset(&a, 0, sizeof a);
    int dev[BOWGPU_CARRY_MAX_AGGS];
    for (int i = 0; i < na; i++) {
        if (outs[i].residency == BOWGPU_DEVICE) {
            a.values[a.n] = reinterpret_cast<uint64_t *>(outs[i].values);
            a.validity[a.n] = outs[i].validity;
            dev[a.n++] = i;
        } else {
            uint8_t *bp = outs[i].validity + (s >> 3);
            const int k = (int)(s & 7);
            was_valid[i] = (uint8_t)((*bp >> k) & 1u);
            *bp = (uint8_t)(*bp & ((1u << k) - 1u));
            reinterpret_cast<uint64_t *>(outs[i].values)[s] = 0;
        }
    }
    if (a.n > 0) {
        BG_TRY(registered_at(c, kRegTailReport, &a.report));
        a.slot = s;
        BG_TRY(launch_shard_tail(c, a));
        BG_HIP(hipStreamSynchronize(c->stream));
        for (int k = 0; k < a.n; k++) was_valid[dev[k]] = a.report[k];
    }
    for (int i = 0; i < na; i++) {
        outs[i].length = s;
        if (!kind_never_nil(sc->aggs[i].kind) && !was_valid[i]) outs[i].null_count -= 1;
    }
    return 0;
}

// rank r's whole part of the call, inside ONE dispatch: begin + pass in flight -> record published -> barrier -> finish (-> the
// second round of the rows-below-s0 corner: begin, barrier, finish) -> tail.  1: another rank failed (nothing of this rank's to report)
int sharded_rank_impl(Worker *w, ShardedCall *sc, int r, Ctx **cp) {
    BG_TRY(sharded_enter(w, sc->ids[r], sc->route, cp));
    Ctx *c = *cp;
    const bowgpu_col *given = sc->cols_by_rank[r];
    RankRows *rk = &sc->ranks[r];
    const int32_t nc = sc->ncols, ts = sc->ts_col, na = sc->naggs;
    bool pageable = false;
    for (int i = 0; i < nc; i++) pageable |= given[i].residency == BOWGPU_HOST;
    if (pageable) {
        BG_TRY(rank_stage(c, StageArgs{given, nc, ts, sc->aggs, na, false}, 0, given[ts].length, rk));
    } else {   // (nothing to stage: the rank's columns as given, without rank_stage's synchronisation)
        rk->cols.assign(given, given + nc);
    }
    int64_t nulls = 0;
    BG_TRY(ts_null_rows(c, &rk->cols[ts], &nulls));
    if (nulls > 0)
        return fail(BOWGPU_ERR_TS_NULLS, "rank %d: interval column has %lld nulls: the sharded call does not serve them", r, (long long)nulls);
    const bowgpu_col *cols = rk->cols.data();
    bowgpu_out *outs = sc->outs_by_rank[r];
    bowgpu_shard_record rec;
    BG_TRY(bowgpu_shard_begin(cols, nc, ts, sc->interval, &sc->opts, sc->aggs, na, nullptr, &rec));
    const int p = bowgpu_shard_pass_begin(cols, nc, ts, sc->interval, &sc->opts, sc->aggs, na, outs, &rec);
    if (p < 0) return p;
    sc->records[0][r] = rec;
    if (!sc->barrier.wait()) return 1;
    for (int round = 0; round < 2; round++) {
        const bowgpu_shard_record *recs = sc->records[round].data();
        bowgpu_shard_decision d;
        BG_TRY(bowgpu_shard_plan(recs, sc->world, r, sc->interval, sc->opts.offset, &d));
        if (!d.retry_with_s0)
            for (int i = 0; i < na; i++)
                if (outs[i].length < d.windows_local)
                    return fail(BOWGPU_ERR_ARG, "rank %d: output %d has %lld slots, %lld needed", r, i, (long long)outs[i].length,
                                (long long)d.windows_local);
        bowgpu_agg_info info;
        const int f = bowgpu_shard_finish(cols, nc, ts, sc->interval, &sc->opts, sc->aggs, na, outs, recs, sc->world, r, &d, &info);
        if (f < 0) return f;
        if (f == 0) {
            // a first window spread over three or more ranks is stitched from the middle ranks' merged partial states
            // (bowgpu_carry_merge: not the reference's row order) - an order-free window, and counted as one where this rank owns it
            if (d.seed_first_rank >= 0 && d.lead_empty_windows < d.windows_owned) {
                int with_rows = 0;
                for (int q = d.seed_first_rank; q < r; q++) with_rows += recs[q].nrows > 0;
                if (with_rows > 1) info.long_windows += 1;
            }
            sc->decisions[r] = d;
            sc->infos[r] = info;
            return sharded_tail(c, sc, r, d);
        }
        if (round == 1) return fail(BOWGPU_ERR_ARG, "internal: the shard protocol did not settle after the second exchange");
        const int64_t s0 = d.s0;   // rows below the first window start split across ranks (rolling.go:96-99): once more, s0 known
        BG_TRY(bowgpu_shard_begin(cols, nc, ts, sc->interval, &sc->opts, sc->aggs, na, &s0, &rec));
        sc->records[1][r] = rec;
        if (!sc->barrier.wait()) return 1;
    }
    return 0;
}

void sharded_rank(Worker *w, ShardedCall *sc, int r) {
    Ctx *c = nullptr;
    const int rc = sharded_rank_impl(w, sc, r, &c);
    if (rc < 0) sc->fail_rank(rc);
    if (c) {
        // (ctx_get outside the protocol's own calls settles a pass still in flight; then nothing of this rank runs any more)
        Ctx *cc;
        if (ctx_get(&cc) == 0) (void)hipStreamSynchronize(cc->stream);
    }
    sc->ranks[r].release_rows();
}

// the layout query of a device-resident interval column: its row count and first / last timestamp, read on the rank's device
void sharded_layout_rank(Worker *w, ShardedCall *sc, int r) {
    const bowgpu_col &t = sc->cols_by_rank[r][sc->ts_col];
    bowgpu_shard_record &rec = sc->records[0][r];
    Ctx *c;
    int rc = sharded_enter(w, sc->ids[r], sc->route, &c);
    int64_t nulls = 0;
    if (rc == 0) rc = ts_null_rows(c, &t, &nulls);
    if (rc == 0 && nulls > 0)
        rc = fail(BOWGPU_ERR_TS_NULLS, "rank %d: interval column has %lld nulls: the sharded call does not serve them", r, (long long)nulls);
    bowgpu_plan p;
    if (rc == 0) rc = bowgpu_plan_windows_ex(&t, sc->interval, sc->opts.offset, &p);
    if (rc == 0) { rec.first_ts = p.first_ts; rec.last_ts = p.last_ts; }
    if (rc < 0) sc->fail_rank(rc);
}

// ---------------------------------------------------------------- the entry point's steps, on the calling thread
int sharded_check_args(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world, int32_t ncols, int32_t ts_col,
                       int64_t interval, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *const *outs_by_rank,
                       const bowgpu_shard_decision *decisions) {
    if (!cols_by_rank || !device_ids || !decisions || !aggs) return fail(BOWGPU_ERR_ARG, "null argument");
    if (world <= 0 || world > 64) return fail(BOWGPU_ERR_ARG, "world %d: 1 .. 64 ranks", world);
    if (ncols <= 0) return fail(BOWGPU_ERR_ARG, "no columns");
    for (int r = 0; r < world; r++) {
        if (!cols_by_rank[r]) return fail(BOWGPU_ERR_ARG, "rank %d: null column array", r);
        if (outs_by_rank && !outs_by_rank[r]) return fail(BOWGPU_ERR_ARG, "rank %d: null output array", r);
    }
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    // one schema: rank 0's types everywhere; within a rank, columns of one length
    for (int r = 0; r < world; r++)
        for (int i = 0; i < ncols; i++) {
            if (cols_by_rank[r][i].type != cols_by_rank[0][i].type)
                return fail(BOWGPU_ERR_ARG, "rank %d: column %d has type %d, rank 0's has type %d (every rank has the same schema)", r, i,
                            cols_by_rank[r][i].type, cols_by_rank[0][i].type);
            if (cols_by_rank[r][i].length != cols_by_rank[r][ts_col].length)
                return fail(BOWGPU_ERR_ARG, "rank %d: column %d has %lld rows, interval column has %lld", r, i, (long long)cols_by_rank[r][i].length,
                            (long long)cols_by_rank[r][ts_col].length);
        }
    return sharded_validate(cols_by_rank[0], ncols, ts_col, interval, aggs, naggs);
}

// the device ids of the ranks (only_device_ts: of those whose interval column the layout query reads on the device)
int sharded_check_ids(const ShardedCall &sc, bool only_device_ts) {
    int count = 0;
    if (bowgpu_device_count(&count) != 0 || count <= 0)
        return fail(BOWGPU_ERR_NO_DEVICE, "no HIP device available; the bowgpu path has no CPU fallback");
    for (int r = 0; r < sc.world; r++) {
        const bowgpu_col &t = sc.cols_by_rank[r][sc.ts_col];
        if (only_device_ts && !(t.residency == BOWGPU_DEVICE && t.length > 0)) continue;
        if (sc.ids[r] < 0 || sc.ids[r] >= count)
            return fail(BOWGPU_ERR_NO_DEVICE, "rank %d: device %d out of range (%d devices)", r, sc.ids[r], count);
    }
    return 0;
}

// the ranks work on streams of their own: what the calling thread's stream still has in flight is done first
int settle_callers_stream() {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// the layout query: each rank's row count and first / last timestamp, then the plan every rank of the full call makes
int sharded_layout(ShardedCall *sc, bowgpu_shard_decision *decisions) {
    const int world = sc->world;
    bool any_device = false;
    for (int r = 0; r < world; r++) {
        const bowgpu_col &t = sc->cols_by_rank[r][sc->ts_col];
        bowgpu_shard_record &rec = sc->records[0][r];
        rec.nrows = t.length;
        rec.naggs = sc->naggs;
        rec.flags = 1;   // (decided with s0 known: what the full call's records say once the protocol has settled)
        if (t.length <= 0) continue;
        if (t.residency == BOWGPU_DEVICE) { any_device = true; continue; }
        const int64_t nulls = host_count_nulls(&t);
        if (nulls > 0)
            return fail(BOWGPU_ERR_TS_NULLS, "rank %d: interval column has %lld nulls: the sharded call does not serve them", r, (long long)nulls);
        const int64_t *v = reinterpret_cast<const int64_t *>(t.values) + t.offset;
        rec.first_ts = v[0];
        rec.last_ts = v[t.length - 1];
    }
    if (any_device) {
        BG_TRY(sharded_check_ids(*sc, true));
        BG_TRY(settle_callers_stream());
        Fanout *f = sharded_pool();
        std::lock_guard<std::mutex> call_lock(f->call_mu);
        sharded_grow_locked(f, world);
        fan_run(f, world, [&](int r) {
            const bowgpu_col &t = sc->cols_by_rank[r][sc->ts_col];
            if (t.residency == BOWGPU_DEVICE && t.length > 0) sharded_layout_rank(f->workers[r], sc, r);
        });
        if (sc->rc < 0) return fail(sc->rc, "%s", sc->err.c_str());
    }
    for (int r = 0; r < world; r++) BG_TRY(bowgpu_shard_plan(sc->records[0].data(), world, r, sc->interval, sc->opts.offset, &decisions[r]));
    return 0;
}

// device-resident buffers of rank r live on device_ids[r]; every output has its two buffers
int sharded_check_buffers(const ShardedCall &sc, int r) {
    auto on_device = [&](const void *p, const char *what, int i) -> int {
        if (!p) return 0;
        int dev = -1;
        BG_TRY(device_of(p, &dev));
        if (dev != sc.ids[r])
            return fail(BOWGPU_ERR_ARG, "rank %d: a device-resident buffer of %s %d lives on device %d, not on device_ids[%d] = %d", r, what, i, dev,
                        r, sc.ids[r]);
        return 0;
    };
    for (int i = 0; i < sc.ncols; i++) {
        const bowgpu_col &cl = sc.cols_by_rank[r][i];
        if (cl.residency != BOWGPU_DEVICE || cl.length <= 0) continue;
        BG_TRY(on_device(cl.values, "column", i));
        if (cl.null_count != 0) BG_TRY(on_device(cl.validity, "column", i));
    }
    for (int i = 0; i < sc.naggs; i++) {
        const bowgpu_out &u = sc.outs_by_rank[r][i];
        if (!u.values || !u.validity) return fail(BOWGPU_ERR_ARG, "rank %d: output %d lacks a values or validity buffer", r, i);
        if (u.residency != BOWGPU_DEVICE) continue;
        BG_TRY(on_device(u.values, "output", i));
        BG_TRY(on_device(u.validity, "output", i));
    }
    return 0;
}

int sharded_full(ShardedCall *sc, bowgpu_shard_decision *decisions, bowgpu_agg_info *info) {
    const int world = sc->world;
    BG_TRY(sharded_check_ids(*sc, false));
    for (int r = 0; r < world; r++) BG_TRY(sharded_check_buffers(*sc, r));
    BG_TRY(settle_callers_stream());
    sc->ranks.resize(world);
    Fanout *f = sharded_pool();
    {
        std::lock_guard<std::mutex> call_lock(f->call_mu);
        sharded_grow_locked(f, world);
        fan_run(f, world, [&](int r) { sharded_rank(f->workers[r], sc, r); });   // the one dispatch, the one join
    }
    if (sc->rc < 0) return fail(sc->rc, "%s", sc->err.c_str());
    const int64_t W = sc->decisions[0].num_windows;
    std::vector<int64_t> owned(world);
    for (int r = 0; r < world; r++) owned[r] = sc->decisions[r].windows_owned;
    int64_t owned_total = 0;
    bowgpu_agg_info merged;
    if (merge_rank_infos(sc->infos.data(), owned.data(), world, sc->decisions[0].s0, W, &merged, &owned_total) != 0)
        return fail(BOWGPU_ERR_ARG, "internal: the ranks own %lld of %lld windows", (long long)owned_total, (long long)W);
    for (int r = 0; r < world; r++) decisions[r] = sc->decisions[r];
    if (info) *info = merged;
    return 0;
}

}  // namespace
}  // namespace bowgpu

using namespace bowgpu;

extern "C" int bowgpu_rolling_aggregate_sharded(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world, int32_t ncols,
                                                int32_t ts_col, int64_t interval, const bowgpu_options *opts, const bowgpu_agg *aggs,
                                                int32_t naggs, bowgpu_out *const *outs_by_rank, bowgpu_shard_decision *decisions,
                                                bowgpu_agg_info *info) {
    BG_TRY(sharded_check_args(cols_by_rank, device_ids, world, ncols, ts_col, interval, aggs, naggs, outs_by_rank, decisions));
    ShardedCall sc;
    sc.cols_by_rank = cols_by_rank; sc.ids = device_ids; sc.world = world; sc.ncols = ncols; sc.ts_col = ts_col; sc.interval = interval;
    sc.opts = options_or(opts); sc.aggs = aggs; sc.naggs = naggs; sc.outs_by_rank = outs_by_rank; sc.route = route_mask();
    sc.records[0].assign(world, bowgpu_shard_record());
    sc.records[1].assign(world, bowgpu_shard_record());
    sc.decisions.assign(world, bowgpu_shard_decision());
    sc.infos.assign(world, bowgpu_agg_info());
    sc.barrier.n = world;
    return outs_by_rank ? sharded_full(&sc, decisions, info) : sharded_layout(&sc, decisions);
}
