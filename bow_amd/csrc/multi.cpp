// multi.cpp — ONE Rolling.Aggregate call over SEVERAL devices, inside one process and behind the C ABI (SURVEY.md §8b
// `bowgpu_set_devices`, §8e; reference rolling/aggregation.go:123-145: the user makes one call).
//
// bowgpu_set_devices(ids, n) names the devices; from then on bowgpu_rolling_aggregate / _planned / _interpolate_aggregate cut the
// rows of a call into row ranges, one per listed device, and run the shard record protocol of this same library over them
// (bowgpu_shard_begin -> records -> bowgpu_shard_finish: the carry-in stitch in row order) on one persistent host thread per
// device.  The "exchange" of the protocol is a vector in host memory - one process holds every record - so there is no collective,
// no transport, no torch.  Each rank reduces into device temporaries and puts the windows it owns at their places in the CALLER's
// buffers: values by one copy per output, validity bits through a host-side bit placement (a rank's first window rarely starts on
// a byte of the frame's bitmap).  The result is bit-identical to the one-device call (the protocol's own guarantee, asserted by
// tests/test_gpu_multi.py against the oracle and against the one-device call).
//
// Who is served: host-resident columns and outputs (pageable: each rank stages ITS rows once, over ITS device's PCIe link; registered:
// each device reads its range in place) on any device list; device-resident buffers only when every listed device is the calling
// thread's device (how a one-GPU box exercises the path: the same id listed N times).  Everything the record protocol declines
// (Mode, Boolean value columns, more than 16 aggregators, interval columns with nulls, strict_order windows over three ranks) is served by the one-device
// path as before.  No CPU implementation of anything here: the ranks run the HIP kernels.
//
// bowgpu_rolling_aggregate_sharded (below the fan-out, with a worker pool of its own) serves the frame the CALLER already holds as row
// ranges, one per device: each rank runs its whole part inside ONE dispatch - record, pass in flight, record published, a barrier among
// the workers, finish straight into the caller's buffers of that rank, the tail of a window it does not own (shard.hip
// shard_tail_kernel) - and the calling thread joins once.  No device temporaries for the outputs, no bitmaps through the host.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "fanout.h"

namespace bowgpu {

int current_device_of_thread();   // runtime.cpp: the device the calling thread's context is (or will be) on

namespace {

std::atomic<int64_t> g_calls_listed{0}, g_calls_served{0};   // bowgpu_fanout_counts
thread_local int g_last_ranks = 1;            // ranks that served the calling thread's last Rolling.Aggregate (bowgpu_last_call_ranks)
std::mutex g_cfg_mu;
std::vector<int> g_ids;                      // guarded by g_cfg_mu
int64_t g_min_rows = (int64_t)1 << 20;       // rows per rank below which a call is not cut further
Fanout *g_fan = nullptr;                     // never destroyed (a worker may sit in its condition variable at process exit)

// BOWGPU_DEVICES="0,1,2,3" / BOWGPU_FANOUT_MIN_ROWS=<rows>, read ONCE per process (like BOWGPU_ROUTE): the initial device list of a process
// that never calls bowgpu_set_devices - how an unmodified program (the C++ mirror's replay of the reference's test tables,
// tests/test_gpu_host_mirror.py) runs through the fan-out.  Nothing on the call path reads the environment.
std::once_flag g_env_once;
void env_defaults() {
    std::call_once(g_env_once, [] {
        const char *d = getenv("BOWGPU_DEVICES");
        const char *m = getenv("BOWGPU_FANOUT_MIN_ROWS");
        std::lock_guard<std::mutex> g(g_cfg_mu);
        if (d && *d && g_ids.empty()) {
            std::vector<int> ids;
            for (const char *q = d; *q;) {
                char *end = nullptr;
                const long v = strtol(q, &end, 10);
                if (end == q) break;
                if (v >= 0 && v < 1024) ids.push_back((int)v);
                q = *end == ',' ? end + 1 : end;
                if (*end != ',' ) break;
            }
            if (ids.size() >= 2 && ids.size() <= 64) g_ids = ids;
        }
        if (m && *m) { const long long v = strtoll(m, nullptr, 10); if (v >= 1) g_min_rows = v; }
    });
}

void worker_main(Worker *w) {
    for (;;) {
        std::function<void()> job;
        {
            std::unique_lock<std::mutex> lk(w->mu);
            w->cv.wait(lk, [&] { return w->has_job || w->quit; });
            if (w->quit && !w->has_job) return;
            job = std::move(w->job);
            w->has_job = false;
        }
        job();
    }
}

void fan_stop_locked(Fanout *f) {   // f->call_mu held
    for (Worker *w : f->workers) {
        { std::lock_guard<std::mutex> g(w->mu); w->quit = true; }
        w->cv.notify_one();
        if (w->th.joinable()) w->th.join();   // (the thread's context, block cache and stream are released by its thread-local destructors)
        delete w;
    }
    f->workers.clear();
    f->ids.clear();
}

void fan_start_locked(Fanout *f, const std::vector<int> &ids) {
    for (int id : ids) {
        Worker *w = new Worker();
        w->device = id;
        w->th = std::thread(worker_main, w);
        f->workers.push_back(w);
    }
    f->ids = ids;
}

}  // namespace

// runs fn(rank) on worker `rank` for rank in [0, world) and waits for all of them
void fan_run(Fanout *f, int world, const std::function<void(int)> &fn) {
    { std::lock_guard<std::mutex> g(f->done_mu); f->pending = world; }
    for (int r = 0; r < world; r++) {
        Worker *w = f->workers[r];
        {
            std::lock_guard<std::mutex> g(w->mu);
            w->job = [f, r, &fn] {
                fn(r);
                std::lock_guard<std::mutex> g2(f->done_mu);
                if (--f->pending == 0) f->done_cv.notify_all();
            };
            w->has_job = true;
        }
        w->cv.notify_one();
    }
    std::unique_lock<std::mutex> lk(f->done_mu);
    f->done_cv.wait(lk, [&] { return f->pending == 0; });
}

namespace {

// ---------------------------------------------------------------- bit placement on the host
// A rank's bitmap (slot k at bit k) goes to bits [d0, d0 + nbits) of the frame's bitmap.  Whole bytes in the middle are stored by the
// rank itself; the first and last byte it touches may be shared with its neighbours and are handed to the calling thread as (index,
// mask, value) - applied after every rank is done, so no two threads ever store to one byte.
struct EdgeByte { int64_t idx; uint8_t mask, val; };

inline uint64_t load_bits64(const uint8_t *src, int64_t bit) {   // 64 bits starting at source bit `bit` (src is padded: 16 readable bytes past the end)
    uint64_t lo, hi;
    memcpy(&lo, src + (bit >> 3), 8);
    memcpy(&hi, src + (bit >> 3) + 8, 8);
    const int r = (int)(bit & 7);
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
}

int64_t place_bits(const uint8_t *src, int64_t nbits, uint8_t *dst, int64_t d0, std::vector<EdgeByte> *edges) {
    if (nbits <= 0) return 0;
    int64_t set = 0;
    const int64_t B0 = d0 >> 3, B1 = (d0 + nbits - 1) >> 3;
    auto byte_at = [&](int64_t B, uint8_t *mask) -> uint8_t {   // dest byte B: its bits that belong to this rank, and their values
        const int64_t lo = std::max<int64_t>(B * 8, d0), hi = std::min<int64_t>(B * 8 + 8, d0 + nbits);   // [lo, hi) global bits
        const uint64_t v = load_bits64(src, lo - d0);
        const int cnt = (int)(hi - lo), sh = (int)(lo - B * 8);
        const uint8_t m = (uint8_t)(((1u << cnt) - 1u) << sh);
        *mask = m;
        return (uint8_t)(((uint32_t)(v & ((1u << cnt) - 1u))) << sh);
    };
    uint8_t m, v = byte_at(B0, &m);
    edges->push_back({B0, m, v});
    set += __builtin_popcount(v);
    if (B1 > B0) {
        v = byte_at(B1, &m);
        edges->push_back({B1, m, v});
        set += __builtin_popcount(v);
    }
    int64_t B = B0 + 1;
    for (; B + 8 <= B1; B += 8) {   // eight whole destination bytes per step
        const uint64_t w = load_bits64(src, B * 8 - d0);
        memcpy(dst + B, &w, 8);
        set += __builtin_popcountll(w);
    }
    for (; B < B1; B++) {
        const uint8_t b = (uint8_t)load_bits64(src, B * 8 - d0);
        dst[B] = b;
        set += __builtin_popcount(b);
    }
    return set;
}

// ---------------------------------------------------------------- one rank of one call
struct Rank {
    // filled by the calling thread
    int64_t row0 = 0, nrows = 0;
    // the rank's columns as the record protocol sees them; pageable columns are staged ONCE (the record pass and the rank's pass both
    // read the staged copy: each row crosses the host link once)
    std::vector<bowgpu_col> cols;
    std::vector<DevBuf> staged_bufs;                  // [2 * ncols]: the values and the bits of column i
    bool staged = false;
    DevFrame out;                                     // its outputs: device temporaries
    std::vector<std::vector<uint8_t>> host_bits;     // the rank's bitmaps on the host (padded)
    std::vector<std::vector<EdgeByte>> edges;         // per output
    std::vector<int64_t> valid;                       // per output: valid slots among the owned ones
    bowgpu_shard_record record;
    bowgpu_shard_decision decision;
    bowgpu_agg_info info;
    // Interpolate -> Aggregate: the rank's points, what lies beyond its two ends, its interpolated rows (device temporaries)
    bowgpu_interp_points points;
    bowgpu_interp_edge edge;
    std::vector<bowgpu_interp> interps;
    DevFrame mid;
    std::vector<bowgpu_col> raw_cols;   // the rank's rows as given (cols becomes the interpolated frame once it exists)
    bool interpolated = false;
    int rc = 0;
    std::string err;
    void fail_from_thread(int code) { rc = code; err = bowgpu_last_error(); }
    void release() {   // on the rank's own thread: the blocks go back to THAT thread's (device's) cache
        staged_bufs.clear(); out.clear(); mid.clear();
        staged = false; interpolated = false;
    }
};

struct Call {
    const bowgpu_col *cols; int32_t ncols, ts_col;
    int64_t interval; bowgpu_options opts;
    const bowgpu_agg *aggs; int32_t naggs;
    bowgpu_out *outs;
    uint32_t route;
    int world;
    std::vector<uint8_t *> frame_bits;   // per output: where the frame's bitmap is assembled (the caller's buffer when it lies on the host)
    std::vector<Rank> ranks;
    std::vector<bowgpu_shard_record> records;
    const bowgpu_interp *interps = nullptr;   // Rolling.Interpolate(...).Aggregate(...): one interpolator per column; nullptr: Aggregate alone
    int32_t ninterps = 0;
    int64_t global_s0 = 0;
};

int rank_enter(Worker *w, const Call &call, Ctx **c) {
    if (!w->device_set) {
        BG_TRY(bowgpu_set_device(w->device));
        w->device_set = true;
    }
    BG_TRY(bowgpu_debug_set_route(call.route));
    return ctx_get(c);
}

// stage the rank's rows of every referenced pageable column into HBM (values from an 8-row boundary so that one offset serves values and bits)
int rank_stage(Ctx *c, const Call &call, Rank *rk) {
    if (rk->staged) return 0;
    std::vector<char> used(call.ncols, call.interps ? 1 : 0);   // (Interpolate rewrites every column: interpolation.go:139-155)
    used[call.ts_col] = 1;
    for (int a = 0; a < call.naggs; a++) used[call.aggs[a].col] = 1;
    rk->cols.resize(call.ncols);
    rk->staged_bufs.resize((size_t)2 * call.ncols);
    for (int i = 0; i < call.ncols; i++) {
        bowgpu_col &s = rk->cols[i];
        if (used[i] && call.cols[i].residency == BOWGPU_HOST && rk->nrows > 0) {   // (pageable: the device ids are not looked at)
            BG_TRY(stage_rows(c, c->device, c->device, call.cols[i], rk->row0, rk->row0 + rk->nrows, &rk->staged_bufs[2 * i],
                              &rk->staged_bufs[2 * i + 1], &s));
            continue;
        }
        s = call.cols[i];
        s.offset = call.cols[i].offset + rk->row0;
        s.length = rk->nrows;
        s.null_count = has_bitmap(call.cols[i]) ? -1 : 0;
    }
    BG_HIP(hipStreamSynchronize(c->stream));   // (the staging halves are free again; the copies are in HBM)
    rk->staged = true;
    return 0;
}

// Interpolate -> Aggregate, phase 1: the rank's first / last valid point per column (what its neighbours' Linear / StepPrevious need)
void rank_points(Worker *w, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    Ctx *c;
    int rc = rank_enter(w, *call, &c);
    if (rc == 0) rc = rank_stage(c, *call, rk);
    if (rc == 0) rc = bowgpu_shard_interp_points(rk->cols.data(), call->ncols, call->ts_col, &rk->points);
    if (rc != 0) rk->fail_from_thread(rc);
}

// ... phase 2: the rank's interpolated rows into device temporaries (bowgpu_shard_interpolate_count + _fill: concatenated in rank order they
// are the unsharded Interpolate, bit for bit); from here on the rank's columns ARE that frame
int rank_interpolate_impl(Ctx *c, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    const int nc = call->ncols;
    int64_t n_out = 0;
    BG_TRY(bowgpu_shard_interpolate_count(rk->cols.data(), nc, call->ts_col, call->interval, &call->opts, call->global_s0, rk->interps.data(),
                                          call->ninterps, &rk->edge, &n_out));
    const int64_t cap = (n_out + 31) & ~(int64_t)31;   // (whole bitmap words: the fill writes device bitmaps in place)
    BG_TRY(rk->mid.alloc(c, nc, cap, false));
    if (n_out > 0)
        BG_TRY(bowgpu_shard_interpolate_fill(rk->cols.data(), nc, call->ts_col, call->interval, &call->opts, call->global_s0, rk->interps.data(),
                                             call->ninterps, &rk->edge, rk->mid.outs.data()));
    rk->raw_cols = rk->cols;
    rk->mid.as_cols(call->cols, n_out, rk->cols.data());
    // the staged copies of the input rows have served
    BG_HIP(hipStreamSynchronize(c->stream));
    rk->staged_bufs.clear();
    rk->interpolated = true;
    return 0;
}

void rank_interpolate(Worker *w, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    Ctx *c = nullptr;
    int rc = rank_enter(w, *call, &c);
    if (rc == 0) rc = rank_interpolate_impl(c, call, r);
    if (rc != 0) rk->fail_from_thread(rc);
}

void rank_begin(Worker *w, Call *call, int r, const int64_t *global_s0) {
    Rank *rk = &call->ranks[r];
    Ctx *c;
    int rc = rank_enter(w, *call, &c);
    if (rc == 0 && !rk->interpolated) rc = rank_stage(c, *call, rk);
    if (rc == 0)
        rc = bowgpu_shard_begin(rk->cols.data(), call->ncols, call->ts_col, call->interval, &call->opts, call->aggs, call->naggs, global_s0,
                                &rk->record);
    if (rc != 0) rk->fail_from_thread(rc);
}

// the rank's pass + stitch into device temporaries, then its owned windows into the caller's buffers
int rank_finish_impl(Ctx *c, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    const bowgpu_shard_decision &d = rk->decision;
    const int na = call->naggs;
    const int64_t cap = std::max<int64_t>(d.windows_local, 1);
    BG_TRY(rk->out.alloc(c, na, cap, false));
    const int rc = bowgpu_shard_finish(rk->cols.data(), call->ncols, call->ts_col, call->interval, &call->opts, call->aggs, na, rk->out.outs.data(),
                                       call->records.data(), call->world, r, &rk->decision, &rk->info);
    if (rc != 0) return rc;   // (BOWGPU_SHARD_RETRY included: the calling thread decides)
    const int64_t owned = d.windows_owned, slot0 = d.first_slot_window_id;
    rk->host_bits.assign(na, std::vector<uint8_t>());
    rk->edges.assign(na, std::vector<EdgeByte>());
    rk->valid.assign(na, 0);
    if (owned <= 0) return 0;
    BG_TRY(ctx_get(&c));
    for (int i = 0; i < na; i++) {
        bowgpu_out *u = &call->outs[i];
        char *dst = reinterpret_cast<char *>(u->values) + 8 * slot0;
        if (u->residency == BOWGPU_DEVICE) BG_HIP(hipMemcpyAsync(dst, rk->out.outs[i].values, (size_t)owned * 8, hipMemcpyDeviceToDevice, c->stream));
        else BG_TRY(copy_d2h(c, dst, rk->out.outs[i].values, (size_t)owned * 8, u->residency == BOWGPU_HOST_PINNED));
        rk->host_bits[i].assign(((size_t)(owned + 7) >> 3) + 24, 0);
        BG_TRY(copy_d2h(c, rk->host_bits[i].data(), rk->out.outs[i].validity, (size_t)((owned + 7) >> 3)));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < na; i++)
        rk->valid[i] = place_bits(rk->host_bits[i].data(), owned, call->frame_bits[i], slot0, &rk->edges[i]);
    return 0;
}

void rank_finish(Worker *w, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    Ctx *c = nullptr;
    int rc = rank_enter(w, *call, &c);
    if (rc == 0) rc = rank_finish_impl(c, call, r);
    if (rc < 0) rk->fail_from_thread(rc); else rk->rc = rc;
    if (rc != BOWGPU_SHARD_RETRY) {
        if (c) (void)hipStreamSynchronize(c->stream);
        rk->release();
    }
}

void rank_cleanup(Worker *w, Call *call, int r) {
    Ctx *c;
    if (rank_enter(w, *call, &c) == 0) (void)hipStreamSynchronize(c->stream);
    call->ranks[r].release();
}

bool is_decline(int rc) { return rc == BOWGPU_ERR_UNSUPPORTED || rc == BOWGPU_ERR_TS_NULLS; }

// ---------------------------------------------------------------- bowgpu_rolling_aggregate_sharded: the caller's shards, one dispatch, one join
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
    std::vector<Call> views;                       // rank r's columns as rank_stage sees them (a Call of one rank: rows [0, length))
    std::vector<Rank> ranks;                       // ... and its staged copies
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

}  // namespace

static Fanout *g_sharded = nullptr;   // the workers of bowgpu_rolling_aggregate_sharded (not the fan-out's); never destroyed, like g_fan

Fanout *sharded_pool() {
    std::lock_guard<std::mutex> g(g_cfg_mu);
    if (!g_sharded) g_sharded = new Fanout();
    return g_sharded;
}

void sharded_grow_locked(Fanout *f, int world) {
    while ((int)f->workers.size() < world) {
        Worker *w = new Worker();
        w->device = -1;
        w->th = std::thread(worker_main, w);
        f->workers.push_back(w);
    }
}

int sharded_enter(Worker *w, int device, uint32_t route, Ctx **c) {
    if (!w->device_set || w->device != device) {
        BG_TRY(bowgpu_set_device(device));
        w->device = device;
        w->device_set = true;
    }
    BG_TRY(bowgpu_debug_set_route(route));
    return ctx_get(c);
}

namespace {

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
    Call &view = sc->views[r];
    Rank *rk = &sc->ranks[r];
    const int32_t nc = sc->ncols, ts = sc->ts_col, na = sc->naggs;
    bool pageable = false;
    for (int i = 0; i < nc; i++) pageable |= view.cols[i].residency == BOWGPU_HOST;
    if (pageable) {
        BG_TRY(rank_stage(c, view, rk));
    } else {   // (nothing to stage: the rank's columns as given, without rank_stage's synchronisation)
        rk->cols.assign(view.cols, view.cols + nc);
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
    sc->ranks[r].release();
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

}  // namespace

int device_of(const void *p, int *dev) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); *dev = -1; return 0; }
    *dev = a.device;
    return 0;
}

// One fanned-out call.  *done = false (and 0 returned): the call is not one for the fan-out - the caller goes on with the one-device
// path.  plan: the frame's (newIntervalRolling's s0 / numWindows), against which the ranks' decisions are checked.  interps != nullptr:
// Rolling.Interpolate(interps...).Aggregate(aggs...) - every rank interpolates its rows first (its neighbours' edge points reach it
// through the same host-memory exchange), then the ranks aggregate their interpolated rows like any other frame.
static int fan_call(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
                    const bowgpu_interp *interps, int32_t ninterps, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                    bowgpu_agg_info *info, bool *done) {
    *done = false;
    g_last_ranks = 1;
    env_defaults();
    std::vector<int> ids;
    int64_t min_rows;
    {
        std::lock_guard<std::mutex> g(g_cfg_mu);
        ids = g_ids;
        min_rows = g_min_rows;
    }
    if (ids.size() >= 2) g_calls_listed.fetch_add(1, std::memory_order_relaxed);
    if (ids.size() < 2) return 0;
    const int64_t n = cols[ts_col].length;
    const int64_t W = plan.W;
    if (n <= 0 || W <= 0) return 0;
    int world = (int)std::min<int64_t>((int64_t)ids.size(), n / std::max<int64_t>(min_rows, 1));
    if (world < 2) return 0;
    if (naggs > BOWGPU_CARRY_MAX_AGGS) return 0;
    for (int i = 0; i < naggs; i++) if (aggs[i].kind == BOWGPU_AGG_MODE) return 0;
    for (int i = 0; i < naggs; i++) if (cols[aggs[i].col].type == BOWGPU_BOOLEAN) return 0;   // (Boolean columns: no record for bit ranges, the caller's device serves the call)
    if (cols[ts_col].validity && cols[ts_col].null_count != 0) return 0;   // (nulls in the interval column: the one-device path serves them)
    if (interps) {
        // the sharded Interpolate's own limit (include/bowgpu.h): at most 8 columns (bowgpu_interp_edge).  Rows below the first window start
        // (a negative first timestamp under Go's truncating division) make the interpolated frame start with its synthetic row at s0 and go
        // on BELOW it: what Aggregate then does with that frame is the one-device path's business
        if (ncols > 8 || ninterps != ncols || plan.first_ts < plan.s0) return 0;
        for (int i = 0; i < ncols; i++) if (interps[i].col != i) return 0;
    }
    // device-resident buffers belong to ONE device: only a list that names the calling thread's device throughout can share them
    bool any_device = false;
    for (int i = 0; i < ncols; i++) any_device |= cols[i].residency == BOWGPU_DEVICE;
    for (int i = 0; i < naggs; i++) {
        any_device |= outs[i].residency == BOWGPU_DEVICE;
        if (outs[i].length < W) return fail(BOWGPU_ERR_ARG, "output column has %lld slots, %lld needed", (long long)outs[i].length, (long long)W);
        if (!outs[i].values || !outs[i].validity) return fail(BOWGPU_ERR_ARG, "output column lacks a values or validity buffer");
    }
    if (any_device) {
        const int mine = current_device_of_thread();
        for (int id : ids) if (id != mine) return 0;
        // the ranks work on streams of their own: what the calling thread's stream (bowgpu_set_stream: possibly the application's) still
        // has in flight on these buffers is done first
        Ctx *c;
        BG_TRY(ctx_get(&c));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    Fanout *f;
    {
        std::lock_guard<std::mutex> g(g_cfg_mu);
        if (!g_fan) g_fan = new Fanout();
        f = g_fan;
    }
    std::lock_guard<std::mutex> call_lock(f->call_mu);
    if (f->ids != ids) { fan_stop_locked(f); fan_start_locked(f, ids); }

    Call call;
    call.cols = cols; call.ncols = ncols; call.ts_col = ts_col; call.interval = plan.interval;
    call.opts.offset = plan.offset; call.opts.inclusive = opt_inclusive ? 1 : 0; call.opts.strict_order = strict ? 1 : 0;
    call.aggs = aggs; call.naggs = naggs; call.outs = outs; call.route = route_mask(); call.world = world;
    call.interps = interps; call.ninterps = ninterps; call.global_s0 = plan.s0;
    call.ranks.resize(world);
    call.records.resize(world);
    // row ranges: multiples of 4096 rows (16-byte aligned value pointers, whole bitmap words) except the last one's end
    {
        const int64_t per = ((n / world) + 4095) & ~(int64_t)4095;
        int64_t at = 0;
        for (int r = 0; r < world; r++) {
            const int64_t end = r + 1 == world ? n : std::min<int64_t>(n, at + per);
            call.ranks[r].row0 = at;
            call.ranks[r].nrows = end - at;
            at = end;
        }
    }
    // where the frame's bitmaps are assembled
    std::vector<std::vector<uint8_t>> frame_tmp(naggs);
    const size_t frame_bytes = (size_t)((W + 7) >> 3);
    call.frame_bits.resize(naggs);
    for (int i = 0; i < naggs; i++) {
        if (outs[i].residency == BOWGPU_DEVICE) { frame_tmp[i].assign(frame_bytes, 0); call.frame_bits[i] = frame_tmp[i].data(); }
        else call.frame_bits[i] = outs[i].validity;
    }
    auto first_error = [&](bool *declined) -> int {
        for (int r = 0; r < world; r++)
            if (call.ranks[r].rc < 0) {
                if (is_decline(call.ranks[r].rc)) { *declined = true; return 0; }
                return fail(call.ranks[r].rc, "%s", call.ranks[r].err.c_str());
            }
        return 0;
    };
    auto cleanup = [&] { fan_run(f, world, [&](int r) { rank_cleanup(f->workers[r], &call, r); }); };

    if (interps) {
        fan_run(f, world, [&](int r) { call.ranks[r].rc = 0; rank_points(f->workers[r], &call, r); });
        bool declined = false;
        int rc = first_error(&declined);
        if (rc != 0 || declined) { cleanup(); return rc; }
        // what lies beyond each rank's two ends, from every rank's points (host arithmetic: the "exchange")
        for (int r = 0; r < world; r++) {
            Rank &rk = call.ranks[r];
            memset(&rk.edge, 0, sizeof rk.edge);
            rk.interps.assign(interps, interps + ninterps);
            int left_last = -1;
            for (int q = 0; q < r; q++) if (call.ranks[q].points.nrows > 0) left_last = q;
            if (left_last >= 0) { rk.edge.has_left = 1; rk.edge.left_last_ts = call.ranks[left_last].points.last_ts; }
            for (int i = 0; i < ncols; i++) {
                for (int q = r - 1; q >= 0; q--) {      // nearest valid point on the left: the reference's own PrevRow mechanism carries it (linear.go:14-18)
                    const bowgpu_interp_points &pq = call.ranks[q].points;
                    if (pq.nrows > 0 && pq.last_valid[i]) {
                        bowgpu_interp &ip = rk.interps[i];
                        ip.has_prev_row = 1; ip.prev_t_valid = 1; ip.prev_v_valid = 1;
                        ip.prev_t = pq.last_t[i]; ip.prev_v = pq.last_v[i]; ip.prev_v_i64 = pq.last_v_i64[i];
                        break;
                    }
                }
                for (int q = r + 1; q < world; q++) {   // nearest valid point on the right
                    const bowgpu_interp_points &pq = call.ranks[q].points;
                    if (pq.nrows > 0 && pq.first_valid[i]) {
                        rk.edge.next_valid[i] = 1; rk.edge.next_t[i] = pq.first_t[i]; rk.edge.next_v[i] = pq.first_v[i];
                        break;
                    }
                }
            }
        }
        fan_run(f, world, [&](int r) { rank_interpolate(f->workers[r], &call, r); });
        rc = first_error(&declined);
        if (rc != 0 || declined) { cleanup(); return rc; }
    }

    int64_t s0_known = 0;
    const int64_t *s0_ptr = nullptr;
    for (int attempt = 0; attempt < 2; attempt++) {
        fan_run(f, world, [&](int r) { call.ranks[r].rc = 0; rank_begin(f->workers[r], &call, r, s0_ptr); });
        bool declined = false;
        int rc = first_error(&declined);
        if (rc != 0 || declined) { cleanup(); return rc; }
        for (int r = 0; r < world; r++) call.records[r] = call.ranks[r].record;
        // every rank's decision from the same records (host arithmetic)
        for (int r = 0; r < world; r++) {
            rc = bowgpu_shard_plan(call.records.data(), world, r, call.interval, call.opts.offset, &call.ranks[r].decision);
            if (rc != 0) { cleanup(); return rc; }
        }
        const bowgpu_shard_decision &d0 = call.ranks[0].decision;
        if (!d0.retry_with_s0 && (d0.s0 != plan.s0 || d0.num_windows != W)) {
            cleanup();
            if (interps) return 0;   // (an interpolated frame whose windows are not the input's: the two calls on one device word whatever there is to say)
            return fail(BOWGPU_ERR_ARG, "the plan was not made for this interval column (its first / last timestamp differ)");
        }
        fan_run(f, world, [&](int r) { rank_finish(f->workers[r], &call, r); });
        rc = first_error(&declined);
        if (rc != 0 || declined) { cleanup(); return rc; }
        bool retry = false;
        for (int r = 0; r < world; r++) retry |= call.ranks[r].rc == BOWGPU_SHARD_RETRY;
        if (!retry) break;
        if (attempt == 1) { cleanup(); return fail(BOWGPU_ERR_ARG, "the shard protocol did not settle after the second exchange"); }
        s0_known = call.ranks[0].decision.s0;   // rows below the first window start split across ranks (rolling.go:96-99): once more, s0 known
        s0_ptr = &s0_known;
    }
    // the bytes ranks share, padding bits, counts
    int64_t owned_total = 0;
    for (int r = 0; r < world; r++) owned_total += std::max<int64_t>(call.ranks[r].decision.windows_owned, 0);
    if (owned_total != W) return fail(BOWGPU_ERR_ARG, "internal: the ranks own %lld of %lld windows", (long long)owned_total, (long long)W);
    for (int i = 0; i < naggs; i++) {
        uint8_t *fb = call.frame_bits[i];
        // (edge bytes: first clear every bit some rank owns, then set - a byte may hold the bits of several ranks)
        for (int r = 0; r < world; r++) for (const EdgeByte &e : call.ranks[r].edges[i]) fb[e.idx] &= (uint8_t)~e.mask;
        for (int r = 0; r < world; r++) for (const EdgeByte &e : call.ranks[r].edges[i]) fb[e.idx] |= e.val;
        if (W & 7) fb[frame_bytes - 1] &= (uint8_t)((1u << (W & 7)) - 1u);   // padding bits stay clear (bowbuffer.go:22-40 zero-initialises)
        int64_t valid = 0;
        for (int r = 0; r < world; r++) valid += call.ranks[r].valid[i];
        outs[i].length = W;
        outs[i].null_count = W - valid;
        for (int r = 0; r < world; r++)   // (the types were resolved by every rank alike)
            if (!call.ranks[r].out.outs.empty()) { outs[i].type = call.ranks[r].out.outs[i].type; break; }
    }
    bool any_dev_out = false;
    for (int i = 0; i < naggs; i++) any_dev_out |= outs[i].residency == BOWGPU_DEVICE;
    if (any_dev_out) {
        Ctx *c;
        BG_TRY(ctx_get(&c));
        for (int i = 0; i < naggs; i++)
            if (outs[i].residency == BOWGPU_DEVICE) BG_TRY(copy_h2d(c, outs[i].validity, frame_tmp[i].data(), frame_bytes));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    if (info) {
        const bowgpu_agg_info &i0 = call.ranks[0].info;
        info->s0 = plan.s0; info->num_windows = W; info->new_interval_col = i0.new_interval_col; info->inclusive = i0.inclusive;
        info->long_windows = 0; info->kernel_ms = 0;
        for (int r = 0; r < world; r++) {
            info->long_windows += call.ranks[r].info.long_windows;
            info->kernel_ms = std::max(info->kernel_ms, call.ranks[r].info.kernel_ms);
        }
    }
    g_last_ranks = world;
    g_calls_served.fetch_add(1, std::memory_order_relaxed);
    *done = true;
    return 0;
}

int multi_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
                    const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, bowgpu_agg_info *info, bool *done) {
    return fan_call(cols, ncols, ts_col, plan, opt_inclusive, strict, nullptr, 0, aggs, naggs, outs, info, done);
}

int multi_interpolate_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
                                const bowgpu_interp *interps, int32_t ninterps, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                                bowgpu_agg_info *info, bool *done) {
    return fan_call(cols, ncols, ts_col, plan, opt_inclusive, strict, interps, ninterps, aggs, naggs, outs, info, done);
}

}  // namespace bowgpu

using namespace bowgpu;

extern "C" {

int bowgpu_set_devices(const int *ids, int n) {
    if (n < 0 || (n > 0 && !ids)) return fail(BOWGPU_ERR_ARG, "bowgpu_set_devices: bad arguments");
    env_defaults();   // (so that a later first call does not overwrite what this call sets)
    if (n > 64) return fail(BOWGPU_ERR_ARG, "bowgpu_set_devices: at most 64 ranks");
    int count = 0;
    if (n > 0) {
        BG_TRY(bowgpu_device_count(&count));
        if (count <= 0) return fail(BOWGPU_ERR_NO_DEVICE, "no HIP device available; the bowgpu path has no CPU fallback");
        for (int i = 0; i < n; i++)
            if (ids[i] < 0 || ids[i] >= count) return fail(BOWGPU_ERR_NO_DEVICE, "device %d out of range (%d devices)", ids[i], count);
    }
    std::lock_guard<std::mutex> g(g_cfg_mu);
    g_ids.assign(ids, ids + n);
    return 0;
}

int bowgpu_get_devices(int *ids, int cap, int *n) {
    if (!n) return fail(BOWGPU_ERR_ARG, "null argument");
    env_defaults();
    std::lock_guard<std::mutex> g(g_cfg_mu);
    *n = (int)g_ids.size();
    for (int i = 0; ids && i < cap && i < (int)g_ids.size(); i++) ids[i] = g_ids[i];
    return 0;
}

int bowgpu_last_call_ranks(int *ranks) {
    if (!ranks) return fail(BOWGPU_ERR_ARG, "null argument");
    *ranks = g_last_ranks;
    return 0;
}

int bowgpu_fanout_counts(int64_t *calls, int64_t *served) {
    if (!calls || !served) return fail(BOWGPU_ERR_ARG, "null argument");
    *calls = g_calls_listed.load(std::memory_order_relaxed);
    *served = g_calls_served.load(std::memory_order_relaxed);
    return 0;
}

int bowgpu_rolling_aggregate_sharded(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world, int32_t ncols,
                                     int32_t ts_col, int64_t interval, const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs,
                                     bowgpu_out *const *outs_by_rank, bowgpu_shard_decision *decisions, bowgpu_agg_info *info) {
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
    BG_TRY(sharded_validate(cols_by_rank[0], ncols, ts_col, interval, aggs, naggs));
    const bowgpu_options o = options_or(opts);

    ShardedCall sc;
    sc.cols_by_rank = cols_by_rank; sc.ids = device_ids; sc.world = world; sc.ncols = ncols; sc.ts_col = ts_col; sc.interval = interval;
    sc.opts = o; sc.aggs = aggs; sc.naggs = naggs; sc.outs_by_rank = outs_by_rank; sc.route = route_mask();
    sc.records[0].assign(world, bowgpu_shard_record());
    sc.records[1].assign(world, bowgpu_shard_record());
    sc.decisions.assign(world, bowgpu_shard_decision());
    sc.infos.assign(world, bowgpu_agg_info());
    sc.barrier.n = world;

    auto check_ids = [&](bool only_device_ts) -> int {
        int count = 0;
        if (bowgpu_device_count(&count) != 0 || count <= 0)
            return fail(BOWGPU_ERR_NO_DEVICE, "no HIP device available; the bowgpu path has no CPU fallback");
        for (int r = 0; r < world; r++) {
            if (only_device_ts && !(cols_by_rank[r][ts_col].residency == BOWGPU_DEVICE && cols_by_rank[r][ts_col].length > 0)) continue;
            if (device_ids[r] < 0 || device_ids[r] >= count)
                return fail(BOWGPU_ERR_NO_DEVICE, "rank %d: device %d out of range (%d devices)", r, device_ids[r], count);
        }
        return 0;
    };

    if (!outs_by_rank) {
        // ---- the layout query: each rank's row count and first / last timestamp, then the plan every rank of the full call makes
        bool any_device = false;
        for (int r = 0; r < world; r++) {
            const bowgpu_col &t = cols_by_rank[r][ts_col];
            bowgpu_shard_record &rec = sc.records[0][r];
            rec.nrows = t.length;
            rec.naggs = naggs;
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
            BG_TRY(check_ids(true));
            {   // (the workers read the interval columns on streams of their own: what the calling thread's stream has in flight first)
                Ctx *c;
                BG_TRY(ctx_get(&c));
                BG_HIP(hipStreamSynchronize(c->stream));
            }
            Fanout *f = sharded_pool();
            std::lock_guard<std::mutex> call_lock(f->call_mu);
            sharded_grow_locked(f, world);
            fan_run(f, world, [&](int r) {
                const bowgpu_col &t = cols_by_rank[r][ts_col];
                if (t.residency == BOWGPU_DEVICE && t.length > 0) sharded_layout_rank(f->workers[r], &sc, r);
            });
            if (sc.rc < 0) return fail(sc.rc, "%s", sc.err.c_str());
        }
        for (int r = 0; r < world; r++) BG_TRY(bowgpu_shard_plan(sc.records[0].data(), world, r, interval, o.offset, &decisions[r]));
        return 0;
    }

    // ---- the full call
    BG_TRY(check_ids(false));
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
            if (cl.residency != BOWGPU_DEVICE || cl.length <= 0) continue;
            BG_TRY(on_device(cl.values, "column", i));
            if (cl.null_count != 0) BG_TRY(on_device(cl.validity, "column", i));
        }
        for (int i = 0; i < naggs; i++) {
            const bowgpu_out &u = outs_by_rank[r][i];
            if (!u.values || !u.validity) return fail(BOWGPU_ERR_ARG, "rank %d: output %d lacks a values or validity buffer", r, i);
            if (u.residency != BOWGPU_DEVICE) continue;
            BG_TRY(on_device(u.values, "output", i));
            BG_TRY(on_device(u.validity, "output", i));
        }
    }
    {   // the ranks work on streams of their own: what the calling thread's stream still has in flight is done first
        Ctx *c;
        BG_TRY(ctx_get(&c));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    sc.views.resize(world);
    sc.ranks.resize(world);
    for (int r = 0; r < world; r++) {
        Call &v = sc.views[r];
        v.cols = cols_by_rank[r]; v.ncols = ncols; v.ts_col = ts_col; v.interval = interval; v.opts = o;
        v.aggs = aggs; v.naggs = naggs; v.outs = nullptr; v.route = sc.route; v.world = 1;
        sc.ranks[r].row0 = 0;
        sc.ranks[r].nrows = cols_by_rank[r][ts_col].length;
    }
    Fanout *f = sharded_pool();
    {
        std::lock_guard<std::mutex> call_lock(f->call_mu);
        sharded_grow_locked(f, world);
        fan_run(f, world, [&](int r) { sharded_rank(f->workers[r], &sc, r); });   // the one dispatch, the one join
    }
    if (sc.rc < 0) return fail(sc.rc, "%s", sc.err.c_str());
    const int64_t W = sc.decisions[0].num_windows;
    int64_t owned = 0;
    for (int r = 0; r < world; r++) owned += std::max<int64_t>(sc.decisions[r].windows_owned, 0);
    if (owned != W) return fail(BOWGPU_ERR_ARG, "internal: the ranks own %lld of %lld windows", (long long)owned, (long long)W);
    for (int r = 0; r < world; r++) decisions[r] = sc.decisions[r];
    if (info) {
        const bowgpu_agg_info &i0 = sc.infos[0];
        info->s0 = sc.decisions[0].s0; info->num_windows = W; info->new_interval_col = i0.new_interval_col; info->inclusive = i0.inclusive;
        info->long_windows = 0; info->kernel_ms = 0;
        for (int r = 0; r < world; r++) {
            info->long_windows += sc.infos[r].long_windows;
            info->kernel_ms = std::max(info->kernel_ms, sc.infos[r].kernel_ms);
        }
    }
    return 0;
}

int bowgpu_set_fanout_min_rows(int64_t rows) {
    if (rows < 1) return fail(BOWGPU_ERR_ARG, "bowgpu_set_fanout_min_rows: at least one row per rank");
    env_defaults();
    std::lock_guard<std::mutex> g(g_cfg_mu);
    g_min_rows = rows;
    return 0;
}

}  // extern "C"
