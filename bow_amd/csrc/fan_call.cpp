// fan_call.cpp — ONE Rolling.Aggregate call over SEVERAL devices, inside one process and behind the C ABI (SURVEY.md §8b
// `bowgpu_set_devices`, §8e; reference rolling/aggregation.go:123-145: the user makes one call).
//
// With devices listed (fanout.cpp), bowgpu_rolling_aggregate / _planned / _interpolate_aggregate cut the rows of a call into row
// ranges, one per listed device, and run the shard record protocol of this same library over them (bowgpu_shard_begin -> records ->
// bowgpu_shard_finish: the carry-in stitch in row order) on one persistent host thread per device.  The "exchange" of the protocol is a
// vector in host memory - one process holds every record - so there is no collective, no transport, no torch.  Each rank reduces into
// device temporaries and puts the windows it owns at their places in the CALLER's buffers: values by one copy per output, validity
// bits through a host-side bit placement (fan_host.h: a rank's first window rarely starts on a byte of the frame's bitmap).  The result
// is bit-identical to the one-device call (the protocol's own guarantee, asserted by tests/test_gpu_multi.py against the oracle and
// against the one-device call).
//
// Who is served: host-resident columns and outputs (pageable: each rank stages ITS rows once, over ITS device's PCIe link; registered:
// each device reads its range in place) on any device list; device-resident buffers only when every listed device is the calling
// thread's device (how a one-GPU box exercises the path: the same id listed N times).  Everything the record protocol declines
// (fan_host.h fan_serves; strict_order windows over three ranks) is served by the one-device path as before.  No CPU implementation
// of anything here: the ranks run the HIP kernels.
#include <string.h>

#include <string>

#include "fan_host.h"
#include "fanout.h"

namespace bowgpu {

int current_device_of_thread();   // runtime.cpp: the device the calling thread's context is (or will be) on

int rank_stage(Ctx *c, const StageArgs &a, int64_t row0, int64_t nrows, RankRows *rk) {
    if (rk->staged) return 0;
    std::vector<char> used(a.ncols, a.all_used ? 1 : 0);   // (Interpolate rewrites every column: interpolation.go:139-155)
    used[a.ts_col] = 1;
    for (int i = 0; i < a.naggs; i++) used[a.aggs[i].col] = 1;
    rk->cols.resize(a.ncols);
    rk->staged_bufs.resize((size_t)2 * a.ncols);
    for (int i = 0; i < a.ncols; i++) {
        bowgpu_col &s = rk->cols[i];
        if (used[i] && a.cols[i].residency == BOWGPU_HOST && nrows > 0) {   // (pageable: the device ids are not looked at)
            BG_TRY(stage_rows(c, c->device, c->device, a.cols[i], row0, row0 + nrows, &rk->staged_bufs[2 * i], &rk->staged_bufs[2 * i + 1], &s));
            continue;
        }
        s = a.cols[i];
        s.offset = a.cols[i].offset + row0;
        s.length = nrows;
        s.null_count = has_bitmap(a.cols[i]) ? -1 : 0;
    }
    BG_HIP(hipStreamSynchronize(c->stream));   // (the staging halves are free again; the copies are in HBM)
    rk->staged = true;
    return 0;
}

namespace {

// ---------------------------------------------------------------- one rank of one call
struct Rank : RankRows {
    int64_t row0 = 0, nrows = 0;                      // filled by the calling thread
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
    void release() {   // on the rank's own thread
        release_rows(); out.clear(); mid.clear();
        interpolated = false;
    }
};

struct Call {
    StageArgs in;                        // the caller's columns and aggregators
    int64_t interval; bowgpu_options opts;
    bowgpu_out *outs;
    uint32_t route;
    int world;
    Fanout *f;
    std::vector<std::vector<uint8_t>> frame_tmp;   // per device-resident output: its bitmap while it is assembled on the host
    std::vector<uint8_t *> frame_bits;   // per output: where the frame's bitmap is assembled (the caller's buffer when it lies on the host)
    std::vector<Rank> ranks;
    std::vector<bowgpu_shard_record> records;
    const bowgpu_interp *interps = nullptr;   // Rolling.Interpolate(...).Aggregate(...): one interpolator per column; nullptr: Aggregate alone
    int32_t ninterps = 0;
    int64_t global_s0 = 0;
    void run(const std::function<void(int)> &fn) { fan_run(f, world, fn); }
};

int rank_enter(Worker *w, const Call &call, Ctx **c) {
    if (!w->device_set) {
        BG_TRY(bowgpu_set_device(w->device));
        w->device_set = true;
    }
    BG_TRY(bowgpu_debug_set_route(call.route));
    return ctx_get(c);
}

// Interpolate -> Aggregate, phase 1: the rank's first / last valid point per column (what its neighbours' Linear / StepPrevious need)
void rank_points(Worker *w, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    Ctx *c;
    int rc = rank_enter(w, *call, &c);
    if (rc == 0) rc = rank_stage(c, call->in, rk->row0, rk->nrows, rk);
    if (rc == 0) rc = bowgpu_shard_interp_points(rk->cols.data(), call->in.ncols, call->in.ts_col, &rk->points);
    if (rc != 0) rk->fail_from_thread(rc);
}

// ... phase 2: the rank's interpolated rows into device temporaries (bowgpu_shard_interpolate_count + _fill: concatenated in rank order they
// are the unsharded Interpolate, bit for bit); from here on the rank's columns ARE that frame
int rank_interpolate_impl(Ctx *c, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    const int nc = call->in.ncols, ts = call->in.ts_col;
    int64_t n_out = 0;
    BG_TRY(bowgpu_shard_interpolate_count(rk->cols.data(), nc, ts, call->interval, &call->opts, call->global_s0, rk->interps.data(),
                                          call->ninterps, &rk->edge, &n_out));
    const int64_t cap = (n_out + 31) & ~(int64_t)31;   // (whole bitmap words: the fill writes device bitmaps in place)
    BG_TRY(rk->mid.alloc(c, nc, cap, false));
    if (n_out > 0)
        BG_TRY(bowgpu_shard_interpolate_fill(rk->cols.data(), nc, ts, call->interval, &call->opts, call->global_s0, rk->interps.data(),
                                             call->ninterps, &rk->edge, rk->mid.outs.data()));
    rk->raw_cols = rk->cols;
    rk->mid.as_cols(call->in.cols, n_out, rk->cols.data());
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
    if (rc == 0 && !rk->interpolated) rc = rank_stage(c, call->in, rk->row0, rk->nrows, rk);
    if (rc == 0)
        rc = bowgpu_shard_begin(rk->cols.data(), call->in.ncols, call->in.ts_col, call->interval, &call->opts, call->in.aggs, call->in.naggs,
                                global_s0, &rk->record);
    if (rc != 0) rk->fail_from_thread(rc);
}

// the rank's pass + stitch into device temporaries, then its owned windows into the caller's buffers
int rank_finish_impl(Ctx *c, Call *call, int r) {
    Rank *rk = &call->ranks[r];
    const bowgpu_shard_decision &d = rk->decision;
    const int na = call->in.naggs;
    const int64_t cap = std::max<int64_t>(d.windows_local, 1);
    BG_TRY(rk->out.alloc(c, na, cap, false));
    const int rc = bowgpu_shard_finish(rk->cols.data(), call->in.ncols, call->in.ts_col, call->interval, &call->opts, call->in.aggs, na,
                                       rk->out.outs.data(), call->records.data(), call->world, r, &rk->decision, &rk->info);
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
        rk->host_bits[i].assign(((size_t)(owned + 7) >> 3) + 24, 0);   // (+ 24: place_bits reads 16 bytes past the position it addresses)
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

// every early return of a call: each rank settles its stream and gives its blocks back, on its own thread
struct CleanupGuard {
    Call *call;
    ~CleanupGuard() { if (call) call->run([this](int r) { rank_cleanup(call->f->workers[r], call, r); }); }
};

// ---------------------------------------------------------------- the steps of one call, on the calling thread
// the first rank that failed: its error as the call's; a decline (*declined, 0 returned) sends the call to the one-device path
int first_error(const Call &call, bool *declined) {
    for (const Rank &rk : call.ranks)
        if (rk.rc < 0) {
            if (rk.rc == BOWGPU_ERR_UNSUPPORTED || rk.rc == BOWGPU_ERR_TS_NULLS) { *declined = true; return 0; }
            return fail(rk.rc, "%s", rk.err.c_str());
        }
    return 0;
}

// The checks that fail the call, and the one gate that needs the runtime: device-resident buffers belong to ONE device - only a list
// that names the calling thread's device throughout can share them (*served = false otherwise)
int check_buffers(const StageArgs &in, const bowgpu_out *outs, int64_t W, const std::vector<int> &ids, bool *served) {
    *served = false;
    bool any_device = false;
    for (int i = 0; i < in.ncols; i++) any_device |= in.cols[i].residency == BOWGPU_DEVICE;
    for (int i = 0; i < in.naggs; i++) {
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
    *served = true;
    return 0;
}

// the ranks' row ranges, and where the frame's bitmaps are assembled
void call_layout(Call *call, int64_t n, int64_t W) {
    const int world = call->world, na = call->in.naggs;
    call->ranks.resize(world);
    call->records.resize(world);
    std::vector<int64_t> row0(world), nrows(world);
    fan_row_ranges(n, world, row0.data(), nrows.data());
    for (int r = 0; r < world; r++) { call->ranks[r].row0 = row0[r]; call->ranks[r].nrows = nrows[r]; }
    call->frame_tmp.resize(na);
    call->frame_bits.resize(na);
    for (int i = 0; i < na; i++) {
        if (call->outs[i].residency == BOWGPU_DEVICE) { call->frame_tmp[i].assign((size_t)((W + 7) >> 3), 0); call->frame_bits[i] = call->frame_tmp[i].data(); }
        else call->frame_bits[i] = call->outs[i].validity;
    }
}

// Interpolate -> Aggregate: every rank's points, the edges of each from all of them (host arithmetic: the "exchange"), its interpolated rows
int interpolate_phase(Call *call, bool *declined) {
    const int world = call->world;
    call->run([&](int r) { call->ranks[r].rc = 0; rank_points(call->f->workers[r], call, r); });
    const int rc = first_error(*call, declined);
    if (rc != 0 || *declined) return rc;
    std::vector<bowgpu_interp_points> points(world);
    for (int r = 0; r < world; r++) points[r] = call->ranks[r].points;
    for (int r = 0; r < world; r++)
        interp_edges(points.data(), world, call->in.ncols, call->interps, call->ninterps, r, &call->ranks[r].edge, &call->ranks[r].interps);
    call->run([&](int r) { rank_interpolate(call->f->workers[r], call, r); });
    return first_error(*call, declined);
}

// The record protocol, twice at the most: begin -> records -> every rank's decision -> finish.  *declined (0 returned): a rank declined,
// or an interpolated frame's windows are not the input's - the one-device path words whatever there is to say
int protocol(Call *call, const Plan &plan, bool *declined) {
    const int world = call->world;
    int64_t s0_known = 0;
    const int64_t *s0_ptr = nullptr;
    for (int attempt = 0; attempt < 2; attempt++) {
        call->run([&](int r) { call->ranks[r].rc = 0; rank_begin(call->f->workers[r], call, r, s0_ptr); });
        int rc = first_error(*call, declined);
        if (rc != 0 || *declined) return rc;
        for (int r = 0; r < world; r++) call->records[r] = call->ranks[r].record;
        // every rank's decision from the same records (host arithmetic)
        for (int r = 0; r < world; r++)
            BG_TRY(bowgpu_shard_plan(call->records.data(), world, r, call->interval, call->opts.offset, &call->ranks[r].decision));
        const bowgpu_shard_decision &d0 = call->ranks[0].decision;
        if (!d0.retry_with_s0 && (d0.s0 != plan.s0 || d0.num_windows != plan.W)) {
            if (call->interps) { *declined = true; return 0; }
            return fail(BOWGPU_ERR_ARG, "the plan was not made for this interval column (its first / last timestamp differ)");
        }
        call->run([&](int r) { rank_finish(call->f->workers[r], call, r); });
        rc = first_error(*call, declined);
        if (rc != 0 || *declined) return rc;
        bool retry = false;
        for (int r = 0; r < world; r++) retry |= call->ranks[r].rc == BOWGPU_SHARD_RETRY;
        if (!retry) break;
        if (attempt == 1) return fail(BOWGPU_ERR_ARG, "the shard protocol did not settle after the second exchange");
        s0_known = call->ranks[0].decision.s0;   // rows below the first window start split across ranks (rolling.go:96-99): once more, s0 known
        s0_ptr = &s0_known;
    }
    return 0;
}

// the frame's bitmaps from the ranks' parts (the bytes ranks share, padding bits), counts, types; device-resident bitmaps to their place
int assemble(Call *call, int64_t W) {
    const int world = call->world, na = call->in.naggs;
    bowgpu_out *outs = call->outs;
    int64_t frame_bytes = 0;
    std::vector<const std::vector<EdgeByte> *> edges(world);
    for (int i = 0; i < na; i++) {
        for (int r = 0; r < world; r++) edges[r] = &call->ranks[r].edges[i];
        frame_bytes = frame_bits_finish(call->frame_bits[i], W, edges.data(), world);
        int64_t valid = 0;
        for (int r = 0; r < world; r++) valid += call->ranks[r].valid[i];
        outs[i].length = W;
        outs[i].null_count = W - valid;
        for (int r = 0; r < world; r++)   // (the types were resolved by every rank alike)
            if (!call->ranks[r].out.outs.empty()) { outs[i].type = call->ranks[r].out.outs[i].type; break; }
    }
    bool any_dev_out = false;
    for (int i = 0; i < na; i++) any_dev_out |= outs[i].residency == BOWGPU_DEVICE;
    if (any_dev_out) {
        Ctx *c;
        BG_TRY(ctx_get(&c));
        for (int i = 0; i < na; i++)
            if (outs[i].residency == BOWGPU_DEVICE) BG_TRY(copy_h2d(c, outs[i].validity, call->frame_tmp[i].data(), (size_t)frame_bytes));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// One fanned-out call.  *done = false (and 0 returned): the call is not one for the fan-out - the caller goes on with the one-device
// path.  plan: the frame's (newIntervalRolling's s0 / numWindows), against which the ranks' decisions are checked.  interps != nullptr:
// Rolling.Interpolate(interps...).Aggregate(aggs...) - every rank interpolates its rows first (its neighbours' edge points reach it
// through the same host-memory exchange), then the ranks aggregate their interpolated rows like any other frame.
int fan_call(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
             const bowgpu_interp *interps, int32_t ninterps, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
             bowgpu_agg_info *info, bool *done) {
    *done = false;
    FanSession fan;
    if (fan.ids.size() < 2) return 0;
    const int64_t n = cols[ts_col].length, W = plan.W;
    if (n <= 0 || W <= 0) return 0;
    const int world = fan_world(fan.ids.size(), n, fan.min_rows);
    if (world < 2) return 0;
    if (!fan_serves(cols, ncols, ts_col, aggs, naggs, interps, ninterps, plan.first_ts, plan.s0)) return 0;
    Call call;
    call.in = StageArgs{cols, ncols, ts_col, aggs, naggs, interps != nullptr};
    bool served = false;
    BG_TRY(check_buffers(call.in, outs, W, fan.ids, &served));
    if (!served) return 0;
    fan.start();

    call.interval = plan.interval;
    call.opts.offset = plan.offset; call.opts.inclusive = opt_inclusive ? 1 : 0; call.opts.strict_order = strict ? 1 : 0;
    call.outs = outs; call.route = route_mask(); call.world = world; call.f = fan.f;
    call.interps = interps; call.ninterps = ninterps; call.global_s0 = plan.s0;
    call_layout(&call, n, W);

    CleanupGuard guard{&call};
    bool declined = false;
    if (interps) {
        BG_TRY(interpolate_phase(&call, &declined));
        if (declined) return 0;
    }
    BG_TRY(protocol(&call, plan, &declined));
    if (declined) return 0;
    std::vector<bowgpu_agg_info> infos(world);
    std::vector<int64_t> owned(world);
    for (int r = 0; r < world; r++) { infos[r] = call.ranks[r].info; owned[r] = call.ranks[r].decision.windows_owned; }
    bowgpu_agg_info merged;
    int64_t owned_total = 0;
    if (merge_rank_infos(infos.data(), owned.data(), world, plan.s0, W, &merged, &owned_total) != 0)
        return fail(BOWGPU_ERR_ARG, "internal: the ranks own %lld of %lld windows", (long long)owned_total, (long long)W);
    guard.call = nullptr;   // (every rank has released in its finish)
    BG_TRY(assemble(&call, W));
    if (info) *info = merged;
    fan.served(world);
    *done = true;
    return 0;
}

}  // namespace

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
