// shard_api.cpp — row-range sharding: the shard protocol, begin -> one exchange -> finish (include/bowgpu.h), and the pass that
// bowgpu_shard_pass_begin leaves in flight on the thread's stream.

#include <string.h>

#include <algorithm>
#include <vector>

#include "agg_host.h"

namespace bowgpu {

// what a window cut by a shard boundary needs on top of validate_aggs: a constant-size running state per reducer (Mode has none)
// and room for it in the record.  Columns and outputs of any residency: host-resident ones are staged through HBM per call the way
// the unsharded entry points stage them (the pass put in flight by _pass_begin keeps its staged copies until _finish collects it)
int shard_check(const bowgpu_col *cols, const bowgpu_agg *aggs, int32_t naggs) {
    for (int i = 0; i < naggs; i++)
        if (aggs[i].kind == BOWGPU_AGG_MODE) return fail(BOWGPU_ERR_UNSUPPORTED, "sharded aggregate: Mode is not a mergeable reducer");
    for (int i = 0; i < naggs; i++)   // (validate_aggs checked aggs[i].col)
        if (cols[aggs[i].col].type == BOWGPU_BOOLEAN)
            return fail(BOWGPU_ERR_UNSUPPORTED, "sharded aggregate: Boolean columns are served by the unsharded call only (the record holds no bit ranges)");
    if (naggs > BOWGPU_CARRY_MAX_AGGS) return fail(BOWGPU_ERR_UNSUPPORTED, "sharded aggregate: too many aggregations");
    return 0;
}

// ---- the pass of a sharded call put in flight BEFORE the exchange (bowgpu_shard_pass_begin): one per thread
struct PendingPass {
    AggJob job;   // (with its copies of the aggregations and of the plan)
    PassState ps;
    std::vector<const void *> col_values, out_values;
    int64_t n = 0, interval = 0, raw_offset = 0, base = 0;
    int32_t ts_col = 0, inclusive = 0;
};
static void pending_pass_delete(void *p) { delete static_cast<PendingPass *>(p); }

}  // namespace bowgpu

using namespace bowgpu;

extern "C" {

int bowgpu_carry_merge(const bowgpu_carry_state *L, const bowgpu_carry_state *R, bowgpu_carry_state *out) {
    // concatenation of two row ranges of one window, left then right (same rules as the device stats_merge)
    if (!L || !R || !out) return fail(BOWGPU_ERR_ARG, "null argument");
    bowgpu_carry_state m = *L;
    m.nrows = L->nrows + R->nrows;
    if (R->has_value) {
        if (!L->has_value) {
            const int64_t nrows = m.nrows;
            m = *R;
            m.nrows = nrows;
        } else {
            m.sum = L->sum + R->sum;
            m.count = L->count + R->count;
            if (R->has_nn) {
                if (R->nn_min < m.vmin) m.vmin = R->nn_min;
                if (R->nn_max > m.vmax) m.vmax = R->nn_max;
                if (!m.has_nn) { m.nn_min = R->nn_min; m.nn_max = R->nn_max; m.has_nn = 1; }
                else { if (R->nn_min < m.nn_min) m.nn_min = R->nn_min; if (R->nn_max > m.nn_max) m.nn_max = R->nn_max; }
            }
            m.last_bits = R->last_bits;
        }
    }
    // the both-valid points of the time-weighted reducers (device stats_merge)
    m.pt = L->pt; m.pv = L->pv; m.first_pt = L->first_pt; m.first_pv = L->first_pv;
    m.integ_step = L->integ_step; m.integ_trap = L->integ_trap; m.has_point = L->has_point; m.has_pair = L->has_pair;
    if (R->has_point) {
        if (L->has_point) {
            m.integ_trap = L->integ_trap + (L->pv + R->first_pv) / 2 * (R->first_pt - L->pt) + R->integ_trap;
            m.integ_step = L->integ_step + L->pv * (R->first_pt - L->pt) + R->integ_step;
            m.has_pair = 1;
        } else {
            m.first_pt = R->first_pt; m.first_pv = R->first_pv; m.integ_trap = R->integ_trap; m.integ_step = R->integ_step;
            m.has_pair = R->has_pair; m.has_point = 1;
        }
        m.pt = R->pt; m.pv = R->pv;
    }
    *out = m;
    return 0;
}

// the rank's first row as the rank to its left needs it for an inclusive window (bowgpu_shard_record.first_row)
static int shard_first_row(const bowgpu_col *cols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs, bowgpu_next_row *out) {
    memset(out, 0, sizeof *out);
    if (cols[ts_col].length == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    auto fetch = [&](const bowgpu_col &col, uint64_t *bits, int32_t *valid) -> int {
        if (col.residency != BOWGPU_DEVICE) {   // host memory (pageable or registered): read where it lies
            memcpy(bits, reinterpret_cast<const char *>(col.values) + 8 * col.offset, 8);
            *valid = (col.validity && col.null_count != 0) ? ((col.validity[col.offset >> 3] >> (col.offset & 7)) & 1) : 1;
            return 0;
        }
        BG_HIP(hipMemcpyAsync(bits, reinterpret_cast<const char *>(col.values) + 8 * col.offset, 8, hipMemcpyDeviceToHost, c->stream));
        *valid = 1;
        if (col.validity && col.null_count != 0) {
            uint8_t byte = 0;
            BG_HIP(hipMemcpyAsync(&byte, col.validity + (col.offset >> 3), 1, hipMemcpyDeviceToHost, c->stream));
            BG_HIP(hipStreamSynchronize(c->stream));
            *valid = (byte >> (col.offset & 7)) & 1;
        }
        return 0;
    };
    uint64_t tsb = 0;
    int32_t tv = 0;
    BG_TRY(fetch(cols[ts_col], &tsb, &tv));
    for (int i = 0; i < naggs; i++) BG_TRY(fetch(cols[aggs[i].col], &out->bits[i], &out->valid[i]));   // (validate_aggs checked aggs[i].col)
    BG_HIP(hipStreamSynchronize(c->stream));
    out->ts = (int64_t)tsb;
    out->present = 1;
    return 0;
}

// largest point of the window grid {offset + k * interval} that is <= t; false when it is not an int64
static bool grid_floor(int64_t t, int64_t interval, int64_t offset_norm, int64_t *out) {
    const __int128 d = (__int128)t - offset_norm;
    const __int128 k = d >= 0 ? d / interval : -((-d + interval - 1) / interval);
    const __int128 b = k * interval + offset_norm;
    if (b < (__int128)INT64_MIN || b > (__int128)INT64_MAX) return false;
    *out = (int64_t)b;
    return true;
}

int bowgpu_shard_begin(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                       const bowgpu_agg *aggs, int32_t naggs, const int64_t *global_s0, bowgpu_shard_record *rec) {
    if (!cols || ncols <= 0 || !rec || !aggs) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    const bowgpu_options o = options_or(opts);
    int inclusive = o.inclusive ? 1 : 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    BG_TRY(shard_check(cols, aggs, naggs));
    memset(rec, 0, sizeof *rec);
    rec->naggs = naggs;
    rec->flags = global_s0 ? 1 : 0;
    rec->nrows = cols[ts_col].length;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    Plan plan;
    BG_TRY(plan_make(c, &cols[ts_col], interval, o.offset, &plan));  // type / interval / first-ts checks; first and last ts
    if (rec->nrows == 0) return 0;
    rec->first_ts = plan.first_ts;
    rec->last_ts = plan.last_ts;
    // the window grid is {offset + k * interval} whatever the frame's first row is (rolling.go:95-99): the window holding this
    // rank's last row starts on it.  Ids here are relative to `base`, a grid point at or below the rank's first row.
    int64_t base;
    if (global_s0) base = *global_s0;
    else if (!grid_floor(plan.first_ts, interval, plan.offset, &base))
        return fail(BOWGPU_ERR_UNSUPPORTED, "interval column reaches below the int64 window grid");
    plan.s0 = base;
    const int64_t wl = plan.last_ts < base ? 0 : (int64_t)(((uint64_t)plan.last_ts - (uint64_t)base) / (uint64_t)interval);
    // (window 0 of the real grid also takes the rows below s0: range_state_kernel starts at row 0 for it)
    rec->carry_from_ts = wl == 0 ? INT64_MIN : (int64_t)((uint64_t)base + (uint64_t)wl * (uint64_t)interval);
    if (inclusive)
        BG_TRY(shard_first_row(cols, ts_col, aggs, naggs, &rec->first_row));
    std::vector<bowgpu_out> no_outs(naggs);
    void *dummy;
    BG_TRY(ctx_pool(c, kPoolShard, 16384, &dummy));
    for (int i = 0; i < naggs; i++) {
        memset(&no_outs[i], 0, sizeof(bowgpu_out));
        no_outs[i].values = dummy; no_outs[i].validity = reinterpret_cast<uint8_t *>(dummy);
        no_outs[i].length = 0; no_outs[i].residency = BOWGPU_DEVICE;
    }
    AggJob job;
    const bool strict = strict_wanted(&o);
    const AggCall call = {cols, ncols, ts_col, plan, 0, strict, false};
    BG_TRY(job_build(c, call, aggs, naggs, no_outs.data(), wl, 0, false, &job));
    bowgpu_carry_state *dst = reinterpret_cast<bowgpu_carry_state *>(dummy);
    uint32_t far = 0;
    if (strict) BG_HIP(hipMemsetAsync(job.P.status + kAggStStrictTooLong, 0, 4, c->stream));
    BG_TRY(launch_range_state(c, job.P, 0, (uint64_t)wl, nullptr, dst, nullptr, 1, strict ? 1 : 0));
    BG_HIP(hipMemcpyAsync(rec->last, dst, sizeof(bowgpu_carry_state) * naggs, hipMemcpyDeviceToHost, c->stream));
    if (strict) BG_HIP(hipMemcpyAsync(&far, job.P.status + kAggStStrictTooLong, 4, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (far) return fail(BOWGPU_ERR_UNSUPPORTED, "strict_order: the shard's last window holds more than 2^20 rows (one lane walks a window in row order: beyond that the call is declined)");
    return 0;
}

// The rank's pass put in flight BEFORE the exchange, from its own record alone: output slot 0 = the window of the rank's first
// row on the offset-aligned grid, i.e. what bowgpu_shard_finish will decide whenever no empty windows lie in front of the rank
// (lead_empty_windows == 0) and no row lies below the frame's first window start.  Enqueued only - the call returns while the
// kernel runs - and collected by the bowgpu_shard_finish that follows on this thread; if the gathered records decide otherwise
// (a gap to the left neighbour, the negative-timestamp corner) finish discards it and runs the pass the serial way.
int bowgpu_shard_pass_begin(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                            const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, const bowgpu_shard_record *me) {
    if (!cols || ncols <= 0 || !outs || !me || !aggs) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    const bowgpu_options o = options_or(opts);
    int inclusive = o.inclusive ? 1 : 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    BG_TRY(shard_check(cols, aggs, naggs));
    if (cols[ts_col].type != BOWGPU_INT64) return fail(BOWGPU_ERR_TS_TYPE, "impossible to create a new intervalRolling on column of type float64");
    if (me->nrows != cols[ts_col].length) return fail(BOWGPU_ERR_ARG, "the record says %lld rows, the interval column has %lld",
                                                      (long long)me->nrows, (long long)cols[ts_col].length);
    PendingOwnerScope owner;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    pending_drop(c);
    c->last_slow_rows = 0;
    // declined (not an error): nothing to reduce, or timestamps below zero, where the frame's first window start may lie ABOVE
    // a rank's rows (rolling.go:96-99) - that needs the records
    if (me->nrows == 0 || me->first_ts < 0 || me->last_ts < me->first_ts) return BOWGPU_SHARD_PASS_DECLINED;
    PendingPass *pp = new PendingPass();
    Plan plan;
    plan.interval = interval;
    int rc = enforce_interval_and_offset(interval, o.offset, &plan.offset);
    int64_t base = 0;
    if (rc == 0 && !grid_floor(me->first_ts, interval, plan.offset, &base)) rc = BOWGPU_SHARD_PASS_DECLINED;
    if (rc != 0) { delete pp; return rc; }
    plan.magic = magic_make((uint64_t)interval);
    plan.s0 = base;                       // local numbering: slot k = window [base + k * interval, ...)
    plan.first_ts = me->first_ts;
    plan.last_ts = me->last_ts;
    plan.W = (int64_t)(((uint64_t)me->last_ts - (uint64_t)base) / (uint64_t)interval) + 1;
    pp->base = base;
    pp->n = me->nrows; pp->interval = interval; pp->raw_offset = o.offset; pp->ts_col = ts_col; pp->inclusive = inclusive;
    for (int i = 0; i < ncols; i++) pp->col_values.push_back(reinterpret_cast<const char *>(cols[i].values) + 8 * cols[i].offset);
    for (int i = 0; i < naggs; i++) pp->out_values.push_back(outs[i].values);
    const AggCall call = {cols, ncols, ts_col, plan, inclusive, strict_wanted(&o), false};
    rc = job_build(c, call, aggs, naggs, outs, 0, plan.W, false, &pp->job);
    if (rc == 0) rc = job_pass_enqueue(c, &pp->job, false, &pp->ps);
    if (rc != 0) { (void)hipStreamSynchronize(c->stream); delete pp; return rc; }
    pending_set(pp, pending_pass_delete);
    return 0;
}

int bowgpu_shard_plan(const bowgpu_shard_record *recs, int32_t world, int32_t rank, int64_t interval, int64_t raw_offset,
                      bowgpu_shard_decision *d) {
    if (!recs || !d || world <= 0 || rank < 0 || rank >= world) return fail(BOWGPU_ERR_ARG, "bad shard plan arguments");
    int64_t off;
    BG_TRY(enforce_interval_and_offset(interval, raw_offset, &off));
    memset(d, 0, sizeof *d);
    d->first_window_id = d->last_window_id = d->first_slot_window_id = -1;
    d->seed_first_rank = d->next_rank = -1;
    int g0 = -1, gl = -1;
    for (int q = 0; q < world; q++) {
        if (recs[q].nrows < 0) return fail(BOWGPU_ERR_ARG, "rank %d: negative row count", q);
        if (recs[q].nrows == 0) continue;
        if (recs[q].last_ts < recs[q].first_ts) return fail(BOWGPU_ERR_TS_UNSORTED, "interval column is not ascending on rank %d", q);
        if (gl >= 0 && recs[gl].last_ts > recs[q].first_ts)
            return fail(BOWGPU_ERR_TS_UNSORTED, "interval column is not ascending across ranks %d and %d", gl, q);
        if (g0 < 0) g0 = q;
        gl = q;
    }
    if (g0 < 0) return 0;  // no rows anywhere: no windows (rolling.go:143-146)
    const int64_t s0 = first_window_start(recs[g0].first_ts, interval, off);
    d->s0 = s0;
    d->holds_global_row0 = rank == g0;
    const int64_t last = recs[gl].last_ts;
    if (s0 > last) return 0;   // countWindows: s0 beyond the last row (only rows below s0) => no windows (rolling.go:150-152)
    if (last > 0 && s0 < 0 && (uint64_t)last - (uint64_t)s0 > (uint64_t)INT64_MAX)
        return fail(BOWGPU_ERR_UNSUPPORTED, "interval column spans more than 2^63: int64 overflow in the reference's countWindows");
    d->num_windows = (int64_t)(((uint64_t)last - (uint64_t)s0) / (uint64_t)interval) + 1;
    // first / last window of a rank; rows below s0 (Go's truncating division on negative timestamps) ride in window 0
    auto wid_of = [&](int64_t t) -> int64_t { return t < s0 ? 0 : (int64_t)(((uint64_t)t - (uint64_t)s0) / (uint64_t)interval); };
    auto wf = [&](int q) { return recs[q].nrows == 0 ? (int64_t)-1 : wid_of(recs[q].first_ts); };
    auto wl = [&](int q) { return recs[q].nrows == 0 ? (int64_t)-1 : wid_of(recs[q].last_ts); };
    auto left_of = [&](int q) { int r = q - 1; while (r >= 0 && recs[r].nrows == 0) r--; return r; };
    auto right_of = [&](int q) { int r = q + 1; while (r < world && recs[r].nrows == 0) r++; return r < world ? r : -1; };
    // window 0 with rows below s0 split over ranks: the first-attempt states were cut on the local grid
    if (s0 > recs[g0].first_ts)
        for (int q = 0; q < world; q++) {
            if (recs[q].nrows == 0 || (recs[q].flags & 1)) continue;
            const int r = right_of(q);
            if (wl(q) == 0 && r >= 0 && wf(r) == 0 && recs[q].carry_from_ts > recs[q].first_ts) d->retry_with_s0 = 1;
        }
    if (recs[rank].nrows == 0) return 0;
    const int64_t f = wf(rank), l = wl(rank);
    d->first_window_id = f;
    d->last_window_id = l;
    const int lq = left_of(rank), rq = right_of(rank);
    d->next_rank = rq;
    // empty windows between the left neighbour's last window and this rank's first one are this rank's to output; with nothing
    // to the left there are none (global row 0 lies in window 0)
    d->lead_empty_windows = lq < 0 ? 0 : std::max<int64_t>(0, f - wl(lq) - 1);
    // ranks (ascending) holding earlier rows of this rank's FIRST window
    int sf = -1;
    for (int q = lq; q >= 0 && wl(q) == f; q = left_of(q)) {
        sf = q;
        if (wf(q) != f) break;   // q only contributes its tail
    }
    d->seed_first_rank = sf;
    d->drops_last = rq >= 0 && wf(rq) == l;
    d->first_slot_window_id = f - d->lead_empty_windows;
    d->windows_local = l - f + 1 + d->lead_empty_windows;
    d->windows_owned = d->windows_local - (d->drops_last ? 1 : 0);
    d->finish_last = !d->drops_last && !(f == l && sf >= 0);
    return 0;
}

int bowgpu_shard_finish(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                        const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, const bowgpu_shard_record *recs, int32_t world,
                        int32_t rank, bowgpu_shard_decision *decision, bowgpu_agg_info *info) {
    if (!cols || ncols <= 0 || !outs || !recs || !aggs) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    PendingOwnerScope owner;   // (the pass in flight is this call's to collect or drop)
    const bowgpu_options o = options_or(opts);
    int inclusive = o.inclusive ? 1 : 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    BG_TRY(shard_check(cols, aggs, naggs));
    const bool strict = strict_wanted(&o);
    bowgpu_shard_decision d;
    BG_TRY(bowgpu_shard_plan(recs, world, rank, interval, o.offset, &d));
    if (decision) *decision = d;
    if (info) {
        memset(info, 0, sizeof *info);
        info->s0 = d.s0; info->num_windows = d.num_windows; info->new_interval_col = nic; info->inclusive = inclusive;
    }
    if (d.retry_with_s0) {
        Ctx *cc;
        if (pending_get() && ctx_get(&cc) == 0) pending_drop(cc);
        return BOWGPU_SHARD_RETRY;
    }
    const bowgpu_shard_record &me = recs[rank];
    if (me.nrows != cols[ts_col].length) return fail(BOWGPU_ERR_ARG, "record of rank %d says %lld rows, the interval column has %lld", rank,
                                                     (long long)me.nrows, (long long)cols[ts_col].length);
    if (cols[ts_col].type != BOWGPU_INT64) return fail(BOWGPU_ERR_TS_TYPE, "impossible to create a new intervalRolling on column of type float64");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (!pending_get()) c->last_slow_rows = 0;   // (a pass in flight has booked its rows already: bowgpu_shard_pass_begin reset the counter)
    // the rank's plan from its own record: no round trip to the device for first / last ts
    Plan plan;
    plan.interval = interval;
    BG_TRY(enforce_interval_and_offset(interval, o.offset, &plan.offset));
    plan.magic = magic_make((uint64_t)interval);
    plan.s0 = d.s0;
    plan.first_ts = me.first_ts;
    plan.last_ts = me.last_ts;
    const int64_t wf = d.first_window_id, wl = d.last_window_id, lead = d.lead_empty_windows;
    plan.W = wf < 0 ? 0 : wl - wf + 1;
    const int64_t Wtot = plan.W + lead;
    AggJob job;
    const bool pre_rows_here = me.nrows > 0 && me.first_ts < d.s0;   // rows below s0 ride in window 0 (rolling.go:194-196)
    int64_t n_long = 0;
    double ms = 0;
    // the pass bowgpu_shard_pass_begin put in flight before the exchange, if the records decide what it assumed
    bool collected = false;
    if (pending_get()) {
        PendingPass *pp = static_cast<PendingPass *>(pending_get());
        bool same = pp->n == me.nrows && pp->interval == interval && pp->raw_offset == o.offset && pp->ts_col == ts_col &&
                    pp->inclusive == inclusive && pp->job.naggs == naggs && (int32_t)pp->col_values.size() == ncols &&
                    memcmp(pp->job.aggs, aggs, sizeof(bowgpu_agg) * (size_t)naggs) == 0;
        for (int i = 0; same && i < ncols; i++) same = pp->col_values[i] == reinterpret_cast<const char *>(cols[i].values) + 8 * cols[i].offset;
        for (int i = 0; same && i < naggs; i++) same = pp->out_values[i] == outs[i].values;
        const bool holds = same && wf >= 0 && lead == 0 && !pre_rows_here && pp->job.plan.W == plan.W &&
                           pp->base == (int64_t)((uint64_t)d.s0 + (uint64_t)wf * (uint64_t)interval);
        if (holds) {
            pending_set(nullptr, nullptr);   // (collected here, not dropped)
            job = std::move(pp->job);   // (it owns copies of the aggregations and of the plan it was built with: nothing of *pp is referred to)
            job.strict = strict;        // (this call's options decide how the pass is completed)
            const int rc = job_pass_complete(c, &job, false, &pp->ps, &n_long, &ms);
            delete pp;
            if (rc != 0) return rc;
            // from the pass's local numbering (slot 0 starts at base) to the frame's: the stitch below speaks global window ids
            job.P.s0 = d.s0;
            job.P.wid_base = wf;
            for (int i = 0; i < naggs; i++) job.douts[i].user = &outs[i];   // (the descriptor array of THIS call receives length / null_count)
            collected = true;
        } else {
            pending_drop(c);
        }
    }
    if (!collected) {
        const AggCall call = {cols, ncols, ts_col, plan, inclusive, strict, false};
        BG_TRY(job_build(c, call, aggs, naggs, outs, wf < 0 ? 0 : wf - lead, Wtot, pre_rows_here, &job));
        BG_TRY(job_run(c, &job, &n_long, &ms, false));
    }
    if (lead > 0) BG_TRY(launch_fill_empty(c, job.P, 0, lead));
    if (plan.W > 0) {
        void *pool;
        BG_TRY(ctx_pool(c, kPoolShard, 16384, &pool));
        bowgpu_carry_state *dseed = reinterpret_cast<bowgpu_carry_state *>(pool);
        bowgpu_next_row *dnext = nullptr;
        const bowgpu_next_row *next_row = d.next_rank >= 0 ? &recs[d.next_rank].first_row : nullptr;
        if (inclusive && next_row && next_row->present) {
            dnext = reinterpret_cast<bowgpu_next_row *>(reinterpret_cast<char *>(pool) + 8192);
            BG_HIP(hipMemcpyAsync(dnext, next_row, sizeof *next_row, hipMemcpyHostToDevice, c->stream));
        }
        // the rank owns its last window and only now knows the row that may close it (rolling.go:201-209)
        if (dnext && d.finish_last) BG_TRY(launch_range_state(c, job.P, 2, (uint64_t)wl, nullptr, nullptr, dnext, 0, strict ? 1 : 0));
        if (d.seed_first_rank >= 0) {
            // running state of this rank's first window over the rows the ranks to the left hold: one rank's state as is,
            // several merged in rank order (empty ranks in between hold zero states: identity)
            bowgpu_carry_state seeds[BOWGPU_CARRY_MAX_AGGS];
            // (window 0 stitched across shards is an empty slice unless one of its rows reaches s0: range_state_kernel's rule)
            int seed_alive = 0;
            for (int q = d.seed_first_rank; q < rank; q++)
                if (recs[q].nrows > 0 && recs[q].last_ts >= d.s0) seed_alive = 1;
            if (strict) {   // (a window spread over three or more ranks merges the middle ranks' partial sums: not row order)
                int with_rows = 0;
                for (int q = d.seed_first_rank; q < rank; q++) with_rows += recs[q].nrows > 0;
                if (with_rows > 1) return fail(BOWGPU_ERR_UNSUPPORTED, "strict_order: a window is spread over three or more shards (its middle shards contribute partial sums)");
            }
            for (int a = 0; a < naggs; a++) {
                seeds[a] = recs[d.seed_first_rank].last[a];
                for (int q = d.seed_first_rank + 1; q < rank; q++) {
                    if (recs[q].nrows == 0) continue;
                    bowgpu_carry_state m;
                    BG_TRY(bowgpu_carry_merge(&seeds[a], &recs[q].last[a], &m));
                    seeds[a] = m;
                }
            }
            // (the records were built by the caller's all_gather: pageable memory, so stage through the pinned block)
            bowgpu_carry_state *hseed;
            static_assert(sizeof seeds == kRegSeeds.size, "the registered block's seeds");
            BG_TRY(registered_at(c, kRegSeeds, &hseed));
            memcpy(hseed, seeds, sizeof(bowgpu_carry_state) * naggs);
            BG_HIP(hipMemcpyAsync(dseed, hseed, sizeof(bowgpu_carry_state) * naggs, hipMemcpyHostToDevice, c->stream));
            // the window may also be the rank's last one: then the next rank's first row can be its inclusive row
            const bool also_last = wf == wl && !d.drops_last;
            BG_TRY(launch_range_state(c, job.P, 1, (uint64_t)wf, dseed, nullptr, also_last ? dnext : nullptr, seed_alive, strict ? 1 : 0));
        }
    }
    BG_TRY(job_finish(c, &job, strict));
    if (info) { info->long_windows = n_long; info->kernel_ms = ms; }
    return 0;
}

}  // extern "C"
