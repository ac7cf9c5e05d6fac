// aggregate_api.cpp — the unsharded Rolling.Aggregate call: window planning, argument validation mirroring the reference's
// drivers, the paths for Mode, Boolean columns and an interval column with nulls, and the bowgpu_rolling_* / bowgpu_plan_windows* /
// bowgpu_window_bounds entry points.

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "agg_host.h"

namespace bowgpu {

// ---------------------------------------------------------------- plan
static int fetch_i64(Ctx *c, const bowgpu_col *col, int64_t row, int64_t *out) {
    const int64_t *p = reinterpret_cast<const int64_t *>(col->values) + col->offset + row;
    if (col->residency == BOWGPU_DEVICE) {
        if (!c) BG_TRY(ctx_get(&c));
        BG_HIP(hipMemcpyAsync(out, p, 8, hipMemcpyDeviceToHost, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
    } else {
        *out = *p;
    }
    return 0;
}

int enforce_interval_and_offset(int64_t interval, int64_t offset, int64_t *out) {
    // reference rolling/rolling.go:114-128
    if (interval <= 0) return fail(BOWGPU_ERR_INTERVAL, "strictly positive interval required");
    if (offset >= interval || offset <= -interval) offset = offset % interval;
    if (offset < 0) offset += interval;
    *out = offset;
    return 0;
}

// s0 of newIntervalRolling (rolling.go:95-99) from the first timestamp: Go's (first/interval)*interval + offset with
// truncating division and wrapping int64 arithmetic
int64_t first_window_start(int64_t first, int64_t interval, int64_t offset_norm) {
    int64_t s0 = (int64_t)((uint64_t)((first / interval) * interval) + (uint64_t)offset_norm);
    if (s0 > first) s0 = (int64_t)((uint64_t)s0 - (uint64_t)interval);
    return s0;
}

int plan_make(Ctx *c, const bowgpu_col *ts, int64_t interval, int64_t raw_offset, Plan *p) {
    // reference rolling/rolling.go:69-112 and :143-154
    if (ts->type != BOWGPU_INT64)
        return fail(BOWGPU_ERR_TS_TYPE, "impossible to create a new intervalRolling on column of type %s", arrow_type_name(ts->type));
    BG_TRY(enforce_interval_and_offset(interval, raw_offset, &p->offset));
    p->interval = interval;
    p->magic = magic_make((uint64_t)interval);
    p->s0 = 0;
    p->W = 0;
    const int64_t n = ts->length;
    if (n == 0) return 0;
    int64_t first = 0, last = 0;
    int64_t row = n - 1;
    if (!ts->validity) {
        // common case (no validity buffer): both scalars with one round trip
        const int64_t *base = reinterpret_cast<const int64_t *>(ts->values) + ts->offset;
        if (ts->residency == BOWGPU_DEVICE) {
            if (!c) BG_TRY(ctx_get(&c));
            int64_t *hp;
            BG_TRY(registered_at(c, kRegTwoTs, &hp));
            BG_TRY(launch_fetch_two(c, base, 0, n - 1, hp));   // (the kernel stores into the registered block)
            BG_HIP(hipStreamSynchronize(c->stream));
            first = hp[0]; last = hp[1];
        } else {
            first = base[0]; last = base[n - 1];
        }
    } else {
        int valid = 1;
        BG_TRY(fetch_valid(c, ts, 0, &valid));
        if (!valid) return fail(BOWGPU_ERR_FIRST_TS_NULL, "the first value of the column should be convertible to int64, got <nil>");
        BG_TRY(fetch_i64(c, ts, 0, &first));
    }
    p->first_ts = first;
    const int64_t s0 = first_window_start(first, interval, p->offset);
    p->s0 = s0;
    if (ts->validity) {
        // countWindows: last VALID ts scanning backwards (GetPrevInt64, bowgetters.go:189-199)
        int lv = 1;
        while (row >= 0) {
            BG_TRY(fetch_valid(c, ts, row, &lv));
            if (lv) break;
            row--;
        }
        if (row < 0) { p->W = 0; return 0; }
        BG_TRY(fetch_i64(c, ts, row, &last));
    }
    p->last_ts = last;
    if (s0 > last) { p->W = 0; return 0; }
    p->W = (int64_t)(((uint64_t)last - (uint64_t)s0) / (uint64_t)interval) + 1;
    // the reference computes (last - s0)/interval in int64: decline ranges where that wraps
    if ((last > 0 && s0 < 0 && (uint64_t)last - (uint64_t)s0 > (uint64_t)INT64_MAX))
        return fail(BOWGPU_ERR_UNSUPPORTED, "interval column spans more than 2^63: int64 overflow in the reference's countWindows");
    return 0;
}

// ---------------------------------------------------------------- aggregate
bool kind_needs_inclusive(int kind) {
    // NewColAggregation(col, true, ...) only at integral.go:9 and weightedmean.go:24
    return kind == BOWGPU_AGG_INTEGRAL_TRAPEZOID || kind == BOWGPU_AGG_WAVG_LINEAR;
}

int kind_type(int kind) {
    switch (kind) {
    case BOWGPU_AGG_WINDOW_START: return BOWGPU_ITERATOR_DEPENDENT;  // windowstart.go:9
    case BOWGPU_AGG_COUNT: return BOWGPU_INT64;                      // count.go:9
    case BOWGPU_AGG_FIRST:
    case BOWGPU_AGG_LAST: return BOWGPU_INPUT_DEPENDENT;             // firstlast.go:9,:24
    case BOWGPU_AGG_MODE: return BOWGPU_INPUT_DEPENDENT;             // mode.go:9
    default: return BOWGPU_FLOAT64;
    }
}

bool kind_never_nil(int kind) {
    return kind == BOWGPU_AGG_WINDOW_START || kind == BOWGPU_AGG_SUM || kind == BOWGPU_AGG_COUNT || kind == BOWGPU_AGG_NUM_ROWS;
}

bool kind_reads_values(int kind) { return !(kind == BOWGPU_AGG_WINDOW_START || kind == BOWGPU_AGG_NUM_ROWS); }

// validation shared by the single-GPU and the sharded entry points
// (indexedAggregations + validateAggregation: reference rolling/aggregation.go:147-188)
int validate_aggs(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs,
                  int *inclusive, int *new_interval_col) {
    if (naggs <= 0) return fail(BOWGPU_ERR_NO_AGG, "at least one column aggregation is required");
    int nic = -1;
    for (int i = 0; i < naggs; i++) {
        if (aggs[i].col < 0 || aggs[i].col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "aggregation %d: no column with index %d", i, aggs[i].col);
        if (aggs[i].kind < 0 || aggs[i].kind >= BOWGPU_AGG__COUNT) return fail(BOWGPU_ERR_ARG, "aggregation %d: unknown kind %d", i, aggs[i].kind);
        if (aggs[i].n_factors < 0 || aggs[i].n_factors > BOWGPU_MAX_FACTORS) return fail(BOWGPU_ERR_ARG, "aggregation %d: bad factor count", i);
        const int t = cols[aggs[i].col].type;
        if (t == BOWGPU_STRING)
            return fail(BOWGPU_ERR_UNSUPPORTED, "aggregation %d: a String column is outside the device path (Float64 / Int64 / Boolean)", i);
        if (t != BOWGPU_FLOAT64 && t != BOWGPU_INT64 && t != BOWGPU_BOOLEAN)
            return fail(BOWGPU_ERR_UNSUPPORTED, "aggregation %d: column type %d is outside the device path (Float64 / Int64 / Boolean)", i, t);
        // transformation.Factor on a Boolean result (factor.go:7-20: "factor: invalid type bool" at the first non-nil value): the
        // caller keeps the reference's path and gets the reference's error
        if (t == BOWGPU_BOOLEAN && aggs[i].n_factors > 0 && kind_type(aggs[i].kind) == BOWGPU_INPUT_DEPENDENT)
            return fail(BOWGPU_ERR_UNSUPPORTED, "aggregation %d: factor: invalid type bool (a Factor on the Boolean result of First / Last / Mode is outside the device path)", i);
        if (kind_needs_inclusive(aggs[i].kind)) *inclusive = 1;  // aggregation.go:183-185
        if (aggs[i].col == ts_col) nic = i;                      // aggregation.go:158-160 (last one wins)
    }
    if (nic == -1) return fail(BOWGPU_ERR_KEEP_INTERVAL, "must keep interval column");
    *new_interval_col = nic;
    return 0;
}

uint32_t need_mask(const bowgpu_agg *aggs, int32_t naggs) {
    uint32_t need = 0;
    for (int i = 0; i < naggs; i++) {
        const int k = aggs[i].kind;
        if (k == BOWGPU_AGG_INTEGRAL_STEP || k == BOWGPU_AGG_WAVG_STEP) need |= kNeedStep;
        if (k == BOWGPU_AGG_INTEGRAL_TRAPEZOID || k == BOWGPU_AGG_WAVG_LINEAR) need |= kNeedTrap;
        if (k == BOWGPU_AGG_MIN || k == BOWGPU_AGG_MAX) need |= kNeedMinMax;
        if (k == BOWGPU_AGG_SUM || k == BOWGPU_AGG_MEAN) need |= kNeedSum;
        if (k == BOWGPU_AGG_FIRST || k == BOWGPU_AGG_LAST) need |= kNeedFirstLast;
        if (k == BOWGPU_AGG_MODE) need |= kNeedMode;
    }
    return need;
}

// reducers that read a BOOLEAN value column (rolling_bool.hip; run_aggregate_bool)
static bool kind_time_weighted(int kind) { return kind >= BOWGPU_AGG_INTEGRAL_STEP && kind <= BOWGPU_AGG_WAVG_LINEAR; }
static bool agg_reads_bool(const bowgpu_col *cols, const bowgpu_agg &a) { return kind_reads_values(a.kind) && cols[a.col].type == BOWGPU_BOOLEAN; }
static bool any_bool_agg(const bowgpu_col *cols, const bowgpu_agg *aggs, int32_t naggs) {
    for (int i = 0; i < naggs; i++) if (agg_reads_bool(cols, aggs[i])) return true;
    return false;
}

static int check_row_counts(const bowgpu_col *cols, int32_t ncols, int32_t ts_col) {
    const int64_t n = cols[ts_col].length;
    for (int i = 0; i < ncols; i++)
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "column %d has %lld rows, interval column has %lld", i, (long long)cols[i].length, (long long)n);
    return 0;
}
// ... and the device path's contract: no null timestamps (run_aggregate has sent such a call to run_aggregate_null_ts)
int front_check(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col) {
    BG_TRY(check_row_counts(cols, ncols, ts_col));
    const bowgpu_col *tsc = &cols[ts_col];
    if (tsc->validity && tsc->null_count != 0) {
        DevCol probe;
        BG_TRY(devcol_prepare(c, tsc, &probe, false, true));
        if (probe.null_count > 0)
            return fail(BOWGPU_ERR_TS_NULLS, "interval column has %lld nulls: outside the device path", (long long)probe.null_count);
    }
    return 0;
}

bool strict_wanted(const bowgpu_options *o) { return (o && o->strict_order) || (route_mask() & BOWGPU_ROUTE_STRICT_ORDER); }

// The first row of every window of a call (launch_window_first_rows) and the interval column it was made from: what the passes over
// window row ranges read (Mode, the Boolean value reducers).  Made once per call, by whichever pass needs it first.
struct WindowRows {
    DevCol dts;
    DevBuf first_idx;   // [W + 1]
    bool ready = false;
};
static int window_rows_make(Ctx *c, const AggCall &call, WindowRows *wr) {
    if (wr->ready) return 0;
    const bowgpu_col *tsc = &call.cols[call.ts_col];
    const int64_t n = tsc->length, W = call.plan.W;
    bowgpu_col t = *tsc;
    t.validity = nullptr;
    t.null_count = 0;
    BG_TRY(devcol_prepare(c, &t, &wr->dts, true, false));
    BG_TRY(wr->first_idx.alloc((size_t)(W + 1) * 8));
    uint32_t *status;
    BG_TRY(scratch_at(c, kScrStatus, &status));
    BG_HIP(hipMemsetAsync(status, 0, kStatusHeadBytes, c->stream));
    BG_TRY(launch_window_first_rows(c, reinterpret_cast<const int64_t *>(wr->dts.values), n, call.plan, reinterpret_cast<int64_t *>(wr->first_idx.p), status));
    uint32_t hstat[4] = {0, 0, 0, 0};
    BG_HIP(hipMemcpyAsync(hstat, status, 16, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (hstat[kAggStUnsorted]) return fail_ts_unsorted();   // (window_first_rows_kernel keeps the Aggregate kernels' word for it)
    wr->ready = true;
    return 0;
}

// aggregation.Mode outputs (mode.go:8-32): not a streaming reducer, so they run apart from the tile kernels, over the
// windows' row ranges (an inclusive window reaches them without its extra row: window.go:23-31, aggregation.go:207-211)
static int run_modes(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, int64_t *long_windows, WindowRows *shared) {
    const bowgpu_col *cols = call.cols;
    const int32_t ts_col = call.ts_col;
    const Plan &plan = call.plan;
    const bowgpu_col *tsc = &cols[ts_col];
    const int64_t n = tsc->length, W = plan.W;
    BG_TRY(front_check(c, cols, call.ncols, ts_col));
    WindowRows own;
    WindowRows *wr = shared ? shared : &own;
    if (W > 0) BG_TRY(window_rows_make(c, call, wr));
    const DevCol &dts = wr->dts;
    const DevBuf &first_idx = wr->first_idx;
    for (int i = 0; i < naggs; i++) {
        if (aggs[i].kind != BOWGPU_AGG_MODE) continue;
        const int col = aggs[i].col;
        DevCol dc;
        const void *values = dts.values;
        const uint32_t *vbits = nullptr;
        int64_t vbit0 = 0;
        if (col != ts_col && W > 0) {
            BG_TRY(devcol_prepare(c, &cols[col], &dc, true, true));
            values = dc.values; vbits = dc.vbits; vbit0 = dc.vbit0;
        }
        DevOut d;
        BG_TRY(devout_prepare(c, &outs[i], W, &d, kPoolMode));
        int64_t nulls = 0;
        if (W > 0) {
            BG_HIP(hipMemsetAsync(d.validity, 0, temp_bits_bytes((size_t)((W + 7) >> 3)), c->stream));
            int64_t n_mid = 0, n_long = 0;
            BG_TRY(launch_mode(c, reinterpret_cast<const int64_t *>(dts.values), reinterpret_cast<const int64_t *>(first_idx.p), n, plan.s0, plan.interval, W,
                               plan.s0 > plan.first_ts ? 1 : 0, call.inclusive, values, vbits, vbit0, cols[col].type == BOWGPU_INT64, &aggs[i], d.values,
                               reinterpret_cast<uint32_t *>(d.validity), &n_mid, &n_long));
            // (Mode is bit-exact in every size class; the classes beyond a lane's are reported for the tests - not under strict_order,
            // whose contract is long_windows == 0)
            if (long_windows && !call.strict) *long_windows += n_mid + n_long;
            BG_TRY(recount_nulls(c, d.validity, W, &nulls));
        }
        BG_TRY(devout_finish(c, &d, W, cols[col].type, nulls));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// (mutually recursive with the two rewriting paths below, which hand it the call they rewrote: the one declaration ahead of a definition here)
static int run_aggregate(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, int64_t *long_windows, double *kernel_ms,
                         WindowRows *rows = nullptr);

// An interval column WITH NULLS (ts_nulls.hip has the semantics: rolling.go:177-239 skips such rows, :143-154 counts windows from the
// last valid timestamp, :162-173 ends the iteration at once when the physically last timestamp is null).  The call is rewritten
// onto a dense interval column - nulls forward-filled - with every value column's validity ANDed with the rows that belong to a
// window (and, for the time-weighted reducers, with the interval column's own validity), and then takes the ordinary path into
// device temporaries; NumRows is counted as Count over the rows that belong to a window; after an inclusive iteration the windows
// behind a row on a window start with a null timestamp right behind it get the outputs of IntegralTrapezoid / WeightedAverageLinear
// from ts_quirk_fix_kernel.  Unsharded calls; Mode is declined.
static int run_aggregate_null_ts(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, DevCol &dts,
                                 int64_t *long_windows, double *kernel_ms) {
    const bowgpu_col *cols = call.cols;
    const int32_t ncols = call.ncols, ts_col = call.ts_col;
    const Plan &plan = call.plan;
    const int inclusive = call.inclusive;
    const bowgpu_col *tsc = &cols[ts_col];
    const int64_t n = tsc->length, W = plan.W;
    if (need_mask(aggs, naggs) & kNeedMode)
        return fail(BOWGPU_ERR_TS_NULLS, "interval column has %lld nulls: Mode over it is outside the device path", (long long)dts.null_count);
    if (any_bool_agg(cols, aggs, naggs))
        return fail(BOWGPU_ERR_TS_NULLS, "interval column has %lld nulls: a Boolean column over it is outside the device path", (long long)dts.null_count);
    BG_TRY(check_row_counts(cols, ncols, ts_col));
    if (long_windows) *long_windows = 0;
    if (kernel_ms) *kernel_ms = 0;
    int last_valid = 1;
    BG_TRY(fetch_valid(c, tsc, n - 1, &last_valid));
    if (!last_valid || W == 0) {
        // HasNext (rolling.go:162-173) is false from the start when the physically last timestamp is null: no window is ever
        // produced and every slot of the numWindows-long output buffers stays nil (bowbuffer.go:22-40: zero data, all-null bitmap)
        for (int i = 0; i < naggs; i++) {
            DevOut d;
            BG_TRY(devout_prepare(c, &outs[i], W, &d, i));
            int t = kind_type(aggs[i].kind);
            if (t == BOWGPU_INPUT_DEPENDENT) t = cols[aggs[i].col].type;
            if (t == BOWGPU_ITERATOR_DEPENDENT) t = tsc->type;
            if (W > 0) {
                BG_HIP(hipMemsetAsync(d.values, 0, (size_t)W * 8, c->stream));
                BG_HIP(hipMemsetAsync(d.validity, 0, (size_t)((W + 7) >> 3), c->stream));
            }
            BG_TRY(devout_finish(c, &d, W, t, W));
            BG_HIP(hipStreamSynchronize(c->stream));
        }
        return 0;
    }
    // the interval column forward-filled + which rows belong to a window (+ inclusive: its validity without the rows ts_nulls.hip describes)
    DevBuf ixbuf, ts_eff, keep, plain_ts, dropped;
    NbrIndex ix;
    BG_TRY(ixbuf.alloc(nbr_index_bytes(n, dts.vbit0)));
    BG_TRY(nbr_index_build(c, dts.vbits, dts.vbit0, n, ixbuf.p, &ix));
    BG_TRY(ts_eff.alloc((size_t)n * 8 + 16));
    const size_t bm_bytes = (size_t)((n + 63) >> 6) * 8 + 8;
    BG_TRY(keep.alloc(bm_bytes));
    if (inclusive) BG_TRY(plain_ts.alloc(bm_bytes));
    BG_TRY(dropped.alloc(16));
    BG_TRY(launch_ts_nullfill(c, reinterpret_cast<const int64_t *>(dts.values), dts.vbits, dts.vbit0, n, ix, plan.s0, plan.interval, plan.magic, inclusive,
                              reinterpret_cast<int64_t *>(ts_eff.p), reinterpret_cast<uint64_t *>(keep.p), reinterpret_cast<uint64_t *>(plain_ts.p),
                              reinterpret_cast<unsigned long long *>(dropped.p)));
    // one rewritten column per (input column, class of reducer) that some reducer reads:
    //   plain       value validity AND keep
    //   step        IntegralStep / WeightedAverageStep: their points are the rows with timestamp AND value (bowgetters.go:299-311); they read
    //               windows through UnsetInclusive, so after an inclusive iteration the rows ts_nulls.hip describes are not among them
    //   linear      IntegralTrapezoid / WeightedAverageLinear: value validity AND the interval column's
    //   rows        NumRows: Count over keep itself
    enum { kPlain = 0, kStep = 1, kLinear = 2, kClasses = 3 };
    std::vector<bowgpu_col> cols2(cols, cols + ncols);
    std::vector<bowgpu_agg> aggs2(aggs, aggs + naggs);
    std::vector<DevCol> dcs(ncols);
    std::vector<DevBuf> bitmaps;
    bitmaps.reserve(kClasses * (size_t)ncols + 1);
    std::vector<int> slot_of(kClasses * (size_t)ncols, -1);
    int rows_slot = -1;
    {
        bowgpu_col &t = cols2[ts_col];
        t.values = ts_eff.p; t.validity = nullptr; t.offset = 0; t.length = n; t.null_count = 0; t.type = BOWGPU_INT64; t.residency = BOWGPU_DEVICE;
    }
    auto device_col = [&](int col, const void **values, const uint32_t **vbits, int64_t *vbit0) -> int {
        if (col == ts_col) { *values = dts.values; *vbits = dts.vbits; *vbit0 = dts.vbit0; return 0; }
        DevCol &dc = dcs[col];
        if (dc.values == nullptr) BG_TRY(devcol_prepare(c, &cols[col], &dc, true, true));
        *values = dc.values; *vbits = dc.vbits; *vbit0 = dc.vbit0;
        return 0;
    };
    bool any_linear = false;
    for (int i = 0; i < naggs; i++) {
        const int kind = aggs[i].kind;
        if (kind == BOWGPU_AGG_NUM_ROWS) {
            if (rows_slot < 0) {
                bowgpu_col nc;
                nc.values = ts_eff.p; nc.validity = reinterpret_cast<const uint8_t *>(keep.p); nc.offset = 0; nc.length = n; nc.null_count = -1;
                nc.type = BOWGPU_INT64; nc.residency = BOWGPU_DEVICE;
                rows_slot = (int)cols2.size();
                cols2.push_back(nc);
            }
            aggs2[i].kind = BOWGPU_AGG_COUNT;
            aggs2[i].col = rows_slot;
            aggs2[i].n_factors = 0;      // (a Factor chain multiplies float64(NumRows): launch_count_to_f64 below applies it, not the Int64 Count)
            continue;
        }
        if (!kind_reads_values(kind)) continue;
        const int col = aggs[i].col;
        const bool linear = kind_needs_inclusive(kind);
        const bool tw = kind >= BOWGPU_AGG_INTEGRAL_STEP && kind <= BOWGPU_AGG_WAVG_LINEAR;
        const int cls = linear ? kLinear : tw ? kStep : kPlain;
        any_linear |= linear;
        int &slot = slot_of[(size_t)cls * ncols + col];
        if (slot < 0) {
            const uint32_t *vbits; int64_t vbit0; const void *values;
            BG_TRY(device_col(col, &values, &vbits, &vbit0));
            bitmaps.emplace_back();
            DevBuf &bm = bitmaps.back();
            BG_TRY(bm.alloc(bm_bytes));
            if (cls == kPlain) BG_TRY(launch_and_bits(c, vbits, vbit0, reinterpret_cast<const uint32_t *>(keep.p), 0, n, reinterpret_cast<uint64_t *>(bm.p)));
            else if (cls == kStep && inclusive) BG_TRY(launch_and_bits(c, vbits, vbit0, reinterpret_cast<const uint32_t *>(plain_ts.p), 0, n, reinterpret_cast<uint64_t *>(bm.p)));
            else BG_TRY(launch_and_bits(c, vbits, vbit0, dts.vbits, dts.vbit0, n, reinterpret_cast<uint64_t *>(bm.p)));
            bowgpu_col nc;
            nc.values = values; nc.validity = reinterpret_cast<const uint8_t *>(bm.p); nc.offset = 0; nc.length = n; nc.null_count = -1;
            nc.type = cols[col].type; nc.residency = BOWGPU_DEVICE;
            slot = (int)cols2.size();
            cols2.push_back(nc);
        }
        aggs2[i].col = slot;
    }
    // the ordinary path, into device temporaries
    DevFrame tmp;
    BG_TRY(tmp.alloc(c, naggs, W, false));
    const AggCall dense = {cols2.data(), (int32_t)cols2.size(), ts_col, plan, inclusive, call.strict, call.check_plan};
    BG_TRY(run_aggregate(c, dense, aggs2.data(), naggs, tmp.outs.data(), long_windows, kernel_ms));
    for (int i = 0; i < naggs; i++)
        if (aggs[i].kind == BOWGPU_AGG_NUM_ROWS) {
            BG_TRY(launch_count_to_f64(c, tmp.values[i].as<uint64_t>(), tmp.bits[i].as<const uint32_t>(), W, aggs[i].n_factors, aggs[i].factors));
            tmp.outs[i].type = BOWGPU_FLOAT64;
        }
    if (inclusive && any_linear) {
        unsigned long long *d_fixed = reinterpret_cast<unsigned long long *>(dropped.p) + 1;
        BG_HIP(hipMemsetAsync(d_fixed, 0, 8, c->stream));
        std::vector<int> fixed;
        QuirkFix fx;
        fx.naggs = 0; fx._pad = 0;
        auto flush = [&]() -> int {
            if (fx.naggs) BG_TRY(launch_ts_quirk_fix(c, reinterpret_cast<const int64_t *>(dts.values), dts.vbits, dts.vbit0, n, ix, plan.s0, plan.interval, plan.magic,
                                                    W, fx, d_fixed));
            fx.naggs = 0;
            return 0;
        };
        for (int i = 0; i < naggs; i++) {
            if (!kind_needs_inclusive(aggs[i].kind)) continue;
            QuirkFixAgg &fa = fx.a[fx.naggs++];
            BG_TRY(device_col(aggs[i].col, &fa.values, &fa.vbits, &fa.vbit0));
            fa.out_values = tmp.values[i].as<uint64_t>(); fa.out_valid = tmp.bits[i].as<uint32_t>();
            fa.type = cols[aggs[i].col].type; fa.kind = aggs[i].kind; fa.n_factors = aggs[i].n_factors; fa._pad = 0;
            for (int f = 0; f < BOWGPU_MAX_FACTORS; f++) fa.factors[f] = aggs[i].factors[f];
            fixed.push_back(i);
            if (fx.naggs == 8) BG_TRY(flush());
        }
        BG_TRY(flush());
        // their null counts again
        for (int i : fixed) BG_TRY(recount_nulls(c, tmp.bits[i].p, W, &tmp.outs[i].null_count));
    }
    // ... and on to the caller's columns
    for (int i = 0; i < naggs; i++) BG_TRY(temp_to_caller(c, tmp, i, W, tmp.outs[i].type, tmp.outs[i].null_count, &outs[i], i));
    return 0;
}

// The value reducers over Boolean columns (aggs[at[.]]: Sum, ArithmeticMean, Min, Max, Count, First, Last, Mode): per column one
// launch of bool_windows_kernel over the window row ranges for every reducer asked of it (kBoolMaxOuts outputs a launch).  Every
// output goes through devout_prepare / devout_finish; a BOOLEAN one (First / Last / Mode) has bit-packed values.  *ms: the kernels' bracket.
static int run_bools(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, const std::vector<int> &at, bowgpu_out *outs, WindowRows *wr, double *ms) {
    const bowgpu_col *cols = call.cols;
    const Plan &plan = call.plan;
    const int64_t n = cols[call.ts_col].length, W = plan.W;
    DevBuf counter;
    if (W > 0) {
        BG_TRY(window_rows_make(c, call, wr));
        BG_TRY(counter.alloc(256));
    }
    std::vector<char> taken(at.size(), 0);
    for (size_t j0 = 0; j0 < at.size(); j0++) {
        if (taken[j0]) continue;
        const int col = aggs[at[j0]].col;
        std::vector<int> grp;   // the outputs of this launch: reducers of `col`, in output order
        for (size_t j = j0; j < at.size() && (int)grp.size() < kBoolMaxOuts; j++)
            if (!taken[j] && aggs[at[j]].col == col) { grp.push_back(at[j]); taken[j] = 1; }
        DevBoolCol dc;
        BoolParams P;
        memset(&P, 0, sizeof P);
        if (W > 0) {
            BG_TRY(devboolcol_prepare(c, &cols[col], &dc));
            P.ts = reinterpret_cast<const int64_t *>(wr->dts.values);
            P.first_idx = reinterpret_cast<const int64_t *>(wr->first_idx.p);
            P.s0 = plan.s0; P.n = n; P.interval = plan.interval; P.W = W;
            P.pre_rows = plan.s0 > plan.first_ts ? 1 : 0;
            P.inclusive = call.inclusive;
            P.tbits = dc.t.words; P.tbit0 = dc.t.bit0;
            P.vbits = dc.v.words; P.vbit0 = dc.v.bit0;
            P.null_windows = counter.as<unsigned long long>();
            P.nouts = (int32_t)grp.size();
        }
        std::vector<DevOut> douts(grp.size());
        std::vector<int> types(grp.size());
        for (size_t o = 0; o < grp.size(); o++) {
            const int i = grp[o];
            int t = kind_type(aggs[i].kind);
            if (t == BOWGPU_INPUT_DEPENDENT) t = BOWGPU_BOOLEAN;   // aggregation.go:114-115
            types[o] = t;
            BoolOut &q = P.outs[o];
            q.kind = aggs[i].kind;
            q.nfac = aggs[i].n_factors;
            for (int f = 0; f < aggs[i].n_factors; f++) q.fac[f] = aggs[i].factors[f];
            BG_TRY(devout_prepare(c, &outs[i], W, &douts[o], -1, t == BOWGPU_BOOLEAN));
            q.values = douts[o].values;
            q.valid = reinterpret_cast<uint32_t *>(douts[o].validity);
        }
        unsigned long long null_windows = 0;
        if (W > 0) {
            BG_HIP(hipMemsetAsync(P.null_windows, 0, 8, c->stream));
            BG_HIP(hipEventRecord(c->ev0, c->stream));
            BG_TRY(launch_bool_windows(c, P));
            BG_HIP(hipEventRecord(c->ev1, c->stream));
            BG_HIP(hipMemcpyAsync(&null_windows, P.null_windows, 8, hipMemcpyDeviceToHost, c->stream));
            BG_HIP(hipStreamSynchronize(c->stream));
            float t = 0;
            BG_HIP(hipEventElapsedTime(&t, c->ev0, c->ev1));
            if (ms) *ms += t;
        }
        for (size_t o = 0; o < grp.size(); o++) {
            const int i = grp[o];
            const int64_t nulls = kind_never_nil(aggs[i].kind) ? 0 : (int64_t)null_windows;
            BG_TRY(devout_finish(c, &douts[o], W, types[o], nulls));
        }
        BG_HIP(hipStreamSynchronize(c->stream));   // (the temporaries of this launch go back to the block cache)
    }
    return 0;
}

// A call that reads Boolean value columns.  The time-weighted reducers over such a column get it widened to a Float64 device
// temporary of 0.0 / 1.0 (8 bytes per row for the call) with its validity beside it, and go with every reducer over the other
// columns through the ordinary batches; the value reducers over Boolean columns are set aside, as Mode is, for run_bools.
static int run_aggregate_bool(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, int64_t *long_windows,
                              double *kernel_ms) {
    const bowgpu_col *cols = call.cols;
    const int32_t ncols = call.ncols;
    const int64_t n = cols[call.ts_col].length;
    BG_TRY(front_check(c, cols, ncols, call.ts_col));
    std::vector<bowgpu_col> cols2(cols, cols + ncols);
    std::vector<int> wide_slot(ncols, -1);
    std::vector<DevBuf> wide_values(ncols), wide_valid(ncols);
    std::vector<bowgpu_agg> rest;
    std::vector<bowgpu_out> rest_outs;
    std::vector<int> rest_at, bool_at;
    double ms_bool = 0;
    for (int i = 0; i < naggs; i++) {
        bowgpu_agg a = aggs[i];
        if (agg_reads_bool(cols, a)) {
            if (!kind_time_weighted(a.kind)) { bool_at.push_back(i); continue; }
            const int col = a.col;
            if (wide_slot[col] < 0) {
                bowgpu_col nc = device_col(nullptr, n, BOWGPU_FLOAT64);
                if (n > 0) {
                    DevBoolCol dc;
                    BG_TRY(devboolcol_prepare(c, &cols[col], &dc));
                    BG_TRY(wide_values[col].alloc(temp_values_bytes(n)));
                    if (dc.v.words) BG_TRY(wide_valid[col].alloc(temp_bits_bytes((size_t)((n + 7) >> 3))));
                    BG_HIP(hipEventRecord(c->ev0, c->stream));
                    BG_TRY(launch_bool_widen(c, dc.t.words, dc.t.bit0, dc.v.words, dc.v.bit0, n, wide_values[col].as<double>(), wide_valid[col].as<uint32_t>()));
                    BG_HIP(hipEventRecord(c->ev1, c->stream));
                    BG_HIP(hipStreamSynchronize(c->stream));   // (the staged bits go back to the block cache)
                    float t = 0;
                    BG_HIP(hipEventElapsedTime(&t, c->ev0, c->ev1));
                    ms_bool += t;
                    nc.values = wide_values[col].p;
                    if (dc.v.words) { nc.validity = wide_valid[col].as<uint8_t>(); nc.null_count = cols[col].null_count; }
                }
                wide_slot[col] = (int)cols2.size();
                cols2.push_back(nc);
            }
            a.col = wide_slot[col];
        }
        rest.push_back(a);
        rest_outs.push_back(outs[i]);
        rest_at.push_back(i);
    }
    if (long_windows) *long_windows = 0;
    if (kernel_ms) *kernel_ms = 0;
    WindowRows rows;
    if (!rest.empty()) {
        const AggCall call2 = {cols2.data(), (int32_t)cols2.size(), call.ts_col, call.plan, call.inclusive, call.strict, call.check_plan};
        BG_TRY(run_aggregate(c, call2, rest.data(), (int32_t)rest.size(), rest_outs.data(), long_windows, kernel_ms, &rows));
        for (size_t j = 0; j < rest_at.size(); j++) outs[rest_at[j]] = rest_outs[j];
    }
    if (!bool_at.empty()) {
        BG_TRY(run_bools(c, call, aggs, bool_at, outs, &rows, &ms_bool));
        if (rest.empty()) c->last_kernel_name = "bool_windows_kernel";
    }
    // bowgpu_agg_info.kernel_ms / bowgpu_last_kernel_ms: the other reducers' bracket + the widening + the Boolean pass
    const double total = (kernel_ms ? *kernel_ms : rest.empty() ? 0.0 : c->last_kernel_ms) + ms_bool;
    if (kernel_ms) *kernel_ms = total;
    c->last_kernel_ms = total;
    return 0;
}

// An unsharded Aggregate call: the streaming reducers in batches that one launch of the tile kernels takes (at most kMaxAggs
// outputs over at most kMaxCols column passes - the reference has no such limits, aggregation.go:190-238 simply loops), then the
// Mode outputs.
static int run_aggregate(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, int64_t *long_windows, double *kernel_ms,
                         WindowRows *rows) {
    const bowgpu_col &tsc = call.cols[call.ts_col];
    const int64_t W = call.plan.W;
    if (tsc.validity && tsc.null_count != 0 && tsc.length > 0) {
        DevCol dts;   // (values + validity on the device; counts the nulls when the caller did not)
        BG_TRY(devcol_prepare(c, &tsc, &dts, true, true));
        if (dts.null_count > 0) return run_aggregate_null_ts(c, call, aggs, naggs, outs, dts, long_windows, kernel_ms);
    }
    if (any_bool_agg(call.cols, aggs, naggs)) return run_aggregate_bool(c, call, aggs, naggs, outs, long_windows, kernel_ms);
    if (long_windows) *long_windows = 0;
    if (kernel_ms) *kernel_ms = 0;
    // greedy batches in output order; ColSlots counts the column passes as job_build will
    std::vector<std::vector<int>> batches;
    {
        std::vector<int> cur;
        ColSlots slots(call.ncols);
        auto flush = [&]() {
            if (!cur.empty()) batches.push_back(cur);
            cur.clear();
            slots.clear();
        };
        for (int i = 0; i < naggs; i++) {
            if (aggs[i].kind == BOWGPU_AGG_MODE) continue;
            const bool reads = kind_reads_values(aggs[i].kind);
            for (int attempt = 0; attempt < 2; attempt++) {
                bool fits = (int)cur.size() < kMaxAggs;
                if (fits && reads && slots.find(aggs[i], 4) < 0) fits = slots.count() < kMaxCols;
                if (!fits) { flush(); continue; }  // (an empty batch always takes one reducer)
                if (reads) slots.take(aggs[i], 4);
                cur.push_back(i);
                break;
            }
        }
        flush();
    }
    for (const std::vector<int> &at : batches) {
        if ((int)at.size() == naggs) {  // the usual case: the whole call in one launch
            AggJob job;
            BG_TRY(job_build(c, call, aggs, naggs, outs, 0, W, true, &job));
            BG_TRY(job_run(c, &job, long_windows, kernel_ms, true, true));
            continue;
        }
        std::vector<bowgpu_agg> part;
        std::vector<bowgpu_out> part_outs;
        for (int i : at) { part.push_back(aggs[i]); part_outs.push_back(outs[i]); }
        int64_t lw = 0;
        double ms = 0;
        AggJob job;
        BG_TRY(job_build(c, call, part.data(), (int32_t)part.size(), part_outs.data(), 0, W, true, &job));
        BG_TRY(job_run(c, &job, &lw, &ms, true, true));
        for (size_t j = 0; j < at.size(); j++) outs[at[j]] = part_outs[j];
        if (long_windows && lw > *long_windows) *long_windows = lw;   // (the same windows in every batch)
        if (kernel_ms) *kernel_ms += ms;
    }
    if (need_mask(aggs, naggs) & kNeedMode) return run_modes(c, call, aggs, naggs, outs, long_windows, rows);
    return 0;
}

int sharded_validate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_agg *aggs, int32_t naggs) {
    // plan_make's order (newIntervalRolling first), then validateAggregation's, then the protocol's own limits
    const int t = cols[ts_col].type;
    if (t != BOWGPU_INT64)
        return fail(BOWGPU_ERR_TS_TYPE, "impossible to create a new intervalRolling on column of type %s", arrow_type_name(t));
    int64_t off;
    BG_TRY(enforce_interval_and_offset(interval, 0, &off));
    int inclusive = 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    return shard_check(cols, aggs, naggs);
}

int ts_null_rows(Ctx *c, const bowgpu_col *ts, int64_t *nulls) {
    *nulls = 0;
    if (!ts->validity || ts->null_count == 0 || ts->length == 0) return 0;
    if (ts->null_count > 0) { *nulls = ts->null_count; return 0; }
    DevCol probe;
    BG_TRY(devcol_prepare(c, ts, &probe, false, true));
    *nulls = probe.null_count;
    BG_HIP(hipStreamSynchronize(c->stream));   // (before the probe's blocks go back to the cache)
    return 0;
}

int ts_contract(Ctx *c, const bowgpu_col *tsc) {
    if (tsc->validity && tsc->null_count != 0) {
        DevCol probe;
        BG_TRY(devcol_prepare(c, tsc, &probe, false, true));
        if (probe.null_count > 0) return fail(BOWGPU_ERR_TS_NULLS, "interval column has %lld nulls: outside the device path", (long long)probe.null_count);
    }
    return 0;
}

int ts_device(Ctx *c, const bowgpu_col *tsc, DevCol *dts) {
    bowgpu_col t = *tsc;
    t.validity = nullptr;
    t.null_count = 0;
    return devcol_prepare(c, &t, dts, true, false);
}

}  // namespace bowgpu

using namespace bowgpu;

extern "C" {

int bowgpu_enforce_interval_and_offset(int64_t interval, int64_t offset, int64_t *offset_out) {
    return enforce_interval_and_offset(interval, offset, offset_out);
}

int bowgpu_plan_windows(const bowgpu_col *ts, int64_t interval, int64_t offset, int64_t *s0, int64_t *num_windows) {
    if (!ts || !s0 || !num_windows) return fail(BOWGPU_ERR_ARG, "null argument");
    // O(1) host arithmetic on ts[0] and the last valid ts; the GPU is touched only to fetch
    // those scalars when the column lives in HBM (plan_make acquires the context lazily).
    Plan p;
    BG_TRY(plan_make(nullptr, ts, interval, offset, &p));
    *s0 = p.s0;
    *num_windows = p.W;
    return 0;
}

// the plan materialised: every window's first row, slice and inclusive flag (the iterator)
int bowgpu_window_bounds(const bowgpu_col *ts, int64_t interval, const bowgpu_options *opts, int64_t *first_index,
                         int64_t *slice_begin, int64_t *slice_end, uint8_t *is_inclusive, int32_t residency) {
    if (!ts) return fail(BOWGPU_ERR_ARG, "null argument");
    const bowgpu_options o = options_or(opts);
    Plan plan;
    BG_TRY(plan_make(nullptr, ts, interval, o.offset, &plan));
    if (plan.W == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_TRY(ts_contract(c, ts));
    DevCol dts;
    BG_TRY(ts_device(c, ts, &dts));
    const int64_t n = ts->length, W = plan.W;
    DevBuf first_idx, d_fi, d_sb, d_se, d_in;
    BG_TRY(first_idx.alloc((size_t)(W + 1) * 8));
    uint32_t *status;
    BG_TRY(scratch_at(c, kScrStatus, &status));
    BG_HIP(hipMemsetAsync(status, 0, kStatusHeadBytes, c->stream));
    BG_TRY(launch_window_first_rows(c, reinterpret_cast<const int64_t *>(dts.values), n, plan, reinterpret_cast<int64_t *>(first_idx.p), status));
    const bool dev = residency == BOWGPU_DEVICE;
    int64_t *pfi = first_index, *psb = slice_begin, *pse = slice_end;
    uint8_t *pin = is_inclusive;
    if (!dev) {
        if (first_index) { BG_TRY(d_fi.alloc((size_t)W * 8)); pfi = reinterpret_cast<int64_t *>(d_fi.p); }
        if (slice_begin) { BG_TRY(d_sb.alloc((size_t)W * 8)); psb = reinterpret_cast<int64_t *>(d_sb.p); }
        if (slice_end) { BG_TRY(d_se.alloc((size_t)W * 8)); pse = reinterpret_cast<int64_t *>(d_se.p); }
        if (is_inclusive) { BG_TRY(d_in.alloc((size_t)W)); pin = reinterpret_cast<uint8_t *>(d_in.p); }
    }
    BG_TRY(launch_window_bounds(c, reinterpret_cast<const int64_t *>(dts.values), n, plan, o.inclusive ? 1 : 0,
                                plan.s0 > plan.first_ts ? 1 : 0, reinterpret_cast<const int64_t *>(first_idx.p), pfi, psb, pse, pin));
    uint32_t hstat[4] = {0, 0, 0, 0};
    BG_HIP(hipMemcpyAsync(hstat, status, 16, hipMemcpyDeviceToHost, c->stream));
    if (!dev) {
        if (first_index) BG_TRY(copy_d2h(c, first_index, pfi, (size_t)W * 8));
        if (slice_begin) BG_TRY(copy_d2h(c, slice_begin, psb, (size_t)W * 8));
        if (slice_end) BG_TRY(copy_d2h(c, slice_end, pse, (size_t)W * 8));
        if (is_inclusive) BG_TRY(copy_d2h(c, is_inclusive, pin, (size_t)W));
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    if (hstat[0]) return fail_ts_unsorted();
    return 0;
}

static int aggregate_with_plan(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, const bowgpu_options *opts, bool check_plan,
                               const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, bowgpu_agg_info *info) {
    const int opt_inclusive = opts ? opts->inclusive : 0;
    const bool strict = strict_wanted(opts);
    int inclusive = opt_inclusive ? 1 : 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    if (!outs) return fail(BOWGPU_ERR_ARG, "no output columns");
    {   // bowgpu_set_devices: the call cut into row ranges over the listed devices (fan_call.cpp); not taken -> the one-device path below
        bool fanned = false;
        BG_TRY(multi_aggregate(cols, ncols, ts_col, plan, opt_inclusive, strict, aggs, naggs, outs, info, &fanned));
        if (fanned) return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    c->last_slow_rows = 0;
    int64_t n_long = 0;
    double ms = 0;
    static const bool prof = [] { const char *e = getenv("BOWGPU_CALL_PROFILE"); return e && e[0] == '1'; }();
    const double t_in = prof ? now_us() : 0;
    const AggCall call = {cols, ncols, ts_col, plan, inclusive, strict, check_plan};
    BG_TRY(run_aggregate(c, call, aggs, naggs, outs, &n_long, &ms));
    if (prof) {
        static thread_local double acc[3] = {0, 0, 0};
        static thread_local int calls = 0;
        const double t_out = now_us();
        // (a route with no single synchronisation point of its own - the long-window forms - leaves the stamps of an EARLIER call behind:
        // such a call is booked whole under "enqueue" instead of producing negative parts)
        if (c->prof_sync_begin >= t_in) { acc[0] += c->prof_sync_begin - t_in; acc[1] += c->prof_sync_end - c->prof_sync_begin; acc[2] += t_out - c->prof_sync_end; }
        else acc[0] += t_out - t_in;
        if (++calls == 200) {
            fprintf(stderr, "bowgpu call profile (200 calls): enqueue %.1f us, synchronise %.1f us, after %.1f us\n", acc[0] / 200, acc[1] / 200, acc[2] / 200);
            acc[0] = acc[1] = acc[2] = 0; calls = 0;
        }
    }
    if (info) {
        info->s0 = plan.s0;
        info->num_windows = plan.W;
        info->new_interval_col = nic;
        info->inclusive = inclusive;
        info->long_windows = n_long;
        info->kernel_ms = ms;
    }
    return 0;
}

int bowgpu_rolling_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                             const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs,
                             bowgpu_out *outs, bowgpu_agg_info *info) {
    if (!cols || ncols <= 0) return fail(BOWGPU_ERR_ARG, "no columns");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    const bowgpu_options o = options_or(opts);
    // reference order: the Rolling exists first (newIntervalRolling errors), then Aggregate validates
    Plan plan;
    BG_TRY(plan_make(nullptr, &cols[ts_col], interval, o.offset, &plan));
    return aggregate_with_plan(cols, ncols, ts_col, plan, &o, false, aggs, naggs, outs, info);
}

/* Rolling.Interpolate(interps...) followed by Rolling.Aggregate(aggs...) on the Rolling it returns (reference
 * rolling/interpolation.go:30-69, rolling/aggregation.go:123-145), without handing the interpolated frame back: one pass over the
 * rows where the shape allows it (rolling_fused.hip), else the two calls through device temporaries - the same bits either way. */
int bowgpu_rolling_interpolate_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                                         const bowgpu_interp *interps, int32_t ninterps, const bowgpu_agg *aggs, int32_t naggs,
                                         bowgpu_out *outs, bowgpu_agg_info *info) {
    if (!cols || ncols <= 0) return fail(BOWGPU_ERR_ARG, "no columns");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    if (!interps) return fail(BOWGPU_ERR_ARG, "null argument");
    const bowgpu_options o = options_or(opts);
    // the reference's order: the Rolling exists first (newIntervalRolling), Interpolate validates its interpolators, then Aggregate
    // validates its aggregators against the interpolated Bow - which has the input's columns and types (interpolation.go:139-155)
    Plan plan;
    BG_TRY(plan_make(nullptr, &cols[ts_col], interval, o.offset, &plan));
    BG_TRY(interp_validate(cols, ncols, ts_col, &o, interps, ninterps));
    int inclusive = o.inclusive ? 1 : 0, nic = -1;
    BG_TRY(validate_aggs(cols, ncols, ts_col, aggs, naggs, &inclusive, &nic));
    for (int i = 0; i < naggs; i++)
        if (cols[aggs[i].col].type == BOWGPU_BOOLEAN)
            return fail(BOWGPU_ERR_UNSUPPORTED, "aggregation %d: Interpolate does not take a Boolean column on the device, so neither does Interpolate + Aggregate", i);
    if (!outs) return fail(BOWGPU_ERR_ARG, "no output columns");
    {   // bowgpu_set_devices: every rank interpolates and aggregates its own row range (fan_call.cpp); not taken -> one device, below
        bool fanned = false;
        BG_TRY(multi_interpolate_aggregate(cols, ncols, ts_col, plan, o.inclusive, strict_wanted(&o), interps, ninterps, aggs, naggs, outs, info, &fanned));
        if (fanned) return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    c->last_slow_rows = 0;   // (bowgpu_last_call_slow_rows speaks of THIS call; the two-call form below resets it again in its own entry points)
    bool done = false;
    double ms = 0;
    BG_TRY(fused_try(c, cols, ncols, ts_col, plan, o, inclusive, interps, aggs, naggs, outs, &ms, &done));
    if (done) {
        if (info) {
            info->s0 = plan.s0; info->num_windows = plan.W; info->new_interval_col = nic; info->inclusive = inclusive;
            info->long_windows = 0; info->kernel_ms = ms;
        }
        return 0;
    }
    // the two calls.  The interpolated frame lives in device temporaries and is aggregated where it lies.
    int64_t n_out = 0;
    BG_TRY(bowgpu_rolling_interpolate_count(cols, ncols, ts_col, interval, &o, interps, ninterps, &n_out));
    DevFrame mid;
    std::vector<bowgpu_col> icols(ncols);
    BG_TRY(mid.alloc(c, ncols, n_out, false));
    if (n_out > 0) BG_TRY(bowgpu_rolling_interpolate_fill(cols, ncols, ts_col, interval, &o, interps, ninterps, mid.outs.data()));
    mid.as_cols(cols, n_out, icols.data());
    const int rc = bowgpu_rolling_aggregate(icols.data(), ncols, ts_col, interval, &o, aggs, naggs, outs, info);
    // (the temporaries go back to the block cache: every entry point above has synchronised the stream)
    return rc;
}

int bowgpu_plan_windows_ex(const bowgpu_col *ts, int64_t interval, int64_t offset, bowgpu_plan *out) {
    if (!ts || !out) return fail(BOWGPU_ERR_ARG, "null argument");
    Plan p;
    BG_TRY(plan_make(nullptr, ts, interval, offset, &p));
    out->s0 = p.s0; out->num_windows = p.W; out->first_ts = p.first_ts; out->last_ts = p.last_ts;
    out->interval = p.interval; out->offset = p.offset; out->nrows = ts->length;
    return 0;
}

int bowgpu_rolling_aggregate_planned(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_plan *pl,
                                     const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs,
                                     bowgpu_out *outs, bowgpu_agg_info *info) {
    if (!cols || ncols <= 0 || !pl) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    const bowgpu_col *ts = &cols[ts_col];
    if (ts->type != BOWGPU_INT64) return fail(BOWGPU_ERR_TS_TYPE, "impossible to create a new intervalRolling on column of type float64");
    if (pl->interval <= 0) return fail(BOWGPU_ERR_INTERVAL, "strictly positive interval required");
    if (pl->nrows != ts->length || pl->offset < 0 || pl->offset >= pl->interval || pl->num_windows < 0)
        return fail(BOWGPU_ERR_ARG, "the plan was not made for this interval column");
    // the plan against itself (host arithmetic) ... and against the column: the pass compares the two timestamps it was made from with
    // the column's first and last row (one tiny launch in front of the tile kernel, no round trip) - a plan made for another
    // column of the same length, or for this buffer before it was refilled, is BOWGPU_ERR_ARG instead of silently wrong routes
    if (ts->length > 0) {
        const int64_t s0 = first_window_start(pl->first_ts, pl->interval, pl->offset);
        const int64_t W = s0 > pl->last_ts ? 0 : (int64_t)(((uint64_t)pl->last_ts - (uint64_t)s0) / (uint64_t)pl->interval) + 1;
        if (pl->last_ts < pl->first_ts || s0 != pl->s0 || W != pl->num_windows)
            return fail(BOWGPU_ERR_ARG, "the plan is not consistent (s0 / num_windows do not follow from its first / last timestamp)");
    }
    Plan plan;
    plan.interval = pl->interval; plan.offset = pl->offset; plan.s0 = pl->s0; plan.W = pl->num_windows;
    plan.first_ts = pl->first_ts; plan.last_ts = pl->last_ts;
    plan.magic = magic_make((uint64_t)pl->interval);
    return aggregate_with_plan(cols, ncols, ts_col, plan, opts, ts->length > 0, aggs, naggs, outs, info);
}

}  // extern "C"
