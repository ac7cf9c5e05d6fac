// interpolate_api.cpp - Rolling.Interpolate (reference rolling/interpolation.go): validation, pass 1 and what it leaves for the fill that
// follows a count, the fill in its attempts, and the bowgpu_rolling_interpolate_* / bowgpu_shard_interp* entry points.  Host code here only
// validates, prepares residency and orchestrates the kernels of interpolate.hip and interp_fill.hip; no column data is reduced on the CPU.
#include <string.h>

#include <vector>

#include "interp_host.h"

namespace bowgpu {

static bool interp_type_ok(int kind, int t) {
    switch (kind) {
    case BOWGPU_INTERP_WINDOW_START: return t == BOWGPU_INT64;                         // interpolation/windowstart.go:9
    case BOWGPU_INTERP_LINEAR: return t == BOWGPU_INT64 || t == BOWGPU_FLOAT64;        // interpolation/linear.go:11
    case BOWGPU_INTERP_STEP_PREVIOUS:                                                  // stepprevious.go:10 (+ Boolean, String)
    case BOWGPU_INTERP_NONE: return t == BOWGPU_INT64 || t == BOWGPU_FLOAT64 || t == BOWGPU_BOOLEAN || (kind == BOWGPU_INTERP_STEP_PREVIOUS && t == BOWGPU_STRING);
    case BOWGPU_INTERP_CONST: return t == BOWGPU_INT64 || t == BOWGPU_FLOAT64;
    default: return false;
    }
}

int interp_validate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_options *o, const bowgpu_interp *interps, int32_t ninterps) {
    // Interpolate + validateInterpolation: reference rolling/interpolation.go:30-96
    if (ninterps <= 0) return fail(BOWGPU_ERR_ARG, "at least one column interpolation is required");
    int nic = -1;
    for (int i = 0; i < ninterps; i++) {
        if (interps[i].col < 0 || interps[i].col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "interpolation %d: no column with index %d", i, interps[i].col);
        const int t = cols[interps[i].col].type;
        if (!interp_type_ok(interps[i].kind, t)) {
            const char *acc = interps[i].kind == BOWGPU_INTERP_WINDOW_START ? "[int64]"
                              : interps[i].kind == BOWGPU_INTERP_LINEAR ? "[int64 float64]"
                              : interps[i].kind == BOWGPU_INTERP_STEP_PREVIOUS ? "[int64 float64 bool utf8]"
                              : interps[i].kind == BOWGPU_INTERP_NONE ? "[int64 float64 bool]" : "[int64 float64]";
            return fail(BOWGPU_ERR_TYPE, "accepts types %s, got type %s", acc, arrow_type_name(t));
        }
        if (interps[i].col == ts_col) nic = i;
    }
    if (nic == -1) return fail(BOWGPU_ERR_KEEP_INTERVAL, "must keep interval column");
    // AppendBows(startBow, window.Bow) needs one schema (bowappend.go:11-13): the interpolators must list the columns in order
    if (ninterps != ncols) return fail(BOWGPU_ERR_UNSUPPORTED, "interpolators must cover every column of the Bow, in order (bowappend.go:11-13)");
    for (int i = 0; i < ninterps; i++) {
        if (interps[i].col != i) return fail(BOWGPU_ERR_UNSUPPORTED, "interpolators must cover every column of the Bow, in order (bowappend.go:11-13)");
        const int t = cols[i].type;
        if (t != BOWGPU_INT64 && t != BOWGPU_FLOAT64) return fail(BOWGPU_ERR_UNSUPPORTED, "column type %s is outside the device path", arrow_type_name(t));
    }
    return 0;
}

using InterpFound = Ctx::InterpCache::Found;

struct InterpJob {
    InterpFound found;   // what pass 1 found (common.h): this call's own, or the preceding _count's in one assignment
    DevCol dts;
    std::vector<DevCol> dcols;
    void *tile_local = nullptr, *super_before = nullptr, *super_sum = nullptr;  // context pool (no hipMalloc / hipFree per call)
    int has_left = 0; // sharded Interpolate: rows exist to the left, the last of them at left_ts, in window found.wbase - 1
    int64_t left_ts = 0;
    bool from_cache = false;   // pass 1 was not run by this call: its results are the preceding _count's
};

// the plan's pieces among the findings, and the Plan they came from again (interval and its magic: the call's argument)
static void found_take_plan(InterpFound *f, const Plan &pl) {
    f->s0 = pl.s0; f->W = pl.W; f->first_ts = pl.first_ts; f->last_ts = pl.last_ts; f->offset_norm = pl.offset;
}
static Plan found_plan(const InterpFound &f, int64_t interval) {
    Plan pl;
    pl.interval = interval; pl.offset = f.offset_norm; pl.s0 = f.s0; pl.W = f.W;
    pl.first_ts = f.first_ts; pl.last_ts = f.last_ts; pl.magic = magic_make((uint64_t)interval);
    return pl;
}

// pass 1 of interpolate.hip: exact heads per tile, their exclusive scan, M = synthetic rows
// shard: global_s0 + edge of a row-range shard (nullptr: the whole frame)
static bool interp_cache_hit(Ctx *c, const bowgpu_col *ts, int64_t interval, int64_t raw_offset, int inclusive, const int64_t *global_s0,
                             const bowgpu_interp_edge *edge) {
    const Ctx::InterpCache &k = c->interp_cache;
    if (!k.valid || ts->residency != BOWGPU_DEVICE) return false;   // (a host column is staged into a fresh device copy per call)
    if (k.ts_values != ts->values || k.ts_offset != ts->offset || k.n != ts->length || k.interval != interval || k.raw_offset != raw_offset) return false;
    if (k.sharded != (global_s0 != nullptr) || k.found.inclusive != (inclusive ? 1 : 0)) return false;
    if (global_s0 && (k.global_s0 != *global_s0 || k.has_left != ((edge && edge->has_left) ? 1 : 0) || (k.has_left && k.left_ts != edge->left_last_ts))) return false;
    if (k.epoch != device_write_epoch()) return false;   // something was written to / freed from device memory through the library since the count
    return k.gen == c->pool_gen[kPoolInterp + 1] && c->pool[kPoolInterp + 1] != nullptr && k.gen0 == c->pool_gen[kPoolInterp + 0] && c->pool[kPoolInterp + 0] != nullptr;
}

static int interp_prepare(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                          const bowgpu_options *o, InterpJob *job, const int64_t *global_s0 = nullptr, const bowgpu_interp_edge *edge = nullptr,
                          bool use_cache = false, const Plan *probe = nullptr) {
    // The _fill call right after _count on the same device-resident, unchanged interval column (Bows are immutable in the
    // reference; include/bowgpu.h, "Rolling.Interpolate", states the contract): pass 1's prefix is still in the context pool.  A
    // write or free THROUGH the library in between drops it (device_write_epoch); the fill kernel checks the output count it
    // arrives at against the cached one and the call fails with BOWGPU_ERR_ARG when they differ (status[6])
    InterpFound &f = job->found;
    if (use_cache && interp_cache_hit(c, &cols[ts_col], interval, o->offset, o->inclusive, global_s0, edge)) {
        const Ctx::InterpCache &k = c->interp_cache;
        for (int i = 0; i < ncols; i++)
            if (cols[i].length != k.n) return fail(BOWGPU_ERR_ARG, "column %d has a different length", i);
        f = k.found; job->has_left = k.has_left; job->left_ts = k.left_ts;
        job->tile_local = c->pool[kPoolInterp + 0];
        job->super_before = c->pool[kPoolInterp + 1];
        job->from_cache = true;
        BG_TRY(ts_device(c, &cols[ts_col], &job->dts));
        c->interp_cache.valid = false;   // one use: the outputs of this fill may be what the next call reads
        return 0;
    }
    c->interp_cache.valid = false;
    Plan pl;
    if (probe) pl = *probe;   // (the caller's constructor checks already fetched the column's first and last timestamp: one round trip, not two)
    else BG_TRY(plan_make(c, &cols[ts_col], interval, o->offset, &pl));
    if (global_s0) {
        // a shard: windows are counted from the frame's s0; the shard accounts for the windows after its left neighbours' last one
        pl.s0 = *global_s0;
        if (cols[ts_col].length > 0) {
            // rows below the first window start (Go's truncating division on a negative first timestamp: rolling.go:96-99) ride in window 0
            // or belong to no window at all - which of the two depends on the first row AT OR ABOVE s0 (interp_quirk_kernel).  They are the
            // frame's first rows: the frame's first shard serves them as the unsharded call does when that row is its own; the corner that
            // is left - a first shard of nothing but such rows, fewer than one interval's worth of time - is declined.
            if (pl.first_ts < pl.s0 && ((edge && edge->has_left) || pl.last_ts < pl.s0))
                return fail(BOWGPU_ERR_UNSUPPORTED, "sharded interpolate: a shard of nothing but rows below the first window start is outside the sharded path");
            const int64_t wl = (int64_t)(((uint64_t)pl.last_ts - (uint64_t)pl.s0) / (uint64_t)interval);
            job->has_left = edge && edge->has_left ? 1 : 0;
            if (job->has_left) {
                if (edge->left_last_ts < pl.s0 || edge->left_last_ts > pl.first_ts) return fail(BOWGPU_ERR_ARG, "sharded interpolate: the left neighbour's last timestamp does not precede this shard");
                job->left_ts = edge->left_last_ts;
                f.wbase = (int64_t)(((uint64_t)edge->left_last_ts - (uint64_t)pl.s0) / (uint64_t)interval) + 1;
            }
            pl.W = wl + 1 - f.wbase;  // windows this shard accounts for
        }
    }
    found_take_plan(&f, pl);
    f.inclusive = o->inclusive ? 1 : 0;
    const int64_t n = cols[ts_col].length, W = pl.W;
    for (int i = 0; i < ncols; i++)
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "column %d has a different length", i);
    f.M = 0;
    if (n == 0) return 0;
    BG_TRY(ts_contract(c, &cols[ts_col]));
    BG_TRY(ts_device(c, &cols[ts_col], &job->dts));
    if (W == 0 && !global_s0) { f.M = -n; return 0; }  // no window at all (every row lies below s0): the concatenation of zero window bows is empty
    f.kq = -1;
    if (pl.s0 <= -1 && (uint64_t)(-1 - pl.s0) % (uint64_t)pl.interval == 0) {
        // (a shard accounts for windows wbase .. wbase + W - 1 of the frame; the one that starts at -1 concerns the shard that accounts for it:
        // its rows, if it has any, can only be that shard's own - the left neighbours end in an earlier window, and when this shard ends
        // in a later one nothing of the window lies to its right)
        const int64_t k = (int64_t)((uint64_t)(-1 - pl.s0) / (uint64_t)pl.interval);
        if (k >= f.wbase && k - f.wbase < W) f.kq = k;
    }
    const int64_t ntiles = 2 * interp_tiles(n);   // exact heads are counted per 256 rows: two entries per tile of the count kernel
    const int64_t nsuper = interp_supers(n);
    BG_TRY(ctx_pool(c, kPoolInterp + 0, (size_t)ntiles * 4 + 16, &job->tile_local));
    BG_TRY(ctx_pool(c, kPoolInterp + 1, (size_t)(nsuper + 1) * 8, &job->super_before));
    BG_TRY(ctx_pool(c, kPoolInterp + 2, (size_t)nsuper * 4 + 16, &job->super_sum));
    uint32_t *status;
    BG_TRY(scratch_at(c, kScrStatus, &status));
    BG_HIP(hipMemsetAsync(status, 0, kStatusHeadBytes, c->stream));
    const int64_t *ts = reinterpret_cast<const int64_t *>(job->dts.values);
    int64_t *d_total = reinterpret_cast<int64_t *>(status + 4);
    int64_t *hback;   // the pass' findings arrive in the registered block by the scan kernel's own stores
    BG_TRY(registered_at(c, kRegInterpCount, &hback));
    BG_TRY(launch_interp_count(c, ts, n, pl, f.kq, job->has_left, job->left_ts, reinterpret_cast<int32_t *>(job->tile_local),
                               reinterpret_cast<int32_t *>(job->super_sum), reinterpret_cast<int64_t *>(job->super_before), d_total, status, hback));
    BG_HIP(hipStreamSynchronize(c->stream));
    const uint32_t hstat[4] = {(uint32_t)(uint64_t)hback[1], (uint32_t)((uint64_t)hback[1] >> 32), (uint32_t)(uint64_t)hback[2], (uint32_t)((uint64_t)hback[2] >> 32)};
    const int64_t total = hback[0];
    if (hstat[0]) return fail_ts_unsorted();
    f.drop = (int64_t)(((uint64_t)hstat[3] << 32) | hstat[2]);
    f.kq_empty = hstat[1] ? 1 : 0;
    if (o->inclusive) {
        // Inclusive windows (rolling.go:201-209 + interpolation.go:98-116): a row on a window's end is also the last row of that
        // window's bow, so it appears twice in the concatenation - every window then contributes exactly one row in front of
        // its first row (a synthetic row, or that copy), except window 0 when row 0 sits on its start: n + W - e0 rows.  The
        // whole-trip wave kernel takes them; its preconditions (interp_fast32, no dropped rows, no -1 sentinel window) bound the shape.
        // A shard (global_s0): the same statement over the windows the shard accounts for (those behind its left neighbours' last
        // one) - the copy of a row that sits on its window's start travels with the row itself, and only the FRAME's first row can
        // be the exact row 0 that gets nothing in front.
        if (!(interp_fast32(pl, f.kq) || interp_wide32(pl, f.kq)) || f.drop != 0)
            return fail(BOWGPU_ERR_UNSUPPORTED, "Interpolate on inclusive windows: rows below s0, intervals of 2^31 and more or timestamps beyond 2^53 are outside the device path");
        f.e0 = (!job->has_left && pl.first_ts == pl.s0) ? 1 : 0;
        f.M = W - f.e0;
    } else
    f.M = W - total - ((f.kq >= 0 && hstat[1]) ? 1 : 0) - f.drop;  // rows added (synthetic) minus rows dropped
    {
        Ctx::InterpCache &k = c->interp_cache;
        const bowgpu_col *tsc = &cols[ts_col];
        k.ts_values = tsc->values; k.ts_offset = tsc->offset; k.n = n; k.interval = interval; k.raw_offset = o->offset;
        k.sharded = global_s0 != nullptr; k.global_s0 = global_s0 ? *global_s0 : 0;
        k.has_left = job->has_left; k.left_ts = job->left_ts;
        k.gen = c->pool_gen[kPoolInterp + 1];
        k.gen0 = c->pool_gen[kPoolInterp + 0];
        k.epoch = device_write_epoch();
        k.found = f;
        k.valid = tsc->residency == BOWGPU_DEVICE;
    }
    return 0;
}

// Rolling.Interpolate on INCLUSIVE windows as ONE pass over the rows (a _fill that does not follow its _count): every window then
// contributes exactly one row in front of its first - n_out = n + W - e0, and a trip's output position depends on nothing a count
// pass would tell - so there is no count pass; the fill kernel checks the order of the interval column itself.  (Exclusive windows
// need the number of rows sitting exactly on a window start before each trip.  A decoupled look-back inside the fill kernel was
// built and measured in round 4: 1.67 ms against 1.12 ms for count pass + fill at 1e8 rows - an uncached word per trip each way
// costs more than the 0.16 ms count pass it replaces; not kept.)  Taken for the shapes interp_wave3_kernel serves on its own: the
// whole frame (no shard), no -1 sentinel window, no rows below s0.  *applies = false: the two-pass path (interp_prepare).
static int interp_onepass_prepare(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *o,
                                  InterpJob *job, bool *applies, const Plan *probe = nullptr) {
    *applies = false;
    if (!o->inclusive) return 0;
    const int64_t n = cols[ts_col].length;
    if (n <= 0) return 0;
    for (int i = 0; i < ncols; i++)
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "column %d has a different length", i);
    Plan pl;
    if (probe) pl = *probe;
    else BG_TRY(plan_make(c, &cols[ts_col], interval, o->offset, &pl));
    if (pl.W <= 0 || pl.first_ts < pl.s0 || pl.s0 <= -1) return 0;   // (s0 <= -1: a window may start at -1 - the reference's sentinel)
    if (!(interp_fast32(pl, -1) || interp_wide32(pl, -1))) return 0;
    BG_TRY(ts_contract(c, &cols[ts_col]));
    BG_TRY(ts_device(c, &cols[ts_col], &job->dts));
    InterpFound &f = job->found;
    found_take_plan(&f, pl);
    f.kq = -1; f.drop = 0; f.kq_empty = 0; job->has_left = 0; f.wbase = 0;
    f.inclusive = 1;
    f.e0 = (o->inclusive && pl.first_ts == pl.s0) ? 1 : 0;
    f.M = pl.W - f.e0;
    c->interp_cache.valid = false;
    *applies = true;
    return 0;
}

int interp_count_impl(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                      const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out, const int64_t *global_s0, const bowgpu_interp_edge *edge) {
    if (!cols || ncols <= 0 || !n_out) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    if (edge && ncols > kMaxCols) return fail(BOWGPU_ERR_UNSUPPORTED, "sharded Interpolate: at most %d columns (bowgpu_interp_edge)", kMaxCols);
    const bowgpu_options o = options_or(opts);
    Plan probe;
    BG_TRY(plan_make(nullptr, &cols[ts_col], interval, o.offset, &probe));  // ctor errors first (rolling.go:69-112)
    BG_TRY(interp_validate(cols, ncols, ts_col, &o, interps, ninterps));
    if (cols[ts_col].length == 0) { *n_out = 0; return 0; }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    InterpJob job;
    BG_TRY(interp_prepare(c, cols, ncols, ts_col, interval, &o, &job, global_s0, edge, false, &probe));
    *n_out = cols[ts_col].length + job.found.M;
    return 0;
}

// Pass 1's part of the kernel parameters: the two prefix blocks and what InterpFound says about the windows.  From the call's own job
// first, and again from a fresh pass 1 before the workgroup kernel runs.  Everything else of InterpParams comes from the call's
// arguments (interp_fill_impl) and is the same for both.
static void params_take_pass1(InterpParams *P, const InterpJob &job) {
    const InterpFound &f = job.found;
    P->tile_local = reinterpret_cast<const int32_t *>(job.tile_local);
    P->super_before = reinterpret_cast<const int64_t *>(job.super_before);
    P->kq = f.kq; P->kq_empty = f.kq_empty; P->drop = f.drop; P->e0 = f.e0;
    P->s0 = f.s0; P->W = f.W;
}

// an interpolator's Options.PrevRow and constant, as InterpCol lays them out (interp_null_ts.cpp has PatchInterps' form)
static void interp_col_take(InterpCol *ic, const bowgpu_interp &ip) {
    ic->const_value = ip.const_value;
    ic->has_prev = ip.has_prev_row; ic->prev_t_valid = ip.prev_t_valid; ic->prev_v_valid = ip.prev_v_valid;
    ic->prev_t = ip.prev_t; ic->prev_v = ip.prev_v; ic->prev_v_i64 = ip.prev_v_i64;
}

// One run of the fill kernels over every column of a call: what it reads, and what it leaves for interp_fill_impl's decisions
struct InterpRun {
    Ctx *c;
    InterpParams &P;                  // the call's parameter block; a run sets its own members (allow_wave2, in_place ...) and each batch's columns
    const std::vector<DevCol> &dcols; // the job's columns on the device
    const bowgpu_col *cols; const bowgpu_interp *interps; const bowgpu_interp_edge *edge;
    bowgpu_out *outs; const std::vector<DevOut> &douts;
    int32_t ncols; int64_t n, n_out;
    bool can_place;                   // the outputs' bitmaps can be written in place
    uint32_t *trip_valid; unsigned long long *dcnt;
    uint32_t hstat[8];                // produced: the status words behind the last batch
    std::vector<uint64_t> hcnt;       // produced: valid outputs per column
};

// One batch of at most kMaxCols columns from column b0 on.  In place: the kernel + the edge fix (which also sums the counts);
// through working copies: ONE launch zeroes the batch's bitmaps (and, first batch, the status words), the kernel(s), ONE launch
// counts the valid bits and copies the bitmaps into the caller's buffers.  hs / hc: the registered status words and counts.
// (with_index: the neighbour index of each nullable column under Linear / StepPrevious - three small launches per column.
// interp_wave3_kernel finds a synthetic row's neighbour points by a bounded walk and says so when one lies further away
// (status[7]): the index is built for the workgroup kernel and for that repeat only.)
static int interp_run_batch(InterpRun &R, int b0, bool place, bool with_index, uint32_t *hs, unsigned long long *hc) {
    Ctx *c = R.c;
    InterpParams &P = R.P;
    const int nb = R.ncols - b0 < kMaxCols ? R.ncols - b0 : kMaxCols;
    const bool last_batch = b0 + nb == R.ncols;
    P.ncols = nb;
    BitmapBatch bb;
    memset(&bb, 0, sizeof bb);
    bb.n = nb; bb.nbits = R.n_out; bb.status = P.status; bb.counts = R.dcnt; bb.status_words = b0 == 0 ? 16 : 0;
    for (int j = 0; j < nb; j++) {
        const int i = b0 + j;
        const DevCol &dc = R.dcols[i];
        InterpCol &ic = P.cols[j];
        memset(&ic, 0, sizeof ic);
        ic.values = reinterpret_cast<const uint64_t *>(dc.values);
        ic.vbits = dc.vbits; ic.vbit0 = dc.vbit0; ic.type = R.cols[i].type; ic.kind = R.interps[i].kind;
        interp_col_take(&ic, R.interps[i]);
        ic.out_values = reinterpret_cast<uint64_t *>(R.douts[i].values);
        ic.out_valid_words = reinterpret_cast<uint32_t *>(place ? R.outs[i].validity : R.douts[i].validity);
        if (R.edge && R.edge->next_valid[i]) { ic.next_valid = 1; ic.next_t = R.edge->next_t[i]; ic.next_v = R.edge->next_v[i]; }
        if (with_index && dc.vbits && (ic.kind == BOWGPU_INTERP_LINEAR || ic.kind == BOWGPU_INTERP_STEP_PREVIOUS)) {
            void *ix;
            BG_TRY(ctx_pool(c, kPoolInterp + 3 + j, nbr_index_bytes(R.n, dc.vbit0), &ix));  // (reused by the next batch: stream order)
            BG_TRY(nbr_index_build(c, dc.vbits, dc.vbit0, R.n, ix, &ic.nbr));
        }
        bb.work[j] = reinterpret_cast<uint32_t *>(R.douts[i].validity);
        bb.user[j] = R.outs[i].residency == BOWGPU_DEVICE ? R.outs[i].validity : nullptr;
        bb.ones[j] = 0;
        bb.count[j] = 1;
    }
    if (place) { if (b0 == 0) BG_HIP(hipMemsetAsync(P.status, 0, kStatusHeadBytes, c->stream)); }   // (the status words; the partial counts are all stored)
    else BG_TRY(launch_preset_bitmaps(c, bb));
    P.aligned16 = (reinterpret_cast<uintptr_t>(P.ts) & 15) == 0 ? 1 : 0;
    for (int j = 0; j < nb; j++) if (reinterpret_cast<uintptr_t>(P.cols[j].values) & 15) P.aligned16 = 0;
    BG_TRY(launch_interp_tiles(c, P));
    c->last_kernel_name = interp_takes_wave3(P) ? "interp_wave3_kernel" : "interp_tile_kernel";   // (bowgpu_last_kernel_name: the last launch's)
    if (!interp_takes_wave3(P) && b0 == 0) c->last_slow_rows += R.n;   // (interp_tile_kernel: 2.2 ms per 1e8 rows where interp_wave3_kernel takes 1.15)
    if (!place) BG_TRY(launch_finish_bitmaps(c, bb));
    // the batch's counts - and, behind the last batch, the status words in front of them: one copy
    if (!place) {
        if (last_batch) BG_HIP(hipMemcpyAsync(hs, P.status, kScrInterpCounts.offset + 8 * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        else BG_HIP(hipMemcpyAsync(hc, R.dcnt, 8 * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    }
    BG_HIP(hipStreamSynchronize(c->stream));   // (per batch: the pinned block is read before the next batch's copy lands in it)
    for (int j = 0; j < nb; j++) {
        unsigned long long v = 0;
        if (place) for (int k = 0; k < kInterpEdgeBlocks; k++) v += hc[j * kInterpEdgeBlocks + k];
        else v = hc[j];
        R.hcnt[b0 + j] = v;
    }
    if (last_batch) memcpy(R.hstat, hs, sizeof R.hstat);
    return 0;
}

// The output positions depend on the interval column alone, so the columns go through the kernel kMaxCols at a time (a Bow
// of any width: interpolation.go:98-161 loops over the interpolators).
static int interp_run_all(InterpRun &R, int allow_wave2, bool with_index) {
    InterpParams &P = R.P;
    P.allow_wave2 = allow_wave2;
    const bool place = R.can_place && interp_takes_wave3(P) && !(route_mask() & BOWGPU_ROUTE_INTERP_COPIES);
    P.in_place = place ? 1 : 0;
    P.trip_valid = place ? R.trip_valid : nullptr;
    uint32_t *hs;
    unsigned long long *hc;
    BG_TRY(registered_at(R.c, kRegStatus, &hs));
    BG_TRY(registered_at(R.c, kRegInterpCounts, &hc));
    // (in place: kInterpEdgeBlocks partial counts per column of the batch, every one of them stored - by interp_edge_fix_kernel, straight
    // into the host's registered block, the status words in front of them: no copy command behind the launches)
    P.valid_counts = place ? hc : R.dcnt;
    P.host_status = place ? hs : nullptr;
    for (int b0 = 0; b0 < R.ncols; b0 += kMaxCols) BG_TRY(interp_run_batch(R, b0, place, with_index, hs, hc));
    return 0;
}

// The kernel parameters of a call before its first run: pass 1's part, then what the call's arguments say, and the edge words from the
// context pool - one word per 512-row trip and column of a launch (at most kMaxCols columns per launch), and one valid-output count
static int params_begin(Ctx *c, const InterpJob &job, int32_t ts_col, int64_t interval, const bowgpu_options &o, int64_t n, int64_t n_out,
                        InterpParams *Pp, uint32_t **trip_valid) {
    InterpParams &P = *Pp;
    memset(&P, 0, sizeof P);
    BG_TRY(scratch_at(c, kScrStatus, &P.status));
    const Plan plan = found_plan(job.found, interval);
    params_take_pass1(&P, job);
    P.ts = reinterpret_cast<const int64_t *>(job.dts.values);
    P.n = n; P.interval = plan.interval; P.magic = plan.magic;
    P.inclusive = o.inclusive ? 1 : 0;
    P.has_left = job.has_left; P.left_ts = job.left_ts; P.wbase = job.found.wbase;
    P.fast32 = interp_fast32(plan, P.kq) ? 1 : 0;
    P.wide32 = interp_wide32(plan, P.kq) ? 1 : 0;
    if (P.fast32 || P.wide32) interp_magic32(plan.interval, &P.m32, &P.sh1_32, &P.sh2_32);
    P.ts_col = ts_col;
    P.n_out = n_out;
    const int64_t ntrips512 = (n + 511) / 512;
    void *ew;
    BG_TRY(ctx_pool(c, kPoolInterpEdge, (size_t)ntrips512 * kMaxCols * 12 + 64, &ew));
    P.edge_words = reinterpret_cast<uint64_t *>(ew);
    *trip_valid = reinterpret_cast<uint32_t *>(P.edge_words + ntrips512 * kMaxCols);
    return 0;
}

// The call's columns and outputs on the device, column by column.
// Device-resident outputs whose bitmaps can take whole 32-bit words - a 4-byte aligned pointer and a capacity that reaches the end
// of the word holding row n_out - 1 - are WRITTEN IN PLACE by interp_wave3_kernel, which stores every word of [0, n_out) itself
// and counts the valid outputs per trip: no launch that zeroes the bitmaps in front of it and no pass over them behind it (round 4:
// preset + finish, 41 us of 1.0 ms at 1e8 rows).  Anything else - a host-resident output, an odd pointer, a capacity of exactly
// n_out rows that ends mid-word, the workgroup kernel - keeps the working copies from the context pool and those two launches.
static int interp_stage(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t n, int64_t n_out, InterpJob *job, bowgpu_out *outs,
                        DevOut *douts, bool *can_place) {
    for (int i = 0; i < ncols; i++) {
        DevCol &dc = job->dcols[i];
        if (i == ts_col) { dc.values = job->dts.values; dc.length = n; dc.type = BOWGPU_INT64; }
        else BG_TRY(devcol_prepare(c, &cols[i], &dc, true, true));
        BG_TRY(devout_prepare(c, &outs[i], n_out, &douts[i], i < 16 ? i : -1));  // validity working copy from the context pool
        *can_place = *can_place && outs[i].residency == BOWGPU_DEVICE && (reinterpret_cast<uintptr_t>(outs[i].validity) & 3) == 0 &&
                     ((outs[i].length + 7) >> 3) >= 4 * ((n_out + 31) >> 5);
    }
    return 0;
}

int interp_fill_impl(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                     const bowgpu_interp *interps, int32_t ninterps, bowgpu_out *outs, const int64_t *global_s0, const bowgpu_interp_edge *edge) {
    if (!cols || ncols <= 0 || !outs) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    if (edge && ncols > kMaxCols) return fail(BOWGPU_ERR_UNSUPPORTED, "sharded Interpolate: at most %d columns (bowgpu_interp_edge)", kMaxCols);
    const bowgpu_options o = options_or(opts);
    Ctx *c = nullptr;
    const bool cached = cols[ts_col].length > 0 && ctx_get(&c) == 0 && interp_cache_hit(c, &cols[ts_col], interval, o.offset, o.inclusive, global_s0, edge);
    Plan probe;
    if (!cached) BG_TRY(plan_make(nullptr, &cols[ts_col], interval, o.offset, &probe));   // (the _count call that filled the cache ran these checks on the same arguments)
    BG_TRY(interp_validate(cols, ncols, ts_col, &o, interps, ninterps));
    const auto col_type = [&](int i) { return cols[i].type; };
    const int64_t n = cols[ts_col].length;
    if (n == 0) { outs_empty(outs, ninterps, col_type); return 0; }
    BG_TRY(ctx_get(&c));
    c->last_slow_rows = 0;
    InterpJob job;
    bool onepass = false;
    if (!cached && !global_s0 && !edge) BG_TRY(interp_onepass_prepare(c, cols, ncols, ts_col, interval, &o, &job, &onepass, &probe));
    if (!onepass) BG_TRY(interp_prepare(c, cols, ncols, ts_col, interval, &o, &job, global_s0, edge, true, cached ? nullptr : &probe));
    const int64_t n_out = n + job.found.M;
    if (n_out == 0) { outs_empty(outs, ninterps, col_type); return 0; }
    job.dcols.resize(ncols);
    std::vector<DevOut> douts(ninterps);
    InterpParams P;
    uint32_t *trip_valid;
    BG_TRY(params_begin(c, job, ts_col, interval, o, n, n_out, &P, &trip_valid));
    bool can_place = true;
    BG_TRY(interp_stage(c, cols, ncols, ts_col, n, n_out, &job, outs, douts.data(), &can_place));
    unsigned long long *dcnt;
    BG_TRY(scratch_at(c, kScrInterpCounts, &dcnt));
    InterpRun R = {c, P, job.dcols, cols, interps, edge, outs, douts, ncols, n, n_out, can_place, trip_valid, dcnt, {0, 0, 0, 0, 0, 0, 0, 0},
                   std::vector<uint64_t>(ninterps, 0)};
    const uint32_t *hstat = R.hstat;
    P.allow_wave2 = 1;
    const bool first_with_index = !interp_takes_wave3(P);
    BG_TRY(interp_run_all(R, 1, first_with_index));
    if (hstat[7] && !first_with_index && !hstat[0] && !hstat[6]) BG_TRY(interp_run_all(R, 1, true));   // a run of thousands of nulls next to a window start
    // An interval column out of order comes FIRST: a one-pass call derives its row count from the first and the last timestamp alone,
    // so on an unsorted column most trips also fail the "fits the counted range" test below - and the documented answer for such a
    // column is the decline (BOWGPU_ERR_TS_UNSORTED: the caller keeps the reference's own path), not an argument error.
    if (hstat[0]) return fail_ts_unsorted();
    // (a reused count whose column has changed since: interp_wave3_kernel stored nothing for the trips that did not fit and said
    // so; the kernels a redo would use do not check, so the error comes first)
    if (hstat[6]) return fail(BOWGPU_ERR_ARG, "Interpolate: the rows produced do not add up to the count - the interval column changed between "
                                              "bowgpu_rolling_interpolate_count and _fill (include/bowgpu.h: the contract between the two calls)");
    if (hstat[5] && (job.from_cache || onepass)) {
        // the redo runs a kernel that trusts pass 1 blindly (and needs one): make pass 1 this call's own before handing it over
        InterpJob fresh;
        BG_TRY(interp_prepare(c, cols, ncols, ts_col, interval, &o, &fresh, global_s0, edge, false));
        if (n + fresh.found.M != n_out) return fail(BOWGPU_ERR_ARG, "Interpolate: the interval column changed between bowgpu_rolling_interpolate_count and _fill");
        params_take_pass1(&P, fresh);
    }
    // some trip has more runs of synthetic rows than interp_wave3_kernel lists, spans 2^31 or more, or holds a gap of millions of empty
    // windows: the workgroup kernel takes the call.  It builds exclusive windows only: an inclusive call is declined instead of being
    // answered with the exclusive layout.
    if (hstat[5] && o.inclusive)
        return fail(BOWGPU_ERR_UNSUPPORTED, "Interpolate on inclusive windows: a 512-row trip that spans 2^31 or more, or holds a gap of "
                                            "millions of empty windows, is outside the device path");
    if (hstat[5]) BG_TRY(interp_run_all(R, 0, true));
    if (hstat[0]) return fail_ts_unsorted();
    for (int i = 0; i < ninterps; i++) BG_TRY(devout_finish(c, &douts[i], n_out, cols[i].type, n_out - (int64_t)R.hcnt[i], false));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace bowgpu

using namespace bowgpu;

extern "C" {

int bowgpu_rolling_interpolate_count(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                                     const bowgpu_options *opts, const bowgpu_interp *interps, int32_t ninterps, int64_t *n_out) {
    bool null_ts = false;
    if (n_out) BG_TRY(interp_null_ts_any(cols, ncols, ts_col, interval, opts, interps, ninterps, n_out, nullptr, &null_ts));
    if (null_ts) return 0;
    return interp_count_impl(cols, ncols, ts_col, interval, opts, interps, ninterps, n_out, nullptr, nullptr);
}

int bowgpu_rolling_interpolate_fill(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                                    const bowgpu_options *opts, const bowgpu_interp *interps, int32_t ninterps, bowgpu_out *outs) {
    bool null_ts = false;
    if (outs) BG_TRY(interp_null_ts_any(cols, ncols, ts_col, interval, opts, interps, ninterps, nullptr, outs, &null_ts));
    if (null_ts) return 0;
    return interp_fill_impl(cols, ncols, ts_col, interval, opts, interps, ninterps, outs, nullptr, nullptr);
}

// ---- row-range sharded Interpolate: a shard + what lies beyond its two ends
int bowgpu_shard_interpolate_count(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                                   int64_t global_s0, const bowgpu_interp *interps, int32_t ninterps, const bowgpu_interp_edge *edge,
                                   int64_t *n_out) {
    return interp_count_impl(cols, ncols, ts_col, interval, opts, interps, ninterps, n_out, &global_s0, edge);
}

int bowgpu_shard_interpolate_fill(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                                  int64_t global_s0, const bowgpu_interp *interps, int32_t ninterps, const bowgpu_interp_edge *edge,
                                  bowgpu_out *outs) {
    return interp_fill_impl(cols, ncols, ts_col, interval, opts, interps, ninterps, outs, &global_s0, edge);
}

// first / last valid point of every column of a shard: what its neighbours' Linear / StepPrevious interpolators may need
int bowgpu_shard_interp_points(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, bowgpu_interp_points *out) {
    if (!cols || !out || ncols <= 0 || ncols > kMaxCols) return fail(BOWGPU_ERR_ARG, "bad argument");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    memset(out, 0, sizeof *out);
    const int64_t n = cols[ts_col].length;
    out->nrows = n;
    if (n == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevCol dts;
    BG_TRY(ts_contract(c, &cols[ts_col]));
    BG_TRY(ts_device(c, &cols[ts_col], &dts));
    void *pool;
    BG_TRY(ctx_pool(c, kPoolShard, 16384, &pool));
    int64_t *drows = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(pool) + 12288);  // [col][first, last]
    std::vector<DevCol> dcs(ncols);
    for (int i = 0; i < ncols; i++) {
        if (cols[i].type != BOWGPU_INT64 && cols[i].type != BOWGPU_FLOAT64) return fail(BOWGPU_ERR_UNSUPPORTED, "column type outside the device path");
        BG_TRY(devcol_prepare(c, &cols[i], &dcs[i], true, true));
        BG_TRY(launch_first_last_valid(c, dcs[i].vbits, dcs[i].vbit0, n, drows + 2 * i));
    }
    int64_t hrows[2 * kMaxCols];
    BG_HIP(hipMemcpyAsync(hrows, drows, sizeof(int64_t) * 2 * ncols, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    auto at = [&](const void *base, int64_t row, uint64_t *v) -> int {
        BG_HIP(hipMemcpyAsync(v, reinterpret_cast<const char *>(base) + 8 * row, 8, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    uint64_t tf = 0, tl = 0;
    BG_TRY(at(dts.values, 0, &tf));
    BG_TRY(at(dts.values, n - 1, &tl));
    uint64_t tv[4 * kMaxCols] = {0};
    for (int i = 0; i < ncols; i++) {
        const int64_t fr = hrows[2 * i], lr = hrows[2 * i + 1];
        out->first_valid[i] = fr >= 0; out->last_valid[i] = lr >= 0;
        if (fr >= 0) { BG_TRY(at(dts.values, fr, &tv[4 * i])); BG_TRY(at(dcs[i].values, fr, &tv[4 * i + 1])); }
        if (lr >= 0) { BG_TRY(at(dts.values, lr, &tv[4 * i + 2])); BG_TRY(at(dcs[i].values, lr, &tv[4 * i + 3])); }
    }
    BG_HIP(hipStreamSynchronize(c->stream));
    out->first_ts = (int64_t)tf; out->last_ts = (int64_t)tl;
    for (int i = 0; i < ncols; i++) {
        auto as_f64 = [&](uint64_t b) { double d; if (cols[i].type == BOWGPU_FLOAT64) memcpy(&d, &b, 8); else d = (double)(int64_t)b; return d; };
        out->first_t[i] = (double)(int64_t)tv[4 * i]; out->first_v[i] = as_f64(tv[4 * i + 1]);
        out->last_t[i] = (double)(int64_t)tv[4 * i + 2]; out->last_v[i] = as_f64(tv[4 * i + 3]);
        out->last_v_i64[i] = (int64_t)tv[4 * i + 3];
    }
    return 0;
}

}  // extern "C"
