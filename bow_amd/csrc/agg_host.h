// agg_host.h — what the host files of Rolling.Aggregate hand each other: agg_pass.cpp (the pass machinery), aggregate_api.cpp
// (the unsharded call) and shard_api.cpp (the shard protocol).  Host only: no .hip file and not common.h includes it.
#pragma once

#include <algorithm>

#include "common.h"

namespace bowgpu {

// What every stage of one Aggregate call is given: the frame, its plan and the call's flags
struct AggCall {
    const bowgpu_col *cols;
    int32_t ncols, ts_col;
    const Plan &plan;
    int inclusive;
    bool strict;       // bowgpu_options.strict_order of the call (or BOWGPU_ROUTE_STRICT_ORDER): every window in row order, or the call is declined
    bool check_plan;   // the plan came from the caller (bowgpu_rolling_aggregate_planned): the pass checks it against the column
};

// Which kinds of reducer a call has, in the encoding the wave-tile kernels read (common.h kNeed*) + Mode, which only the host asks about
constexpr uint32_t kNeedMode = 32, kNeedTimeWeighted = kNeedStep | kNeedTrap;

// One aggregate call in three stages so that the sharded entry points can reuse them:
//   job_build  - device residency of columns / outputs + the kernels' descriptor block
//   job_run    - bitmap initialisation, tile kernel, long-window kernel
//   job_finish - null counts of the nullable outputs, copy-back of host-resident outputs
struct AggJob {
    std::vector<DevCol> dcols;
    std::vector<DevOut> douts;
    DevCol dts;
    AggParams P;
    int64_t W = 0;
    unsigned long long *counts = nullptr;   // kScrAggCounts of the scratch block (P.status: its kScrStatus)
    int inclusive = 0;
    bool counts_used = false;   // the valid counters hold a previous count (they accumulate): zero them before counting again
    bool tail_wrote_host = false;   // the finish launch stores the status words and the counts into the registered host block itself
    // the call as job_build was given it - copies, so that a job outlives the entry point that built it (bowgpu_shard_pass_begin)
    bowgpu_agg aggs[kMaxAggs];
    int32_t naggs = 0;
    uint32_t need = 0;          // need_mask of aggs
    Plan plan;
    bool strict = false, check_plan = false;   // AggCall's
};

// Which column pass (slot) serves each reducer that reads values: its column's, or a new one when the column has none yet or when
// its slot already serves per_pass nullable reducers (the general kernel takes 4 per pass; rolling_fused.hip has no such limit)
struct ColSlots {
    std::vector<int> slot_of, nullable_in_slot;
    explicit ColSlots(int ncols) : slot_of(ncols, -1) {}
    int count() const { return (int)nullable_in_slot.size(); }
    void clear() { nullable_in_slot.clear(); std::fill(slot_of.begin(), slot_of.end(), -1); }
    int find(const bowgpu_agg &a, int per_pass) const {   // -1: take() would open a slot
        const int s = slot_of[a.col];
        return (s >= 0 && !kind_never_nil(a.kind) && nullable_in_slot[s] >= per_pass) ? -1 : s;
    }
    int take(const bowgpu_agg &a, int per_pass) {
        int s = find(a, per_pass);
        if (s < 0) { s = count(); slot_of[a.col] = s; nullable_in_slot.push_back(0); }
        if (!kind_never_nil(a.kind)) nullable_in_slot[s]++;
        return s;
    }
};

// Windows longer than a tile's look-ahead: workspace from the context pool, then long_windows.hip
struct LongWork {
    void *entries; int32_t *nchunks; int64_t *offsets, *sums, *total; int32_t *work_entry; void *parts;
    int64_t max_work;
};
// The attempts of a tile pass.  A wave-tile kernel raises kAggStRedo when some tile is beyond what it can describe - more window heads
// than its small list holds (clumpy data: a high average of rows per window, yet a dense tile), window ids it cannot encode - and
// job_pass_complete then makes PassState::redo_with the next attempt
enum TileAttempt { kAttemptFirst, kAttemptLargeList /* no compacting kernel, the large head list (400 heads per 640 rows) */,
                   kAttemptNoSimple /* the general lean kernel */, kAttemptNone };
struct PassState {
    TileAttempt redo_with = kAttemptNone;   // job_launch_tiles: the attempt that follows the one it launched (kAttemptNone: nothing that raises kAggStRedo ran)
    bool band_rows = false;     // job_run: a nullable column under extrema / First + Last alone, 129 .. 200 rows per window - rolling_simple.hip + the queue launch, not rolling_twc.hip
    uint32_t *hstat = nullptr;
    uint64_t *hcnt = nullptr;
    bool queue = false;     // long_queue_kernel rides behind the tile kernel: the queued windows are served without the host in between
    LongWork qw{};          // ... its workspace (sized for the queue's capacity)
};

// agg_pass.cpp
int job_build(Ctx *c, const AggCall &call, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, int64_t wid_base, int64_t W,
              bool holds_row0, AggJob *job, int nullable_per_pass = 4);
int job_run(Ctx *c, AggJob *job, int64_t *long_windows, double *kernel_ms, bool finish, bool allow_long_only = false);
int job_pass_enqueue(Ctx *c, AggJob *job, bool finish, PassState *ps);
int job_pass_complete(Ctx *c, AggJob *job, bool finish, PassState *ps, int64_t *long_windows, double *kernel_ms);
int job_finish(Ctx *c, AggJob *job, bool strict);
int fused_try(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, const bowgpu_options &o, int inclusive,
              const bowgpu_interp *interps, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, double *kernel_ms, bool *done);
double now_us();   // CLOCK_MONOTONIC: the stamps of BOWGPU_CALL_PROFILE
// aggregate_api.cpp
int enforce_interval_and_offset(int64_t interval, int64_t offset, int64_t *out);
int64_t first_window_start(int64_t first, int64_t interval, int64_t offset_norm);
int validate_aggs(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs, int *inclusive, int *new_interval_col);
uint32_t need_mask(const bowgpu_agg *aggs, int32_t naggs);
int front_check(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t ts_col);
bool strict_wanted(const bowgpu_options *o);
// shard_api.cpp
int shard_check(const bowgpu_col *cols, const bowgpu_agg *aggs, int32_t naggs);

}  // namespace bowgpu
