// What the calls over several devices share (fan_call.cpp: the fan-out of bowgpu_set_devices; sharded_call.cpp:
// bowgpu_rolling_aggregate_sharded; sort_shard_api.cpp: bowgpu_sort_by_col_sharded): one persistent library thread per rank, the
// dispatch of one function over them, a barrier among the ranks of one call (fanout.cpp), the staging of a rank's rows (fan_call.cpp).
#pragma once

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"

namespace bowgpu {

// ---------------------------------------------------------------- the workers: one persistent thread per listed device
struct Worker {
    int device = 0;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, quit = false;
    bool device_set = false;
};

struct Fanout {
    std::mutex call_mu;            // one fanned-out call at a time (the devices are busy with it anyway)
    std::vector<Worker *> workers;
    std::vector<int> ids;          // what the workers were started for
    std::mutex done_mu;
    std::condition_variable done_cv;
    int pending = 0;
};

// runs fn(rank) on worker `rank` for rank in [0, world) and waits for all of them
void fan_run(Fanout *f, int world, const std::function<void(int)> &fn);

// One call's view of the fan-out of bowgpu_set_devices (fanout.cpp owns the list, the pool and the counters).  Constructed: the list
// and the row threshold as they are now (environment defaults applied), the calling thread's bowgpu_last_call_ranks back to 1, the
// call counted as listed when two or more devices are.  start(): call_mu taken for the session's lifetime (one fanned-out call per
// process at a time), the workers restarted when the list has changed.  served(): the call counted, its ranks remembered.
struct FanSession {
    std::vector<int> ids;
    int64_t min_rows = 0;
    Fanout *f = nullptr;
    std::unique_lock<std::mutex> call_lock;
    FanSession();
    void start();
    void served(int world);
};

// A rank's rows of a call's columns as the record protocol sees them.  Pageable columns are staged ONCE (the record pass and the
// rank's pass both read the staged copy: each row crosses the host link once), values from an 8-row boundary so that one offset
// serves values and bits; the others are the caller's buffers at the rank's offset.  rank_stage synchronises the stream.
struct RankRows {
    std::vector<bowgpu_col> cols;
    std::vector<DevBuf> staged_bufs;   // [2 * ncols]: the values and the bits of column i
    bool staged = false;
    void release_rows() { staged_bufs.clear(); staged = false; }   // on the rank's own thread: the blocks go back to THAT thread's (device's) cache
};
struct StageArgs {   // what rank_stage reads of a call
    const bowgpu_col *cols; int32_t ncols, ts_col;
    const bowgpu_agg *aggs; int32_t naggs;
    bool all_used;   // every column is staged, not only the interval column and the aggregators' (Interpolate rewrites them all)
};
int rank_stage(Ctx *c, const StageArgs &a, int64_t row0, int64_t nrows, RankRows *rk);

// the workers of the calls over the CALLER's shards (not the fan-out's): one pool, one call at a time (call_mu), grown to the
// largest world seen; a worker moves to the device its rank names
Fanout *sharded_pool();
void sharded_grow_locked(Fanout *f, int world);
int sharded_enter(Worker *w, int device, uint32_t route, Ctx **c);

// the device a pointer lives on (-1: not device memory the runtime knows)
int device_of(const void *p, int *dev);

// A barrier among the workers of one call, in two forms that one call does not mix.
// wait / abort - sticky abort: once a rank has failed, every wait - now or later - returns false, so no worker is left waiting for
// a rank that will not come.
// vote - every rank reaches every barrier, whatever its status, and says whether it is well; all of them get the same answer: whether
// every rank was.  For calls whose ranks read each other's device memory: a rank that has failed still stands at the barrier behind
// which its buffers are no longer read.
struct Barrier {
    std::mutex mu;
    std::condition_variable cv;
    int n = 0, arrived = 0;
    uint64_t gen = 0;
    bool aborted = false;
    bool all_ok = true, result[2] = {true, true};   // vote: the generation under way; the last two that completed
    bool wait() {
        std::unique_lock<std::mutex> lk(mu);
        if (aborted) return false;
        const uint64_t g = gen;
        if (++arrived == n) { arrived = 0; gen++; cv.notify_all(); return true; }
        cv.wait(lk, [&] { return gen != g || aborted; });
        return gen != g;
    }
    void abort() {
        std::lock_guard<std::mutex> g(mu);
        aborted = true;
        cv.notify_all();
    }
    bool vote(bool ok) {
        std::unique_lock<std::mutex> lk(mu);
        all_ok = all_ok && ok;
        const uint64_t g = gen;
        if (++arrived == n) {
            result[g & 1] = all_ok;   // (read by the ranks of generation g; written again by g + 2, which needs them all at g + 1 first)
            all_ok = true;
            arrived = 0;
            gen++;
            cv.notify_all();
            return result[g & 1];
        }
        cv.wait(lk, [&] { return gen != g; });
        return result[g & 1];
    }
};

}  // namespace bowgpu
