// What the calls over several devices share (multi.cpp: the fan-out of bowgpu_set_devices and bowgpu_rolling_aggregate_sharded;
// sort_shard_api.cpp: bowgpu_sort_by_col_sharded): one persistent library thread per rank, the dispatch of one function over them,
// a barrier among the ranks of one call.  Defined in multi.cpp.
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
