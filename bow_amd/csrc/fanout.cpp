// fanout.cpp — the library threads of the calls over several devices and the configuration of the fan-out (fanout.h; SURVEY.md §8b
// `bowgpu_set_devices`, §8e).  bowgpu_set_devices(ids, n) names the devices; from then on bowgpu_rolling_aggregate / _planned /
// _interpolate_aggregate are cut into row ranges, one per listed device, on one persistent host thread per device (fan_call.cpp).
// The calls over the CALLER's shards (sharded_call.cpp, sort_shard_api.cpp) have a pool of their own.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "fanout.h"

namespace bowgpu {
namespace {

std::atomic<int64_t> g_calls_listed{0}, g_calls_served{0};   // bowgpu_fanout_counts
thread_local int g_last_ranks = 1;            // ranks that served the calling thread's last Rolling.Aggregate (bowgpu_last_call_ranks)
std::mutex g_cfg_mu;
std::vector<int> g_ids;                      // guarded by g_cfg_mu
int64_t g_min_rows = (int64_t)1 << 20;       // rows per rank below which a call is not cut further
Fanout *g_fan = nullptr;                     // never destroyed (a worker may sit in its condition variable at process exit)
Fanout *g_sharded = nullptr;                 // the workers of the calls over the caller's shards (not the fan-out's); never destroyed either

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

FanSession::FanSession() {
    g_last_ranks = 1;
    env_defaults();
    {
        std::lock_guard<std::mutex> g(g_cfg_mu);
        ids = g_ids;
        min_rows = g_min_rows;
    }
    if (ids.size() >= 2) g_calls_listed.fetch_add(1, std::memory_order_relaxed);
}

void FanSession::start() {
    {
        std::lock_guard<std::mutex> g(g_cfg_mu);
        if (!g_fan) g_fan = new Fanout();
        f = g_fan;
    }
    call_lock = std::unique_lock<std::mutex>(f->call_mu);
    if (f->ids != ids) { fan_stop_locked(f); fan_start_locked(f, ids); }
}

void FanSession::served(int world) {
    g_last_ranks = world;
    g_calls_served.fetch_add(1, std::memory_order_relaxed);
}

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

int device_of(const void *p, int *dev) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); *dev = -1; return 0; }
    *dev = a.device;
    return 0;
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

int bowgpu_set_fanout_min_rows(int64_t rows) {
    if (rows < 1) return fail(BOWGPU_ERR_ARG, "bowgpu_set_fanout_min_rows: at least one row per rank");
    env_defaults();
    std::lock_guard<std::mutex> g(g_cfg_mu);
    g_min_rows = rows;
    return 0;
}

}  // extern "C"
