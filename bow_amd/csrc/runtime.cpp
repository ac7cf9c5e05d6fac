// runtime.cpp — what every entry point of libbowgpu.so stands on: errors, the route mask, the per-thread device state (context,
// block cache, the pass a shard call left in flight), and the C ABI of devices, streams, memory, timers, generators and probes.
// Without a GPU every entry point fails with BOWGPU_ERR_NO_DEVICE.

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "common.h"

namespace bowgpu {

// ---------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof g_err, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    if (e == hipErrorOutOfMemory) return BOWGPU_ERR_OOM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) return BOWGPU_ERR_NO_DEVICE;
    return BOWGPU_ERR_HIP;
}

// ---------------------------------------------------------------- test / A-B routing
// Which kernel serves a call is decided from the call's shape alone.  The tests (and A/B measurements) need to push one call
// through every kernel that can take it: bowgpu_debug_set_route() sets a PER-THREAD mask of BOWGPU_ROUTE_* bits.  Nothing on the
// call path reads the environment; BOWGPU_ROUTE=<mask> is read ONCE per process as the initial mask of every thread (so that a
// profiler run of an unmodified script can pick a kernel).
static uint32_t route_env_default() {
    static const uint32_t v = [] { const char *e = getenv("BOWGPU_ROUTE"); return e ? (uint32_t)strtoul(e, nullptr, 0) : 0u; }();
    return v;
}
static thread_local uint32_t g_route = route_env_default();
uint32_t route_mask() { return g_route; }

static std::atomic<uint64_t> g_write_epoch{1};
uint64_t device_write_epoch() { return g_write_epoch.load(std::memory_order_relaxed); }
void device_write_epoch_bump() { g_write_epoch.fetch_add(1, std::memory_order_relaxed); }

// ---------------------------------------------------------------- context
// All device state is per calling thread (cgo calls arrive on arbitrary OS threads).  A thread that exits gives its state
// back: stream, events, pools, pinned block and its cache of scratch blocks - unless the process itself is exiting (the HIP
// runtime may already be going down then; the sentinel below is constructed after the runtime's own statics, so it is
// destroyed before them).
static bool g_process_exiting = false;
namespace {
struct ExitSentinel { ~ExitSentinel() { g_process_exiting = true; } };
void ctx_release(Ctx *c) {
    if (!c->inited) return;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->null_ts_cache && c->null_ts_cache_free) { void *q = c->null_ts_cache; c->null_ts_cache = nullptr; c->null_ts_cache_free(q); }
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->d_params) (void)hipFree(c->d_params);
    for (int i = 0; i < Ctx::kPoolSlots; i++) if (c->pool[i]) (void)hipFree(c->pool[i]);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_bounce) { (void)hipHostFree(c->h_bounce); (void)hipEventDestroy(c->bounce_ev[0]); (void)hipEventDestroy(c->bounce_ev[1]); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    *c = Ctx();
}
struct CtxHolder {
    Ctx c;
    ~CtxHolder() { if (!g_process_exiting) ctx_release(&c); }
};
}  // namespace

// ---------------------------------------------------------------- per-thread cache of device scratch blocks
// Each thread keeps the blocks its calls freed (steady-state calls issue no hipMalloc / hipFree).  The caches are registered
// process-wide so that memory one thread hoards does not starve another: a failed allocation trims EVERY thread's cache before
// it gives up, bowgpu_trim() does the same on request, and a thread that exits frees its own.
namespace {
struct BufCache;
std::mutex g_caches_mu;
std::vector<BufCache *> g_caches;   // guarded by g_caches_mu
struct BufCache {
    struct E { void *p; size_t cap; };
    std::mutex mu;                  // the owner works under it; another thread takes it only to trim
    std::vector<E> v;
    size_t total = 0;
    BufCache() { std::lock_guard<std::mutex> g(g_caches_mu); g_caches.push_back(this); }
    size_t drop_all_locked() {
        size_t freed = 0;
        for (const E &e : v) { (void)hipFree(e.p); freed += e.cap; }
        v.clear();
        total = 0;
        return freed;
    }
    size_t drop_all() { std::lock_guard<std::mutex> g(mu); return drop_all_locked(); }
    ~BufCache() {
        { std::lock_guard<std::mutex> g(g_caches_mu); g_caches.erase(std::remove(g_caches.begin(), g_caches.end(), this), g_caches.end()); }
        if (!g_process_exiting) drop_all();   // (process exit: the runtime may already be gone; leave the blocks to it)
    }
};
constexpr size_t kCacheEntries = 24;
constexpr size_t kCacheBytes = (size_t)24 << 30;   // per thread
size_t trim_all_threads() {
    std::lock_guard<std::mutex> g(g_caches_mu);
    size_t freed = 0;
    for (BufCache *c : g_caches) freed += c->drop_all();
    return freed;
}

// ONE owner of a thread's device state.  Members are destroyed in reverse order of declaration: the pass in flight and the
// null-timestamp cache hold blocks of `bufs` and use the stream of `ctx`, so ~ThreadState settles them first, then bufs, then ctx go.
struct InFlight {   // bowgpu_shard_pass_begin's PendingPass (shard_api.cpp), opaque here as Ctx::null_ts_cache is
    void *p = nullptr;
    void (*destroy)(void *) = nullptr;
    void drop(Ctx *c) {
        if (!p) return;
        if (c && c->inited) (void)hipStreamSynchronize(c->stream);   // its kernels are done with the scratch blocks before anyone reuses them
        void *q = p;
        p = nullptr;
        destroy(q);
    }
};
struct ThreadState {
    CtxHolder ctx;
    BufCache bufs;
    InFlight pending;
    bool pending_owner = false;
    ~ThreadState() {   // (at process exit the pass is left to the runtime, as the blocks are)
        if (g_process_exiting || !ctx.c.inited) return;
        (void)hipSetDevice(ctx.c.device);
        pending.drop(&ctx.c);
        ctx_drop_null_ts_cache(&ctx.c);
    }
};
thread_local ThreadState g_thread;
}  // namespace

// BOWGPU_ABORT_TRACE=1 (diagnostic): the C stack of whoever calls abort() - the HIP runtime does so on a queue error, with no
// message when stderr is not a terminal - before the process dies
static void abort_trace(int) {
    void *frames[64];
    const int n = backtrace(frames, 64);
    static const char msg[] = "bowgpu: SIGABRT, C stack:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(SIGABRT, SIG_DFL);
    raise(SIGABRT);
}

// bowgpu_shard_pass_begin leaves a pass in flight on the thread's stream (shard_api.cpp PendingPass): its kernels use the context's
// scratch, pools and pinned read-back block.  Its two owners (bowgpu_shard_pass_begin, bowgpu_shard_finish) mark themselves; EVERY
// other entry point that takes the context settles and drops the pass first, so nothing reuses that memory under running kernels
// (the header states the rule; this enforces it).  A thread that exits with a pass in flight: ~ThreadState.
PendingOwnerScope::PendingOwnerScope() : was(g_thread.pending_owner) { g_thread.pending_owner = true; }
PendingOwnerScope::~PendingOwnerScope() { g_thread.pending_owner = was; }
void pending_set(void *p, void (*destroy)(void *)) { g_thread.pending.p = p; g_thread.pending.destroy = destroy; }
void *pending_get() { return g_thread.pending.p; }
void pending_drop(Ctx *c) { g_thread.pending.drop(c); }

int ctx_get(Ctx **out) {
    static ExitSentinel sentinel;   // (constructed on the first call of any thread)
    (void)sentinel;
    static const bool traced = [] {
        const char *t = getenv("BOWGPU_ABORT_TRACE");
        if (t && t[0] == '1') signal(SIGABRT, abort_trace);
        return true;
    }();
    (void)traced;
    Ctx *c = &g_thread.ctx.c;
    if (!c->inited) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0)
            return fail(BOWGPU_ERR_NO_DEVICE, "no HIP device available (hipGetDeviceCount: %s); the bowgpu path has no CPU fallback",
                        e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        if (c->device >= n) return fail(BOWGPU_ERR_NO_DEVICE, "device %d out of range (%d devices)", c->device, n);
        BG_HIP(hipSetDevice(c->device));
        BG_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        BG_HIP(hipEventCreate(&c->ev0));
        BG_HIP(hipEventCreate(&c->ev1));
        if (!c->stream) c->stream = c->own_stream;
        c->inited = true;
    } else {
        BG_HIP(hipSetDevice(c->device));  // cgo calls may hop OS threads: no thread-affine HIP state assumed
    }
    if (!g_thread.pending_owner) g_thread.pending.drop(c);
    *out = c;
    return 0;
}

int current_device_of_thread() { return g_thread.ctx.c.device; }

void ctx_drop_null_ts_cache(Ctx *c) {
    if (c->null_ts_cache && c->null_ts_cache_free) { void *p = c->null_ts_cache; c->null_ts_cache = nullptr; c->null_ts_cache_free(p); }
}

int ctx_scratch(Ctx *c, size_t bytes, void **dptr) {
    if (bytes < kScrFixedBytes) bytes = kScrFixedBytes;   // (ctx_blocks.h: only a tile pass' long-window list asks for more)
    if (c->d_scratch_bytes < bytes) {
        if (c->d_scratch) (void)hipFree(c->d_scratch);
        c->d_scratch = nullptr;
        c->d_scratch_bytes = 0;
        BG_HIP(hipMalloc(&c->d_scratch, bytes));
        c->d_scratch_bytes = bytes;
    }
    *dptr = c->d_scratch;
    return 0;
}

int ctx_pinned(Ctx *c, void **hptr) {
    if (!c->h_pinned) {   // one block for every small user: it never moves under them
        BG_HIP(hipHostMalloc(&c->h_pinned, kRegBytes, hipHostMallocDefault));
        c->h_pinned_bytes = kRegBytes;
    }
    *hptr = c->h_pinned;
    return 0;
}

int ctx_params(Ctx *c, void **dptr) {
    if (!c->d_params) BG_HIP(hipMalloc(&c->d_params, 4096));
    *dptr = c->d_params;
    return 0;
}

int ctx_pool(Ctx *c, int slot, size_t bytes, void **dptr) {
    if (slot < 0 || slot >= Ctx::kPoolSlots) return fail(BOWGPU_ERR_ARG, "bad pool slot");
    c->pool_gen[slot]++;
    if (c->pool_bytes[slot] < bytes) {
        if (c->pool[slot]) (void)hipFree(c->pool[slot]);
        c->pool[slot] = nullptr;
        c->pool_bytes[slot] = 0;
        BG_HIP(hipMalloc(&c->pool[slot], bytes));
        c->pool_bytes[slot] = bytes;
    }
    *dptr = c->pool[slot];
    return 0;
}

void devbuf_cache_drop() { g_thread.bufs.drop_all(); }

int devbuf_acquire(size_t n, void **p, size_t *cap) {
    {
        std::lock_guard<std::mutex> g(g_thread.bufs.mu);
        // smallest cached block that holds n without wasting more than half of itself (or 1 MiB)
        int best = -1;
        for (size_t i = 0; i < g_thread.bufs.v.size(); i++) {
            const size_t c = g_thread.bufs.v[i].cap;
            if (c >= n && (c <= 2 * n || c <= n + (1u << 20)) && (best < 0 || c < g_thread.bufs.v[best].cap)) best = (int)i;
        }
        if (best >= 0) {
            *p = g_thread.bufs.v[best].p;
            *cap = g_thread.bufs.v[best].cap;
            g_thread.bufs.total -= *cap;
            g_thread.bufs.v.erase(g_thread.bufs.v.begin() + best);
            return 0;
        }
    }
    hipError_t e = hipMalloc(p, n);
    if (e == hipErrorOutOfMemory) {  // give every thread's cached blocks back and try once more
        (void)hipGetLastError();
        if (trim_all_threads() > 0) e = hipMalloc(p, n);
    }
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    *cap = n;
    return 0;
}

void devbuf_release(void *p, size_t cap) {
    std::lock_guard<std::mutex> g(g_thread.bufs.mu);
    g_thread.bufs.v.push_back({p, cap});
    g_thread.bufs.total += cap;
    while (g_thread.bufs.v.size() > kCacheEntries || g_thread.bufs.total > kCacheBytes) {  // evict the largest
        size_t big = 0;
        for (size_t i = 1; i < g_thread.bufs.v.size(); i++) if (g_thread.bufs.v[i].cap > g_thread.bufs.v[big].cap) big = i;
        (void)hipFree(g_thread.bufs.v[big].p);
        g_thread.bufs.total -= g_thread.bufs.v[big].cap;
        g_thread.bufs.v.erase(g_thread.bufs.v.begin() + big);
    }
}

int DevBuf::alloc(size_t n) {
    if (p) { devbuf_release(p, cap); p = nullptr; cap = 0; }
    bytes = n;
    if (n == 0) return 0;
    return devbuf_acquire(n, &p, &cap);
}

// ---------------------------------------------------------------- magic division
MagicDiv magic_make(uint64_t d) {
    // Granlund & Montgomery, "Division by invariant integers using multiplication", fig. 4.1, N = 64
    MagicDiv r;
    int l = 0;
    while (l < 64 && ((unsigned __int128)1 << l) < d) l++;
    const unsigned __int128 two_l = (unsigned __int128)1 << l;
    const unsigned __int128 num = ((two_l - d) << 64);
    r.m = (uint64_t)(num / d) + 1;
    r.sh1 = l < 1 ? (uint32_t)l : 1u;
    r.sh2 = l > 1 ? (uint32_t)(l - 1) : 0u;
    return r;
}

}  // namespace bowgpu

using namespace bowgpu;

// ====================================================================================== C ABI
extern "C" {

int bowgpu_abi_version(void) { return BOWGPU_ABI_VERSION; }

int bowgpu_debug_set_route(uint32_t mask) {
    if (mask & ~(uint32_t)BOWGPU_ROUTE__ALL) return fail(BOWGPU_ERR_ARG, "unknown route bits 0x%x", mask & ~(uint32_t)BOWGPU_ROUTE__ALL);
    g_route = mask;
    return 0;
}
int bowgpu_debug_get_route(uint32_t *mask) {
    if (!mask) return fail(BOWGPU_ERR_ARG, "null argument");
    *mask = g_route;
    return 0;
}

const char *bowgpu_last_error(void) { return g_err; }

int bowgpu_device_count(int *count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
    *count = n;
    return 0;
}

int bowgpu_set_device(int device) {
    Ctx *c = &g_thread.ctx.c;
    if (c->inited && c->device != device) {
        // drop per-device state of the old device
        (void)hipSetDevice(c->device);
        ctx_drop_null_ts_cache(c);   // (its blocks go back to the cache that is dropped next)
        devbuf_cache_drop();
        ctx_release(c);
    }
    c->device = device;
    Ctx *cc;
    return ctx_get(&cc);
}

int bowgpu_trim(int32_t all_threads, int64_t *bytes_freed) {
    // cached scratch blocks back to the device: the calling thread's, or every thread's (an idle service about to hand the GPU
    // to someone else; a host that saw BOWGPU_ERR_OOM from another library)
    Ctx *c;
    BG_TRY(ctx_get(&c));
    ctx_drop_null_ts_cache(c);
    const size_t freed = all_threads ? trim_all_threads() : g_thread.bufs.drop_all();
    if (bytes_freed) *bytes_freed = (int64_t)freed;
    return 0;
}

// The range is registered as given.  A range that an earlier registration already covers is fine; one it covers only partly is
// refused (two small buffers inside one page can do that: register the enclosing allocation instead).
int bowgpu_host_register(void *ptr, int64_t bytes) {
    if (!ptr || bytes <= 0) return fail(BOWGPU_ERR_ARG, "null buffer / non-positive size");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    if (e == hipErrorHostMemoryAlreadyRegistered) {
        if (host_mapped(ptr, "first byte's") && host_mapped(reinterpret_cast<char *>(ptr) + bytes - 1, "last byte's")) return 0;
        return fail(BOWGPU_ERR_ARG, "bowgpu_host_register: the range overlaps an earlier registration only partly");
    }
    return hip_fail(e, "hipHostRegister");
}

int bowgpu_host_unregister(void *ptr) {
    if (!ptr) return fail(BOWGPU_ERR_ARG, "null buffer");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipStreamSynchronize(c->stream));   // nothing of this thread is still reading it
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {   // (a range that an earlier, still live registration covers stays with its owner)
        (void)hipGetLastError();
        if (e != hipErrorHostMemoryNotRegistered && e != hipErrorInvalidValue) return hip_fail(e, "hipHostUnregister");
    }
    return 0;
}

int bowgpu_mem_info(int64_t *free_bytes, int64_t *total_bytes) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    size_t f = 0, t = 0;
    BG_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}

int bowgpu_device_name(char *buf, int cap) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    hipDeviceProp_t prop;
    BG_HIP(hipGetDeviceProperties(&prop, c->device));
    snprintf(buf, (size_t)cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
}

int bowgpu_set_stream(void *hip_stream) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return 0;
}

int bowgpu_synchronize(void) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

const char *bowgpu_last_kernel_name(void) {
    Ctx *c;
    if (ctx_get(&c) != 0) return "";
    return c->last_kernel_name;
}

int bowgpu_last_call_slow_rows(int64_t *rows) {
    if (!rows) return fail(BOWGPU_ERR_ARG, "null argument");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    *rows = c->last_slow_rows;
    return 0;
}

int bowgpu_last_kernel_ms(double *ms) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    *ms = c->last_kernel_ms;
    return 0;
}

int bowgpu_malloc(void **ptr, int64_t bytes) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (bytes < 0) return fail(BOWGPU_ERR_ARG, "negative size");
    *ptr = nullptr;
    BG_HIP(hipMalloc(ptr, (size_t)(bytes > 0 ? bytes : 1)));
    return 0;
}

int bowgpu_free(void *ptr) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    device_write_epoch_bump();   // (the address may come back from the allocator holding other data)
    if (ptr) BG_HIP(hipFree(ptr));
    return 0;
}

int bowgpu_memcpy_h2d(void *dst, const void *src, int64_t bytes) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (bytes > 0) {
        device_write_epoch_bump();
        BG_TRY(copy_h2d(c, dst, src, (size_t)bytes));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int bowgpu_memcpy_d2h(void *dst, const void *src, int64_t bytes) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (bytes > 0) {
        BG_TRY(copy_d2h(c, dst, src, (size_t)bytes));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int bowgpu_memset(void *dst, int value, int64_t bytes) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (bytes > 0) { device_write_epoch_bump(); BG_HIP(hipMemsetAsync(dst, value, (size_t)bytes, c->stream)); }
    return 0;
}

struct Timer {
    hipEvent_t a, b;
};

int bowgpu_timer_create(void **timer) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    Timer *t = new Timer();
    BG_HIP(hipEventCreate(&t->a));
    BG_HIP(hipEventCreate(&t->b));
    *timer = t;
    return 0;
}
int bowgpu_timer_start(void *timer) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipEventRecord(reinterpret_cast<Timer *>(timer)->a, c->stream));
    return 0;
}
int bowgpu_timer_stop(void *timer) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_HIP(hipEventRecord(reinterpret_cast<Timer *>(timer)->b, c->stream));
    return 0;
}
int bowgpu_timer_elapsed_ms(void *timer, double *ms) {
    Timer *t = reinterpret_cast<Timer *>(timer);
    BG_HIP(hipEventSynchronize(t->b));
    float f = 0;
    BG_HIP(hipEventElapsedTime(&f, t->a, t->b));
    *ms = f;
    return 0;
}
int bowgpu_timer_destroy(void *timer) {
    Timer *t = reinterpret_cast<Timer *>(timer);
    if (!t) return 0;
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
    return 0;
}

int bowgpu_gen_dense(int64_t row0, int64_t n, uint64_t seed, int64_t *ts_dev, double *val_dev) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    device_write_epoch_bump();
    return launch_gen_dense(c, row0, n, seed, ts_dev, val_dev);
}

int bowgpu_gen_sparse(int64_t row0, int64_t n, uint64_t seed, int64_t *ts_dev, double *val_dev, uint8_t *validity_dev) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    if (row0 & 7) return fail(BOWGPU_ERR_ARG, "row0 must be a multiple of 8");
    device_write_epoch_bump();
    return launch_gen_sparse(c, row0, n, seed, ts_dev, val_dev, validity_dev);
}

int bowgpu_stream_read_ceiling(const void *dev_a, const void *dev_b, int64_t bytes_each, double *gb_per_s) {
    if (!dev_a || !dev_b || !gb_per_s || bytes_each < (1 << 20)) return fail(BOWGPU_ERR_ARG, "two device buffers of at least 1 MiB each are needed");
    if ((reinterpret_cast<uintptr_t>(dev_a) | reinterpret_cast<uintptr_t>(dev_b)) & 15) return fail(BOWGPU_ERR_ARG, "buffers must be 16-byte aligned");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    uint64_t *dout;
    BG_TRY(scratch_at(c, kScrProbe, &dout));
    double best = 0.0;
    const int shapes[][2] = {{0, 8}, {0, 16}, {0, 32}, {1, 0}};  // {mode, workgroups per CU}
    for (const auto &sh : shapes) {
        float ms = 0;
        BG_TRY(stream_sum_run(c, dev_a, dev_b, bytes_each, sh[0], sh[1], 5, dout, &ms));
        const double gbs = 2.0 * (double)(bytes_each / 16 * 16) / (ms * 1e-3) / 1e9;
        if (gbs > best) best = gbs;
    }
    *gb_per_s = best;
    return 0;
}

int bowgpu_stream_rw_probe(const void *dev_a, const void *dev_b, int64_t bytes_each, void *out_a, void *out_b, int64_t rows_per_slot,
                             double *read_gb_per_s, double *ms_out) {
    if (!dev_a || !dev_b || !out_a || !out_b || !read_gb_per_s || bytes_each < (1 << 20) || rows_per_slot <= 0)
        return fail(BOWGPU_ERR_ARG, "two device input buffers of at least 1 MiB each and two output buffers are needed");
    if ((reinterpret_cast<uintptr_t>(dev_a) | reinterpret_cast<uintptr_t>(dev_b)) & 15) return fail(BOWGPU_ERR_ARG, "buffers must be 16-byte aligned");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    const int64_t rows = bytes_each / 4096 * 512;
    const int64_t nslots = (rows + rows_per_slot - 1) / rows_per_slot;
    double best = 0.0, best_ms = 0.0;
    for (int nt = 0; nt < 2; nt++) {
        float ms = 0;
        BG_TRY(stream_rw_run(c, dev_a, dev_b, bytes_each, out_a, out_b, rows_per_slot, nslots, nt != 0, 5, &ms));
        const double gbs = 2.0 * (double)rows * 8.0 / (ms * 1e-3) / 1e9;
        if (gbs > best) { best = gbs; best_ms = ms; }
    }
    *read_gb_per_s = best;
    if (ms_out) *ms_out = best_ms;
    return 0;
}

// diagnostic builds only (in-kernel stamps): words [first, first + n) of the calling thread's device status block
int bowgpu_debug_host_copy(void *dst, const void *src, int64_t bytes) {
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(BOWGPU_ERR_ARG, "null buffer / negative size");
    if (bytes > 0) staged_memcpy(dst, src, (size_t)bytes);
    return 0;
}

int bowgpu_debug_status(int32_t first, int32_t n, uint32_t *out, int32_t zero_after) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    // (a thread that has made no call yet has no status block to show)
    if (!out || first < 0 || n <= 0 || (size_t)(first + n) * 4 > kScrDiag.size || !c->d_scratch) return fail(BOWGPU_ERR_ARG, "bad status range");
    uint32_t *words;
    BG_TRY(scratch_at(c, kScrDiag, &words));
    BG_TRY(copy_d2h(c, out, words + first, (size_t)n * 4));
    BG_HIP(hipStreamSynchronize(c->stream));
    if (zero_after) BG_HIP(hipMemsetAsync(words + first, 0, (size_t)n * 4, c->stream));
    return 0;
}

int bowgpu_checksum64(const void *dev, int64_t n_words, uint64_t *xor_out, uint64_t *sum_out) {
    return bowgpu_checksum64_at(dev, n_words, 0, xor_out, sum_out);
}

int bowgpu_checksum64_at(const void *dev, int64_t n_words, int64_t index_base, uint64_t *xor_out, uint64_t *sum_out) {
    Ctx *c;
    BG_TRY(ctx_get(&c));
    uint64_t *dout;
    BG_TRY(scratch_at(c, kScrProbe, &dout));
    BG_TRY(launch_checksum64(c, dev, n_words, dout, (uint64_t)index_base));
    uint64_t h[2] = {0, 0};
    BG_HIP(hipMemcpyAsync(h, dout, 16, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    *xor_out = h[0];
    *sum_out = h[1];
    return 0;
}

}  // extern "C"
