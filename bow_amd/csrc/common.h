// Internal declarations shared by the HIP translation units of libbowgpu.so.
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts, 160 KB LDS per CU, 256 CUs in 8 XCDs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/bowgpu.h"
#include "bit_span.h"
#include "debug_routes.h"

namespace bowgpu {

// ---------------------------------------------------------------- errors
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);
int fail_ts_unsorted();   // BOWGPU_ERR_TS_UNSORTED: what every device path says about an interval column that is not ascending (agg_pass.cpp)
int hip_fail(hipError_t e, const char *what);
// the Arrow name of a column type as the reference's error texts spell it (bowtypes.go:89-96)
inline const char *arrow_type_name(int t) {
    return t == BOWGPU_FLOAT64 ? "float64" : t == BOWGPU_INT64 ? "int64" : t == BOWGPU_BOOLEAN ? "bool" : t == BOWGPU_STRING ? "utf8" : "undefined";
}
// a call's options: the caller's, or the defaults when it passed none
inline bowgpu_options options_or(const bowgpu_options *opts) { return opts ? *opts : bowgpu_options{0, 0, 0}; }

#define BG_HIP(expr)                                         \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(_e, #expr);    \
    } while (0)

#define BG_TRY(expr)              \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

// Counts the calls that write to or free device memory THROUGH THE LIBRARY, in any thread (bowgpu_free, bowgpu_memcpy_h2d, bowgpu_memset,
// the generators): results cached from a caller's device buffer (the Interpolate count -> fill prefix) are dropped when it moves.
uint64_t device_write_epoch();
void device_write_epoch_bump();

// test / A-B routing of the calling thread (BOWGPU_ROUTE_* bits; bowgpu_debug_set_route): never the environment
uint32_t route_mask();

// ---------------------------------------------------------------- per-thread context
struct Ctx {
    int device = 0;
    bool inited = false;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // stream in use (own or external)
    // the scratch block (device) and the registered block (pinned host memory): runtime.cpp owns the fields, ctx_blocks.h the layouts
    void *d_scratch = nullptr;
    size_t d_scratch_bytes = 0;
    void *h_pinned = nullptr;
    size_t h_pinned_bytes = 0;     // kRegBytes once allocated
    void *h_bounce = nullptr;   // two halves of pinned staging for copies of pageable caller buffers (copy_d2h / copy_h2d)
    hipEvent_t bounce_ev[2] = {nullptr, nullptr};
    bool bounce_busy[2] = {false, false};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_kernel_ms = 0.0;
    const char *last_kernel_name = "";  // the tile kernel last_kernel_ms brackets
    int64_t last_slow_rows = 0;         // rows of the last Aggregate / Interpolate call served by a kernel kept for the shapes the fast ones decline (bowgpu_last_call_slow_rows)
    // grow-only pool of temporaries reused across calls (word-aligned validity working copies, ...):
    // hipMalloc / hipFree per call cost more than the kernels' fixed overhead
    static constexpr int kPoolSlots = 40;   // 0..15 output validity working copies, kPoolInterp.. Interpolate / fill scratch, last: long windows
    void *pool[kPoolSlots] = {};
    size_t pool_bytes[kPoolSlots] = {};
    uint64_t pool_gen[kPoolSlots] = {};     // bumped on every ctx_pool() of the slot: lets a cached result notice that its block was handed out again
    // what bowgpu_rolling_interpolate_count leaves for the _fill call that follows it on the same (unchanged) columns: the
    // per-trip prefix of exact window heads, so that the interval column is not scanned a second time (interpolate_api.cpp)
    struct InterpCache {
        bool valid = false;
        const void *ts_values = nullptr;
        int64_t ts_offset = 0, n = 0, interval = 0, raw_offset = 0;
        bool sharded = false;
        int64_t global_s0 = 0, left_ts = 0;
        int has_left = 0;
        uint64_t gen = 0, gen0 = 0;         // pool_gen of the two prefix blocks when they were written
        uint64_t epoch = 0;                 // device_write_epoch() when it was written: any write / free through the library since then drops it
        // What pass 1 found (interpolate_api.cpp interp_prepare): the plan's pieces, then InterpParams' kq / drop / wbase / kq_empty /
        // e0 and M = output rows - input rows.  An InterpJob holds the same struct: count -> fill hands it over in one assignment.
        // (inclusive is a KEY field of the cache, not a finding: it sits here because the members keep their places)
        struct Found {
            int64_t s0 = 0, W = 0, first_ts = 0, last_ts = 0, offset_norm = 0, kq = -1, drop = 0, M = 0, wbase = 0;
            int kq_empty = 0, inclusive = 0, e0 = 0;
        } found;
    } interp_cache;
    void *d_params = nullptr;      // 4 KB device block holding the kernels' descriptor struct
    // what an Interpolate _count over an interval column WITH NULLS leaves for its _fill (interp_null_ts.cpp NullTsState: device temporaries);
    // freed through null_ts_cache_free by the fill, bowgpu_trim, bowgpu_set_device and at thread exit
    void *null_ts_cache = nullptr;
    void (*null_ts_cache_free)(void *) = nullptr;
    double prof_sync_begin = 0, prof_sync_end = 0;   // BOWGPU_CALL_PROFILE: around the one synchronisation of a tile pass (job_pass_complete)
};
void ctx_drop_null_ts_cache(Ctx *c);
int ctx_get(Ctx **out);                       // initialises HIP on first use; fails loudly without a GPU; settles and drops a pass in flight unless an owner calls
// the pass bowgpu_shard_pass_begin left in flight on the calling thread (runtime.cpp holds the slot, shard_api.cpp knows what is in it)
void pending_set(void *pass, void (*destroy)(void *));   // (overwrites: the caller has dropped or collected what was there)
void *pending_get();
void pending_drop(Ctx *c);                    // synchronises the stream, then destroys
struct PendingOwnerScope { bool was; PendingOwnerScope(); ~PendingOwnerScope(); };   // the two owners: ctx_get leaves the pass to them
int ctx_scratch(Ctx *c, size_t bytes, void **dptr);   // for scratch_at / registered_at (below) and runtime.cpp alone
int ctx_pinned(Ctx *c, void **hptr);
int ctx_params(Ctx *c, void **dptr);
int ctx_pool(Ctx *c, int slot, size_t bytes, void **dptr);

// ---------------------------------------------------------------- temp device buffers
// RAII device allocation (stream-ordered free at scope exit after a sync by the caller).
// Device scratch of one call.  Blocks come from / go back to a small per-thread cache (runtime.cpp devbuf_*), so a call pays
// neither hipMalloc nor hipFree (which also synchronises the device) once the sizes have been seen; every entry point
// synchronises its stream before its DevBufs go out of scope.
void devbuf_release(void *p, size_t cap);
void devbuf_cache_drop();
int devbuf_acquire(size_t n, void **p, size_t *cap);
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;  // requested
    size_t cap = 0;    // size of the underlying block
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap) { o.p = nullptr; o.bytes = 0; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { if (p) devbuf_release(p, cap); p = o.p; bytes = o.bytes; cap = o.cap; o.p = nullptr; o.bytes = 0; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { if (p) devbuf_release(p, cap); }
    int alloc(size_t n);
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---------------------------------------------------------------- dev_cols.cpp: caller buffers in and out of the device
// the device address of registered host memory; nullptr: not registered - the error text says so, naming `what` (BOWGPU_ERR_ARG)
const void *host_mapped(const void *p, const char *what);
// n bits from bit `offset` of a caller's byte buffer - a validity bitmap, a Boolean column's values - as aligned 32-bit words on
// the device, at any byte address and any offset: read in place (device, registered) or uploaded into `own` (pageable)
struct DevBits {
    const uint32_t *words = nullptr;   // 4-byte aligned
    int64_t bit0 = 0;                  // bit index (from words) of row 0
    int64_t nwords = 0;                // readable 32-bit words at `words`
    DevBuf own;                        // .p: the bits were staged
};
int stage_bits(Ctx *c, const uint8_t *bytes, int64_t offset, int64_t n, int32_t residency, const char *what, DevBits *out);
// a Boolean column's value bits and - where it has a bitmap to read - its validity bits (the 8-byte rule is for 8-byte values)
struct DevBoolCol { DevBits t, v; };
int devboolcol_prepare(Ctx *c, const bowgpu_col *col, DevBoolCol *out);

// A column of 8-byte values made device-resident: aliases the caller's pointers (BOWGPU_DEVICE, BOWGPU_HOST_PINNED) or owns an
// uploaded copy (BOWGPU_HOST).  values points at element `offset` already; validity is kept as stage_bits gives it.
struct DevCol {
    const void *values = nullptr;      // element 0 of the logical array
    const uint32_t *vbits = nullptr;   // 4-byte aligned word containing bit `vbit0`
    int64_t vbit0 = 0;                 // bit index (from vbits) of logical row 0
    int64_t vwords = 0;                // number of readable 32-bit words at vbits
    int64_t length = 0;
    int64_t null_count = 0;            // exact (counted on device if the caller said -1)
    int32_t type = 0;
    DevBuf own_values, own_validity;
};
int devcol_prepare(Ctx *c, const bowgpu_col *col, DevCol *out, bool need_values, bool need_validity);
int count_nulls_device(Ctx *c, DevCol *dc);

// An output column on the device: aliases the caller's buffers or owns temporaries that are
// copied back by finish().  The validity is always a word-aligned working copy of temp_bits_bytes(); bit_values: the values are
// bit-packed too (a BOOLEAN output) and assembled the same way, ceil(slots / 8) bytes of each copied back.
struct DevOut {
    void *values = nullptr;
    uint8_t *validity = nullptr;
    bool bit_values = false;
    DevBuf own_values, own_validity;
    bowgpu_out *user = nullptr;
};
// copies of caller buffers: pageable ones through the context's pinned staging, registered ones (BOWGPU_HOST_PINNED) directly
int copy_d2h(Ctx *c, void *dst, const void *src, size_t bytes, bool registered = false);
int copy_h2d(Ctx *c, void *dst, const void *src, size_t bytes, bool registered = false);
void staged_memcpy(void *dst, const void *src, size_t n);   // the CPU side of those copies: large ones split over the helper threads
// checks in this order: capacity, empty (nothing else is looked at), buffers, residency, alignment
int devout_prepare(Ctx *c, bowgpu_out *out, int64_t slots, DevOut *d, int pool_slot = -1, bool bit_values = false);
int devout_finish(Ctx *c, DevOut *d, int64_t slots, int32_t type, int64_t null_count, bool copy_bitmap = true);

// ---------------------------------------------------------------- frame_cols.cpp: what the frame-level operations share on the host
// (Bow.SortByCol, Bow.Filter: once the key is sorted / the mask built, both move the rows of every column of a frame into the caller's
// bowgpu_out columns, kMoveCols columns a launch)
constexpr int kMoveCols = 4;          // columns moved per launch (the permutation / the bitmap is read once per group)
struct MoveCols {                     // the columns of one launch, as gather_kernel and filter_scatter_kernel read them
    int32_t ncols, _pad;
    const uint64_t *values[kMoveCols];
    const uint32_t *vbits[kMoveCols];            // nullptr: no nulls
    int64_t vbit0[kMoveCols];
    uint64_t *out_values[kMoveCols];
    unsigned long long *out_valid[kMoveCols];    // 8-byte aligned, ceil(count / 64) words (the working copy of devout_prepare,
                                                 // temp_bits_bytes(ceil(count / 8)), always holds them)
};
bool movable_type(int32_t t);         // Int64 / Float64
bool residency_ok(int32_t r);
// nulls of a column where that is known without the device (host-resident bitmaps are counted here); -1: ask the device
int64_t host_count_nulls(const bowgpu_col *col);
// a column whose bitmap has to be read: it has one, and its null count is not stated to be 0
bool has_bitmap(const bowgpu_col &col);
// the column as the kernels that read the bitmap anyway want it staged: an unknown null count is NOT counted first
bowgpu_col uncounted(const bowgpu_col &col);
// the per-column checks of a frame of n rows, in the order the entry points report them.  Filter's form (residencies = true) reports a
// negative length before a differing one and checks the residencies; Sort's leaves both to the key's checks and to devcol_prepare
int frame_cols_checks(const bowgpu_col *cols, int32_t ncols, int64_t n, bool residencies);
// output columns for `slots` rows each; slots < 0: the count is not known yet (Filter) - residency and capacity must make sense
int outs_checks(const bowgpu_out *outs, int32_t ncols, int64_t slots);
// a caller's side buffer (`what`: "index", "mask") on the device: as is, through its registration, or staged into *own
int aux_in(Ctx *c, const void *p, size_t bytes, int32_t residency, const char *what, const void **dptr, DevBuf *own);
// a device buffer as the only column of a frame without nulls (what the scatter and the argsort take)
bowgpu_col device_col(const void *values, int64_t n, int32_t type);
// ... as a key: that column and its prepared form, the pair argsort_device and the join's count take
struct DeviceKey {
    bowgpu_col col;
    DevCol dev;
    DeviceKey(const void *values, int64_t n, int32_t type);
};
bool any_device_out(const bowgpu_out *outs, int32_t n);   // some output column is device-resident (the write epoch moves with the call)
void out_empty(bowgpu_out *out, int32_t type);            // an output column of a result without rows
template <class TypeOf> void outs_empty(bowgpu_out *outs, int32_t n, TypeOf type_of) {   // ... n of them, column i of type type_of(i)
    for (int32_t i = 0; i < n; i++) out_empty(&outs[i], type_of(i));
}
// a result buffer handed to the caller: dst in device memory is src itself or gets a device-to-device copy (and the write epoch moves)
int aux_out(Ctx *c, void *dst, const void *src, size_t bytes, int32_t residency);
int synced(Ctx *c, int rc);            // rc - a failure only after the stream has drained: the call's kernels may still be running on its work buffers
void kernel_done(Ctx *c, const char *name);   // last_kernel_ms = what ev0 .. ev1 bracket; name must outlive the call
// columns a call has staged before it moves the frame (Sort: the key; Filter: the predicate columns), by frame column
struct StagedCols {
    DevCol dc[BOWGPU_FILTER_MAX_PREDS];
    int32_t col[BOWGPU_FILTER_MAX_PREDS];
    int n = 0;
    DevCol *add(int32_t c) { col[n] = c; return &dc[n++]; }   // (to be filled in by devcol_prepare)
    const DevCol *find(int32_t c) const {
        for (int i = 0; i < n; i++) if (col[i] == c) return &dc[i];
        return nullptr;
    }
};
// One group of up to kMoveCols columns from frame column g0 on.  prepare: stages the inputs `have` lacks, prepares the outputs for
// `count` slots, fills cols.  The caller launches and reads its counts (kScrMoveCounts of the scratch block) back.  finish:
// devout_finish of every output + the group's one synchronise.  Both report a failure
// through synced().  A group's staged inputs and
// output temporaries go back when the MoveGroup does: before the next group's are taken.
struct MoveGroup {
    MoveCols cols;
    DevCol staged[kMoveCols];
    DevOut douts[kMoveCols];
};
int move_group_prepare(Ctx *c, const bowgpu_col *cols, int32_t ncols, int32_t g0, const StagedCols &have, bowgpu_out *outs, int64_t count, MoveGroup *g);
// the second half of prepare alone, for a call whose inputs are not one column each (AppendBows: a list of pieces): ncols, the
// outputs; the caller describes its inputs to its kernel itself
int move_group_outputs(Ctx *c, int32_t ncols, int32_t g0, bowgpu_out *outs, int64_t count, MoveGroup *g);
int move_group_finish(Ctx *c, MoveGroup *g, const bowgpu_col *cols, int32_t g0, int64_t count, const int64_t *null_counts);

// The one size rule of device temporaries that hold rows of a frame.  Values: 8 bytes a row + 16, the margin devcol_prepare's
// uploads carry too, against the kernels' 16-byte loads (the sites this rule replaced added 0, 8 or 16; none is known to need it).
// Bitmap: temp_bits_bytes() of bit_span.h.
inline size_t temp_values_bytes(int64_t rows) { return (size_t)rows * 8 + 16; }
// A frame of device temporaries: `rows` slots by ncols columns that live only in HBM, filled by one call (which takes `outs`)
// and read by the next (which takes as_cols).  A caller whose fill writes bitmaps in place rounds `rows` up itself.
struct DevFrame {
    std::vector<DevBuf> values, bits;
    std::vector<bowgpu_out> outs;     // the frame as output columns of `rows` slots; the filling call leaves length / null_count / type
    int alloc(Ctx *c, int32_t ncols, int64_t rows, bool zero_bits);   // zero_bits: for a fill that only sets bits (one memset a column, no synchronise)
    // The first n <= rows rows of the filled frame as input columns, types from schema.  The bitmap pointer always stays and the
    // null count is carried (0 for n == 0): every reader of such a column - devcol_prepare, has_bitmap, and through them
    // gather_frame, stage_rows and the aggregate's checks - looks at a bitmap only where `validity && null_count != 0`, so a
    // column without nulls reads like one without a bitmap.  (plan_make alone asks a bitmap that is there for row 0 and the last
    // row before it reads them; it finds them valid and computes the same plan.)
    void as_cols(const bowgpu_col *schema, int64_t n, bowgpu_col *cols) const;
    // on the owning thread: the blocks go back to THAT thread's (device's) cache.  What the fill reported in outs stays, the pointers do not
    void clear();
};
// Rows [a, b) of a column of any residency (device-resident: on device src_dev) into two buffers of the current device dst_dev, on
// its stream: values from an 8-row boundary of the source buffer, so that one Arrow offset serves values and bits, and - where the
// column has a bitmap to read - the validity bytes that cover the rows, in a zeroed, padded block.  *out: the piece as a
// device-resident column (null_count -1 with a bitmap, else 0).  Host and registered sources go through copy_h2d, the same device
// through hipMemcpyAsync, another device through hipMemcpyPeerAsync.  No synchronise
int stage_rows(Ctx *c, int dst_dev, int src_dev, const bowgpu_col &sc, int64_t a, int64_t b, DevBuf *values, DevBuf *bits, bowgpu_col *out);
// the nulls among the first n bits of a device bitmap (32-bit aligned): popcount through the context scratch, read back, synchronised
int recount_nulls(Ctx *c, const void *bits, int64_t n, int64_t *nulls);
// column i of a filled temporary frame, n rows, handed to the caller's output column (pool_slot: devout_prepare's); synchronises
int temp_to_caller(Ctx *c, const DevFrame &f, int32_t i, int64_t n, int32_t type, int64_t null_count, bowgpu_out *out, int pool_slot);

// ---------------------------------------------------------------- division by the interval
// Granlund–Montgomery round-up method (N = 64): exact floor(n / d) for every 0 <= n < 2^64.
struct MagicDiv {
    uint64_t m;
    uint32_t sh1, sh2;
};
MagicDiv magic_make(uint64_t d);

// ---------------------------------------------------------------- window plan (host side)
struct Plan {
    int64_t interval = 0;
    int64_t offset = 0;    // normalised
    int64_t s0 = 0;
    int64_t W = 0;
    int64_t first_ts = 0, last_ts = 0;
    MagicDiv magic{};
};
int plan_make(Ctx *c, const bowgpu_col *ts, int64_t interval, int64_t raw_offset, Plan *p);
bool kind_needs_inclusive(int kind);
int kind_type(int kind);
bool kind_never_nil(int kind);
bool kind_reads_values(int kind);

// fan_call.cpp: one Rolling.Aggregate over the devices of bowgpu_set_devices (*done = false: not a call for it, nothing was touched)
int multi_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
                    const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, bowgpu_agg_info *info, bool *done);
int multi_interpolate_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const Plan &plan, int opt_inclusive, bool strict,
                                const bowgpu_interp *interps, int32_t ninterps, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                                bowgpu_agg_info *info, bool *done);

// aggregate_api.cpp, for bowgpu_rolling_aggregate_sharded (sharded_call.cpp): the checks of bowgpu_rolling_aggregate that need no column data
// (interval column type, interval, aggregators) plus the shard protocol's own (Mode, at most 16 aggregators) - host only
int sharded_validate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_agg *aggs, int32_t naggs);
// nulls of an interval column (counted on the calling thread's device when the caller said -1)
int ts_null_rows(Ctx *c, const bowgpu_col *ts, int64_t *nulls);
// the callers that take no null in the interval column: BOWGPU_ERR_TS_NULLS when it has one; the column on the device, its bitmap left out
int ts_contract(Ctx *c, const bowgpu_col *tsc);
int ts_device(Ctx *c, const bowgpu_col *tsc, DevCol *dts);

// shard.hip: the tail of a rank of bowgpu_rolling_aggregate_sharded that does not own its last output slot (one lane per output)
struct ShardTailArgs {
    uint64_t *values[BOWGPU_CARRY_MAX_AGGS];
    uint8_t *validity[BOWGPU_CARRY_MAX_AGGS];
    uint8_t *report;     // host-mapped block: byte i = whether output i's slot was valid
    int64_t slot;
    int32_t n;
};
int launch_shard_tail(Ctx *c, const ShardTailArgs &a);

// ---------------------------------------------------------------- kernels (rolling_agg.hip)
constexpr int kMaxCols = 8;    // value columns reduced per launch
constexpr int kMaxAggs = 16;   // output columns per launch

struct AggDesc {
    int32_t kind;
    int32_t slot;        // index into AggParams::cols (value column), -1 for ts-only reducers
    int32_t out_type;    // BOWGPU_FLOAT64 / BOWGPU_INT64
    int32_t n_factors;
    double factors[BOWGPU_MAX_FACTORS];
    void *out_values;
    uint32_t *out_valid; // nullptr when the reducer never yields nil (WindowStart/Sum/Count/NumRows)
};

struct ColDesc {
    const void *values;
    const uint32_t *vbits;  // nullptr => no nulls
    int64_t vbit0;
    int64_t vwords;
    int32_t type;
    int32_t need_ts;        // some reducer of this column integrates over time
};

enum : uint32_t { kPassNeedVals = 1, kPassMinMax = 2, kPassFirstLast = 4, kPassNullable = 8 };

struct AggParams {
    const int64_t *ts;
    int64_t n;              // rows in this launch's column slice
    int64_t row_base;       // global row index of ts[0] (sharding); 0 otherwise
    int64_t s0;
    int64_t interval;
    int64_t W;              // windows addressable in the outputs
    int64_t wid_base;       // global window id of output slot 0 (sharding); 0 otherwise
    MagicDiv magic;
    uint32_t m32, sh1_32, sh2_32;  // 32-bit form of the same division (valid when fits32)
    int32_t fits32;         // interval < 2^32: tiles whose ts span fits 32 bits use 32-bit window arithmetic
    int32_t inclusive;      // effective Options.Inclusive
    int32_t ncols;
    int32_t naggs;
    int32_t _pad0;
    int32_t pre_rows;       // s0 > ts[0] (negative ts + truncating division): rows below s0 ride in window 0
    ColDesc cols[kMaxCols];
    AggDesc aggs[kMaxAggs];
    // per column-slot pass summary (index = slot + 1; index 0 is the "no column" pass), precomputed on the host so
    // the kernels do not scan the aggregator list per tile
    uint32_t pass_mask[kMaxCols + 1];   // bit a set: aggregator a belongs to this pass
    uint32_t pass_flags[kMaxCols + 1];  // kPass* bits
    int32_t first_pass_slot, last_val_slot, n_nullable_max;
    int32_t bits_preset;    // output bitmaps start as all-ones (rolling_simple.hip): the long-window path clears empties instead of setting valids
    // status block in device memory
    uint32_t *status;       // kAggSt* words, [kLongCountWord ..) the long-window counts
    int64_t *long_list;     // kLongLists sub-lists of pairs (global window id, first row), long_cap pairs each
    int64_t long_cap;
};

constexpr int kSimpleMaxAggs = 16;
enum : uint32_t { kNeedStep = 1, kNeedTrap = 2, kNeedMinMax = 4, kNeedSum = 8, kNeedFirstLast = 16 };
// descriptor of rolling_simple.hip's kernel: value columns of one type, factor-free outputs, 32-bit window ids
struct SimpleParams {
    const int64_t *ts;
    int64_t n, s0, interval, W;            // s0 = start of output slot 0 (a shard: global s0 + wid_base * interval)
    int64_t wid_base;                      // global id of output slot 0 (only for the long-window queue)
    MagicDiv magic;                        // 64-bit magic of the interval: the per-tile base window of the kWide variants
    int32_t shift_k;                       // kWide: trailing zero bits of the interval; m32 / sh1 / sh2 then divide by interval >> shift_k
    uint32_t kind_mask[5];                 // outputs by class (bit a = output a): 0 Sum / Mean / First / Last, 1 Min / Max, 2 step integrals, 3 trapezoid integrals, 4 WindowStart / Count / NumRows
    uint32_t col_mask[kMaxCols];           // outputs of value column c
    uint32_t need;                         // kNeed* bits: which running statistics the outputs of the call read (set by the host: one scalar test per use in the kernels)
    uint32_t m32, sh1, sh2;
    int32_t naggs;
    int32_t ncols;                         // value columns (>= 1; reducers over the interval column use it as a column)
    int32_t inclusive;                     // rolling_tw.hip: windows are built inclusive (some reducer needs it)
    int32_t pre_rows;                      // s0 lies above the first timestamp: the rows below it ride in window 0
    uint32_t unaligned_mask;               // bit c: value column c starts on an 8-byte, not a 16-byte boundary; bit 31: the interval column
    const void *values[kMaxCols];
    const uint32_t *vbits[kMaxCols];       // nullptr: this column has no nulls
    int64_t vbit0[kMaxCols], vwords[kMaxCols];
    int32_t col_is_int[kMaxCols];          // Int64 column (read as float64(v), First / Last return Int64)
    int32_t kind[kSimpleMaxAggs];
    int32_t col[kSimpleMaxAggs];           // column slot each output reads (WindowStart / NumRows ride with slot 0)
    int32_t nfac[kSimpleMaxAggs];          // transformation.Factor chain of each output (factor.go:7-20), usually empty
    double fac[kSimpleMaxAggs][BOWGPU_MAX_FACTORS];
    uint64_t *out_values[kSimpleMaxAggs];
    uint32_t *out_valid[kSimpleMaxAggs];   // nullptr for never-nil reducers; all bitmaps are preset to ones by the host
    uint32_t *status;         // kAggSt* words, [kLongCountWord ..) the long-window counts
    int64_t *long_list;
    int64_t long_cap;
};
int launch_rolling_simple(Ctx *c, const SimpleParams &p, int need, bool is_int, bool has_nulls, bool wide, bool dense);   // dense: the larger head list (windows of < 3 rows)
bool rolling_simple_plain(const SimpleParams &p, bool is_int, bool has_nulls);   // the call takes the unpadded instantiation (short windows over one Float64 column without nulls): its small list holds 254 heads
int launch_rolling_tw(Ctx *c, const SimpleParams &p, bool is_int, bool has_nulls, bool wide, bool ts32);  // time-weighted reducers / inclusive windows (rolling_tw.hip)

// rolling_fused.hip: Interpolate -> Aggregate in one pass.  Per value column pass: the column's interpolator (what interp_device.h
// synth_value_pt reads of an InterpCol, same field names)
struct FusedCol {
    int32_t type, kind;            // BOWGPU_FLOAT64 / BOWGPU_INT64 ; BOWGPU_INTERP_*
    int32_t has_prev, prev_t_valid, prev_v_valid, next_valid;   // Options.PrevRow (linear.go:14-18, stepprevious.go:13-15); next_valid: always 0 here
    double const_value, prev_t, prev_v, next_t, next_v;
    int64_t prev_v_i64;
};
struct FusedParams {
    SimpleParams s;                // FIRST: the kernel reads the output pointers through the kernel-argument segment at SimpleParams' offsets
    FusedCol cols[kMaxCols];       // by column pass (SimpleParams::values[c])
    double inv_interval;           // (1 / interval) * (1 + 2^-40): floor(x * inv_interval) == x / interval for every x < 2^32 (rolling_fused.hip fdiv32)
};
int launch_rolling_fused(Ctx *c, const FusedParams &fp, int need, bool has_nulls);
// Interpolate + validateInterpolation (interpolate_api.cpp; reference rolling/interpolation.go:30-96)
int interp_validate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_options *o, const bowgpu_interp *interps, int32_t ninterps);

int launch_rolling_twc(Ctx *c, const SimpleParams &p, bool long_halo = false);   // (long_halo: 256 rows of look-ahead) nullable columns under time-weighted reducers, 32-bit times: the valid points compacted first (rolling_twc.hip)
constexpr int64_t kCompactLongMaxAvgRows = 255;             // ... and, with 256 rows of look-ahead, up to this many (beyond: the streaming form) - one kind of integral, First / Last
constexpr int64_t kCompactLongBothMaxAvgRows = 176;         //     both kinds of integral, Min / Max: the streaming form is ahead from 192 rows on (agg_pass.cpp compact_long_max_rows)
constexpr int64_t kCompactValuesMinAvgRows = 48;            // value reducers alone: only sums AND extrema on a nullable column, from this window length on
constexpr int64_t kCompactMinAvgRows = 12;                  // ... for calls whose windows average at least this many rows (its head list: 92 per 640 rows)
int launch_rolling_aggregate(Ctx *c, const AggParams &p);   // general kernel (rolling_agg.hip)
int launch_rolling_fast(Ctx *c, const AggParams &p);        // lean kernel for exclusive windows without time-weighted reducers (rolling_fast.hip)
constexpr int kLongChunkRows = 4096;
constexpr int kLongStreamRows = 512;  // chunk of the streaming form of the long-window reduction (long_stream.hip)
constexpr int64_t kLongOnlyAvgRows = 128;   // calls with BOTH kinds of integral whose windows average at least this many rows skip the tile kernels: streaming form (agg_pass.cpp job_run)
constexpr int64_t kLongStreamAnyAvgRows = 129;   // ... the same for every other reducer set (256 until long_short_kernel took a boundary per 128-row trip; 128 until the tile kernels' walks became branch-free: windows of exactly 128 rows fit a tile's look-ahead and the tile kernels win there)
constexpr int64_t kLongBisectAvgRows = 512; // ... bisection form where the streaming form does not apply (BOWGPU_ROUTE_LONG_CLASSIC; W >= 2^32)
constexpr int64_t kLongClassicAvgRows = 1ll << 22;   // ... and from here on the handful of giant windows go by bisection + per-window chunks
constexpr int kLongLists = 64;      // sub-lists of the long-window queue (agg_device.h push_long_window)
constexpr int kLongCountWord = 16;  // status[kLongCountWord + s] = entries in sub-list s
constexpr int kStatusWords = kLongCountWord + kLongLists;
// the words below kLongCountWord that the Aggregate kernels raise and agg_pass.cpp agg_status_error reads (Interpolate keeps a status block
// of its own whose words 5 - 7 mean other things: interpolate.hip, interpolate_api.cpp).  rolling_agg.hip, rolling_fast.hip and shard.hip spell
// them by name; the wave-tile kernels, long_windows.hip, long_stream.hip, long_device.h and agg_device.h still write the numbers (an edit to those files asks for the
// round's counter files again: tests/test_profiles_fresh.py)
constexpr int kAggStUnsorted = 0;        // the interval column is not ascending
constexpr int kAggStListOverflow = 2;    // the long-window list overflowed (agg_device.h push_long_window)
constexpr int kAggStRedo = 4;            // some tile is beyond what the wave-tile kernel that ran can describe: the call is redone (agg_pass.cpp job_pass_complete)
constexpr int kAggStFusedDeclines = 5;   // rolling_fused.hip: a far neighbour point - the call takes the two-call form
constexpr int kAggStPlanMismatch = 6;    // the preset launch: a caller's plan was not made for this interval column
constexpr int kAggStStrictTooLong = 7;   // strict_order: a window of more than 2^20 rows
struct LongListStarts { int64_t start[kLongLists + 1]; };  // prefix sums of the sub-list counts (host side)
size_t long_entry_size();
size_t long_part_size();
int stream_rw_run(Ctx *c, const void *a, const void *b, int64_t bytes_each, void *o0, void *o1, int64_t rows_per_slot, int64_t nslots, bool nt,
                  int reps, float *ms);
int stream_sum_run(Ctx *c, const void *a, const void *b, int64_t bytes_each, int mode, int blocks_per_cu, int reps, uint64_t *d_out, float *ms);
int launch_long_windows_v2(Ctx *c, const AggParams &p, const LongListStarts *starts, void *entries, int32_t *nchunks, int64_t *offsets,
                           int64_t *block_sums, int64_t *d_total, int32_t *work_entry, void *partials, int64_t max_work, bool strict = false,
                           int64_t n_given = 0);
// the queued windows of a tile pass without the host in between: grid from the queue's capacity, counts read on the device; short windows
// walked in row order, the others listed in big_entries / big_nchunks (status[kQueueBigWord] of them) for launch_long_windows_v2(n_given)
int launch_long_queue(Ctx *c, const AggParams &p, int64_t capacity, void *big_entries, int32_t *big_nchunks, int64_t walk_max_rows, bool strict);
constexpr int kQueueBigWord = 8;          // status word: windows long_queue_kernel left to the chunked machinery
constexpr int64_t kQueueWalkMaxRows = 1024;   // ... those longer than this
size_t long_stream_workspace(int64_t n, int64_t W, int ncols);
int launch_long_stream(Ctx *c, const AggParams &p, void *workspace);   // every window of the call, one read of the rows (long_stream.hip)
// its last step while windows span a few chunks: stream_final_kernel, then long_final_block_kernel for what it leaves (both compiled in long_windows.hip)
int launch_stream_final(Ctx *c, const AggParams &p, int64_t nchunks, const void *meta, const void *parts, const void *recs, const void *wparts,
                        void *entries, int64_t *off0, int64_t *off1, unsigned long long *n_leftover, int lite);
int launch_fix_tail_bits(Ctx *c, uint8_t *bitmap, int64_t nbits);
// every output bitmap of one call in one launch (rolling_agg.hip)
struct BitmapBatch {
    int32_t n, status_words;
    int64_t nbits;                 // W
    uint32_t *work[kMaxAggs];      // word-aligned working copies the kernels update
    uint8_t *user[kMaxAggs];       // finish: the caller's device buffer of ceil(W/8) bytes (nullptr: host-resident output, copied separately)
    int32_t ones[kMaxAggs];        // preset: start all-valid (else all-null)
    int32_t count[kMaxAggs];       // finish: count the valid bits into counts[a]
    uint32_t *status;              // preset zeroes status[0 .. status_words) and counts[0 .. kMaxAggs)
    unsigned long long *counts;
    char *host_block;              // finish, one workgroup per bitmap (nbits <= kFinishHostBits): registered host memory that receives the status
                                   // words [0, status_words) and, in kRegAggCounts, bitmap a's count - by the kernel's own stores
    const int64_t *check_ts;       // preset: a caller-supplied plan is checked against this interval column (nullptr: no check);
    int64_t check_n, check_first, check_last;   // status[kAggStPlanMismatch] = 1 when its first / last row are not the plan's two timestamps
};
constexpr int64_t kFinishHostBits = 262144;   // up to here ONE workgroup finishes a bitmap (32 KB: a microsecond) and can hand its count to the host itself
int launch_preset_bitmaps(Ctx *c, const BitmapBatch &b);
int launch_finish_bitmaps(Ctx *c, const BitmapBatch &b);
int launch_popcount(Ctx *c, const uint32_t *words, int64_t bit0, int64_t nbits, uint64_t *d_count);
int launch_fetch_two(Ctx *c, const int64_t *col, int64_t i0, int64_t i1, int64_t *host_out);   // host_out: registered host memory

// mode.hip: one aggregation.Mode output over the windows whose first rows are first_idx[0 .. W]
int launch_mode(Ctx *c, const int64_t *ts, const int64_t *first_idx, int64_t n, int64_t s0, int64_t interval, int64_t W, int pre_rows,
                int inclusive, const void *values,
                const uint32_t *vbits, int64_t vbit0, int is_int, const bowgpu_agg *agg, void *out_values, uint32_t *out_valid,
                int64_t *n_mid, int64_t *n_long);

// rolling_bool.hip: the value reducers of one BOOLEAN column (Arrow bit-packed values) over the same window row ranges, every
// requested one in one launch
constexpr int kBoolMaxOuts = 16;     // outputs of one launch
constexpr int kBoolLaneRows = 256;   // windows up to this many rows: one lane each; longer ones: the 64 lanes of a wavefront together
struct BoolOut {
    int32_t kind, nfac;
    double fac[BOWGPU_MAX_FACTORS];
    void *values;       // Float64 / Int64 results: W slots of 8 bytes; Boolean results (First / Last / Mode): whole 32-bit words of bits
    uint32_t *valid;    // whole 32-bit words (a word-aligned working copy)
};
struct BoolParams {
    const int64_t *ts, *first_idx;          // first_idx[W + 1]: launch_window_first_rows
    int64_t s0, n, interval, W;
    int32_t pre_rows, inclusive;
    const uint32_t *tbits, *vbits;          // value / validity words (vbits nullptr: no nulls)
    int64_t tbit0, vbit0;                   // bit of row 0 in them
    unsigned long long *null_windows;       // += windows without a valid row: the null count of every nullable output
    int32_t nouts, _pad;
    BoolOut outs[kBoolMaxOuts];
};
int launch_bool_windows(Ctx *c, const BoolParams &P);
int launch_bool_widen(Ctx *c, const uint32_t *tbits, int64_t tbit0, const uint32_t *vbits, int64_t vbit0, int64_t n, double *out, uint32_t *out_valid);

// neighbour index of a validity bitmap (interp_fill.hip nbr_index_build)
struct NbrIndex {
    const int64_t *prev_before;  // [nblocks] last valid row in any earlier block, -1 if none
    const int64_t *next_after;   // [nblocks] first valid row in any later block, -1 if none
    int64_t g0;                  // absolute block number of the column's first bit
};
// ts_nulls.hip: an interval column with nulls rewritten for the tile kernels (forward-filled timestamps, the rows that belong to a window)
// (inclusive: the keep rule of inclusive windows; plain - inclusive only - receives the interval column's validity without the rows
// that sit on a window start with a null timestamp right behind them: ts_nulls.hip)
int launch_ts_nullfill(Ctx *c, const int64_t *ts, const uint32_t *tbits, int64_t tbit0, int64_t n, const struct NbrIndex &ix, int64_t s0, int64_t interval,
                       const MagicDiv &magic, int inclusive, int64_t *ts_eff, uint64_t *keep, uint64_t *plain, unsigned long long *d_dropped);
// the outputs of IntegralTrapezoid / WeightedAverageLinear for the windows behind such rows, recomputed by a walk in the reference's order
struct QuirkFixAgg {
    const void *values; const uint32_t *vbits; int64_t vbit0;     // the reducer's input column (its own validity)
    uint64_t *out_values; uint32_t *out_valid;                    // its output: 8-byte slots, validity words (bit 0 = window 0)
    int32_t type, kind, n_factors, _pad;
    double factors[BOWGPU_MAX_FACTORS];
};
struct QuirkFix { int32_t naggs, _pad; QuirkFixAgg a[8]; };
int launch_ts_quirk_fix(Ctx *c, const int64_t *ts, const uint32_t *tbits, int64_t tbit0, int64_t n, const struct NbrIndex &ix, int64_t s0, int64_t interval,
                        const MagicDiv &magic, int64_t W, const QuirkFix &fx, unsigned long long *d_fixed);
int launch_count_to_f64(Ctx *c, uint64_t *v, const uint32_t *valid, int64_t n, int n_factors, const double *factors);   // (valid: W bits; the factors go onto the float64)
int fetch_valid(Ctx *c, const bowgpu_col *col, int64_t row, int *valid);   // (dev_cols.cpp) validity bit of one row of a column, wherever it lives
// Rolling.Interpolate over an interval column with nulls: the kept rows compacted (ts_nulls.hip)
constexpr int kMaxCompactCols = 16;
struct CompactCols {
    int32_t ncols, ts_col;
    const uint64_t *values[kMaxCompactCols]; const uint32_t *vbits[kMaxCompactCols]; int64_t vbit0[kMaxCompactCols];   // the call's columns
    uint64_t *out_values[kMaxCompactCols];      // their kept rows
    uint64_t *lookup_bits[kMaxCompactCols];     // validity of the compacted call's columns (nullptr: the interval column - dense)
    uint64_t *patch_values[kMaxCompactCols]; uint32_t *patch_valid[kMaxCompactCols];   // the outputs interp_patch_kernel corrects
    uint64_t *ts_bits;                          // inclusive iteration: which compacted rows have a timestamp (nullptr: not wanted)
};
// the interpolators of the call + the both-valid bitmaps of the compacted columns with their neighbour indices: what interp_patch_kernel
// needs to make the synthetic row of a window that begins behind null rows (inclusive iteration)
struct PatchInterps {
    int64_t m;
    const uint64_t *both_bits[kMaxCompactCols];
    NbrIndex nbr[kMaxCompactCols];
    int32_t type[kMaxCompactCols], kind[kMaxCompactCols], has_prev[kMaxCompactCols], prev_t_valid[kMaxCompactCols], prev_v_valid[kMaxCompactCols];
    double const_value[kMaxCompactCols], prev_t[kMaxCompactCols], prev_v[kMaxCompactCols];
    int64_t prev_v_i64[kMaxCompactCols];
};
int launch_keep_counts(Ctx *c, const uint64_t *keep, int64_t nw, int32_t *counts);
int launch_compact_rows(Ctx *c, const uint64_t *keep, const int64_t *base, int64_t n, const int64_t *ts_eff, const uint32_t *tbits, int64_t tbit0,
                        const uint64_t *plain, const CompactCols &cc, int64_t *marker, uint32_t *flags);
int launch_pack_flags(Ctx *c, const uint32_t *flags, int64_t m, const CompactCols &cc, uint64_t *marker_bits);
int launch_interp_patch(Ctx *c, const int64_t *marker_out, const uint32_t *marker_valid, int64_t m_out, const uint32_t *flags, const CompactCols &cc,
                        const PatchInterps &px);
int launch_and_bits(Ctx *c, const uint32_t *a, int64_t abit0, const uint32_t *b, int64_t bbit0, int64_t n, uint64_t *out);

// shard.hip
int launch_range_state(Ctx *c, const AggParams &p, int mode, uint64_t wid, const bowgpu_carry_state *d_seeds,
                       bowgpu_carry_state *d_states_out, const bowgpu_next_row *d_next, int seed_alive, int strict);

int launch_fill_empty(Ctx *c, const AggParams &p, int64_t slot0, int64_t slot1);

// interp_fill.hip
int launch_window_first_rows(Ctx *c, const int64_t *ts, int64_t n, const Plan &plan, int64_t *first_idx, uint32_t *status);
int launch_exclusive_scan(Ctx *c, const int32_t *in, int64_t n, int64_t *out, int64_t *block_sums, int64_t *d_total);
int launch_col_order(Ctx *c, const uint64_t *values, const uint32_t *vbits, int64_t vbit0, int64_t n, int32_t type, uint32_t *d_flags);
int launch_window_bounds(Ctx *c, const int64_t *ts, int64_t n, const Plan &plan, int inclusive, int pre_rows,
                         const int64_t *first_idx, int64_t *first_index, int64_t *slice_begin, int64_t *slice_end, uint8_t *is_incl);
int whole_run(Ctx *c, const void *params_blob, int64_t nblocks);
int whole_final_run(Ctx *c, const void *partials, int64_t nblocks, int64_t nrows, int64_t first_value, int64_t last_value,
                    const void *final_blob);
size_t stats_size();

// Neighbour index of one validity bitmap: for every block of kNbrBlockBits bits (absolute bit positions, so blocks are
// word-aligned whatever the Arrow offset) the nearest valid ROW before the block and after it.  Bounds every
// previous/next-valid lookup to one block of words + one table read, however long the runs of nulls are.
constexpr int kNbrBlockBits = 4096;
constexpr int kPoolMode = 17;    // aggregation.Mode: its output's validity working copy
constexpr int kPoolColOrder = 18; // IsColSorted: one (first valid, last valid) record per 512-row trip
constexpr int kPoolShard = 19;   // shard stitch: the record's states, the seeds and the next shard's first row
constexpr int kPoolGaps = 32;    // window_first_rows: queued runs of empty windows
constexpr int kPoolWhole = 33;        // bowgpu_aggregate_whole: partial states, the reducers' values and validity bytes
constexpr int kPoolInterpEdge = 31;   // Interpolate: the trips' edge words (interp_wave3_kernel)
constexpr int kPoolInterp = 20;  // context pool slots 20..30: tile counts, their scan, scan sums, one neighbour index per column
constexpr int kPoolAppend = 34;  // AppendBows: the piece table of one launch group
// every user its own slot: 0..15 the outputs' validity working copies, 17..19, 20..30 (kPoolInterp + 0..10), 31, 32, 33, 34, kPoolSlots - 1 the long windows
static_assert(kPoolAppend > kPoolWhole && kPoolAppend < Ctx::kPoolSlots - 1, "context pool slots must be distinct");
static_assert(kPoolMode != kPoolColOrder && kPoolColOrder != kPoolShard && kPoolMode != kPoolShard && kPoolMode > 15 && kPoolShard < kPoolInterp &&
              kPoolInterp + 10 < kPoolInterpEdge && kPoolInterpEdge < kPoolGaps && kPoolGaps < kPoolWhole && kPoolWhole < Ctx::kPoolSlots - 1,
              "context pool slots must be distinct");
// kernel parameter blocks of interp_fill.hip (filled by interpolate_api.cpp, fill_api.cpp and whole_api.cpp, passed by value)
struct InterpCol {
    const uint64_t *values;
    const uint32_t *vbits;
    int64_t vbit0;
    int32_t type;
    int32_t kind;
    double const_value;
    int32_t has_prev, prev_t_valid, prev_v_valid, _pad;
    double prev_t, prev_v;
    int64_t prev_v_i64;
    uint64_t *out_values;
    uint32_t *out_valid_words; // output validity bitmap (zeroed by the host before the launch)
    NbrIndex nbr;              // of this column's bitmap (Linear / StepPrevious look their neighbours up through it)
    int32_t next_valid, _pad2; // sharded Interpolate: the nearest valid point on the shards to the right (Linear)
    double next_t, next_v;
};
struct InterpParams {
    const int64_t *ts;
    int64_t n, s0, interval, W;
    MagicDiv magic;
    const int32_t *tile_local;         // pass 1 of interpolate.hip: per 256 rows, the exact heads in the earlier rows of the same super-tile
    const int64_t *super_before;       // ... and per super-tile of kInterpSuperRows rows, the exact heads in all earlier super-tiles
    uint32_t *status;                  // [0] |= 1: interval column not ascending; [1]: window kq has no row of its own
    int64_t kq;                        // index of the window that starts at -1 (the reference's "no first value" sentinel), else -1
    int64_t drop;                      // leading rows that belong to no window (interp_quirk_kernel), normally 0
    uint32_t m32, sh1_32, sh2_32;      // 32-bit magic of the interval (fast32 only)
    int32_t fast32;                    // interp_fast32(plan, kq): 32-bit window ids, integer exact-head test
    int32_t has_left, wide32;          // wide32: interp_wide32() - interp_wave3_kernel's trip-relative form applies (fast32 implies it); sharded Interpolate: rows exist on shards to the left, the last of them at left_ts;
    int64_t left_ts, wbase;            // the windows up to theirs (wbase = its id + 1) are not this shard's to account for
    int32_t ncols, ts_col;
    int32_t allow_wave2;               // the whole-trip wave kernel may take the call (0: the call is being redone after its run list overflowed)
    int32_t kq_empty;                  // window kq has no row of its own (pass 1's finding)
    int32_t inclusive, e0;             // Options.Inclusive (interp_wave2 / wave3 kernels only); e0: row 0 sits exactly on the first window's start
    int64_t n_out;                     // rows the call is to produce (n + what the count pass found): interp_wave3_kernel's last trip checks that it ends there
    uint64_t *edge_words;              // interp_wave3_kernel: [ncols][trips of 512 rows] - a trip's bits of the bitmap word it shares with the trip before it
    uint32_t *trip_valid;              // interp_wave3_kernel: [ncols][trips] valid outputs per trip (nullptr: not kept - a pass over the bitmaps counts them)
    unsigned long long *valid_counts;  // ... summed by interp_edge_fix_kernel into [ncols][kInterpEdgeBlocks] partial counts
    uint32_t *host_status;             // in place: registered host memory that interp_edge_fix_kernel copies the 16 status words into (valid_counts then lies there too)
    int32_t in_place, aligned16;       // aligned16: ts and every input column's values are 16-byte aligned (interp_wave3_kernel's vector loads unconditional); out_valid_words ARE the caller's bitmaps and nobody zeroed them: every word of [0, n_out) gets stored
    InterpCol cols[kMaxCols];
};
int64_t interp_tiles(int64_t n);
bool interp_fast32(const Plan &plan, int64_t kq);
bool interp_wide32(const Plan &plan, int64_t kq);   // ... without the bound on the frame's span: 32-bit arithmetic relative to each trip
void interp_magic32(int64_t interval, uint32_t *m, uint32_t *sh1, uint32_t *sh2);   // the 32-bit magic divisor of an interval < 2^32 (also agg_pass.cpp: job_build, simple_params_build)
constexpr int kInterpSuperRows = 8192;
constexpr int kInterpEdgeBlocks = 128;   // interp_edge_fix_kernel: workgroups (= partial valid-output counts) per column
int64_t interp_supers(int64_t n);
// pass 1: tile_local [ceil(n/256)] + super_sum [supers] (scratch) + super_before [supers + 1] + *d_total; two launches
int launch_interp_count(Ctx *c, const int64_t *ts, int64_t n, const Plan &plan, int64_t kq, int has_left, int64_t left_ts,
                        int32_t *tile_local, int32_t *super_sum, int64_t *super_before, int64_t *d_total, uint32_t *status,
                        int64_t *host_back /* registered host memory: [0] total, [1], [2] the four status words */);
int launch_interp_tiles(Ctx *c, const InterpParams &p);
bool interp_takes_wave3(const InterpParams &p);   // (with p.allow_wave2 set) - that kernel needs no neighbour index on its first attempt
enum { kFillLinear = -1 };  // FillParams::method; >= 0: BOWGPU_FILL_PREVIOUS / NEXT / MEAN
struct FillParams {
    const uint64_t *ref_values; const uint32_t *ref_vbits; int64_t ref_vbit0; int32_t ref_type;  // FillLinear only
    const uint64_t *fill_values; const uint32_t *fill_vbits; int64_t fill_vbit0; int32_t fill_type;
    int32_t method;
    int64_t n;
    uint64_t *out_values;
    uint32_t *out_valid_words;   // 8-byte aligned, a multiple of 64 bits long
    unsigned long long *valid_count;  // += valid output rows
    NbrIndex nbr;                // of the fill column's bitmap; prev_before == nullptr: not built - the kernel then looks at most 2048
                                 // rows beyond a trip's ends and raises *far_flag when that does not reach (the host repeats the call with the index)
    uint32_t *far_flag;
};
// builds the index of (vbits, vbit0, n) into `work` (nbr_index_bytes(n, vbit0) bytes of device memory)
int launch_first_last_valid(Ctx *c, const uint32_t *vbits, int64_t vbit0, int64_t n, int64_t *d_rows);
size_t nbr_index_bytes(int64_t n, int64_t vbit0);
int nbr_index_build(Ctx *c, const uint32_t *vbits, int64_t vbit0, int64_t n, void *work, NbrIndex *out);
int fill_run(Ctx *c, const FillParams &p);
struct WholeParamsH {
    const int64_t *ts;
    const uint64_t *values;
    const uint32_t *vbits;
    int64_t vbit0;
    int64_t n;
    int32_t type;
    int32_t need_ts;
    void *partials;
    int64_t chunk;
};
struct WholeFinalH {
    int32_t kind, out_type, col_is_int, n_factors;
    double factors[BOWGPU_MAX_FACTORS];
    uint64_t *out_value;
    uint8_t *out_valid_byte;
};

struct WholeFinishH {
    const int64_t *ts;
    int64_t nrows;
    int32_t n, _pad;
    int32_t slot[kMaxAggs];
    WholeFinalH f[kMaxAggs];
    uint64_t *host_values;    // registered host memory
    uint8_t *host_valid;
};
int whole_value_run(Ctx *c, const void *params_blob, int64_t nblocks);
int whole_finish_run(Ctx *c, const void *partials, int64_t nblocks, const WholeFinishH &fin);

// sort.hip: Bow.SortByCol - stable LSD radix argsort over (key image, 32-bit row index) pairs, and the gather (host side: sort_api.cpp)
constexpr int kSortTileRows = 4096;   // rows per scatter tile: one 256-entry digit histogram each
struct GatherArgs {
    MoveCols cols;                               // out_valid: ceil(n_idx / 64) words, every one stored whole by its wave
    int64_t n_idx, length;                       // rows to produce; rows of the source columns
    unsigned long long *null_counts;             // [kMoveCols], zeroed by the host
    uint32_t *bad;                               // |= 1: a caller's index outside [0, length)
};
// what the join's gather takes: an index of -1 is "no row" (a null output slot), and on such rows the column key_slot reads a second
// source - the other frame's key - through idx2.  Passed to that instantiation alone: the other two take GatherArgs as it is
struct GatherNoRowArgs : GatherArgs {
    const int32_t *idx2;                         // [n_idx] source row of the second source, -1: none
    const uint64_t *values2;
    const uint32_t *vbits2;
    int64_t vbit02;
    int32_t key_slot, _pad;                      // -1: no column of this launch has a second source
};
// workgroups of a grid-stride kernel over n rows
inline int64_t stream_grid(int64_t n, int threads) {
    int64_t grid = (n + threads - 1) / threads;
    if (grid > 256 * 8) grid = 256 * 8;
    return grid < 1 ? 1 : grid;
}
// hist: [8][256] digit counts, flags: [0] not ascending, [1] NaN seen (both zeroed by the host); img_out: nullable
int launch_sort_hist(Ctx *c, const uint64_t *key, int64_t n, int is_float, uint32_t *d_hist, uint32_t *d_flags, uint64_t *img_out);
// one stable pass on digit `shift / 8`.  mode 0 / 1: src holds raw Int64 / Float64 keys, 2: images; src_idx == nullptr: row i carries index i.
// tile_hist: 256 * ceil(n / kSortTileRows) words; sums: ceil(that / 4096) words
int launch_sort_pass(Ctx *c, const uint64_t *src, int mode, const uint32_t *src_idx, int64_t n, int shift, uint32_t *tile_hist, uint32_t *sums,
                     uint64_t *dst, uint32_t *dst_idx);
// sort_api.cpp: the sorted (image, row index) pairs of one key column
struct SortWork {
    DevBuf keys[2], idx[2], tiles, sums;
    int cur = 0;                 // which of the two buffers holds the result
    int passes = 0;              // radix passes run (8 - passes: digits that are the same in every key)
    const uint32_t *perm() const { return idx[cur].as<const uint32_t>(); }
};
int argsort_device(Ctx *c, const bowgpu_col *key, const DevCol &dk, SortWork *w, int32_t *sorted);
inline int argsort_device(Ctx *c, const DeviceKey &k, SortWork *w, int32_t *sorted) { return argsort_device(c, &k.col, k.dev, w, sorted); }
// out[i] = idx[i] as 64 bits: idx32 (row numbers) zero-extended, else idx32s sign-extended (-1 stays -1)
int launch_widen(Ctx *c, const uint32_t *idx32, const int32_t *idx32s, int64_t n, int64_t *out);
// The index of a gather, exactly one of three: u32 (the library's own permutation: trusted), i64 (a caller's indices: range-checked,
// *bad), i32 (the join's: -1 = no row, else in range).  With i32, frame column key_col (-1: none) reads *key2 through i32_2 on the
// rows where i32 says "no row"
struct GatherIdx {
    const uint32_t *u32 = nullptr;
    const int64_t *i64 = nullptr;
    const int32_t *i32 = nullptr, *i32_2 = nullptr;
    int32_t key_col = -1;
    const DevCol *key2 = nullptr;
};
// gather_kernel's instantiation for ix (the second-source fields of `a` are read with ix.i32 alone)
int launch_gather(Ctx *c, const GatherNoRowArgs &a, const GatherIdx &ix);
// sort_api.cpp, next to argsort_device: the host side of every gather (Sort, take, Distinct, Join).
// the launch half of a gather of the columns `cols` (frame columns g0 ..) of `length` rows: the scratch words zeroed, the kernel, ev1
// recorded behind it (no synchronise)
int gather_enqueue(Ctx *c, const MoveCols &cols, int32_t g0, int64_t length, const GatherIdx &ix, int64_t n_idx);
// ... over a prepared group, then the outputs' null counts and *bad (synchronises)
int gather_launch(Ctx *c, const MoveGroup &g, int32_t g0, int64_t length, const GatherIdx &ix, int64_t n_idx, int64_t *nulls, bool *bad);
// the columns of a frame, kMoveCols a launch, gathered through ix into outs.  *bad: an index outside the frame - nothing of that
// group was handed out
int gather_frame(Ctx *c, const bowgpu_col *cols, int32_t ncols, const StagedCols &have, const GatherIdx &ix, int64_t n_idx, bowgpu_out *outs,
                 bool *bad);

// exclusive scan of m 32-bit counts in place (their total below 2^32); sums: ceil(m / 4096) words of scratch
int launch_scan_u32(Ctx *c, uint32_t *v, int64_t m, uint32_t *sums);

// filter.hip: Bow.Filter - value-set predicates into a row bitmap, ordered compaction of the selected rows (host side: filter_api.cpp)
constexpr int kFilterTileRows = 4096;   // rows per tile: 64 mask words, one selected count
struct FilterPredDev {
    const uint64_t *values;
    const uint32_t *vbits;               // nullptr: no nulls
    int64_t vbit0;
    int32_t n_values, match_null, is_float, _pad;
    uint64_t set[BOWGPU_FILTER_MAX_VALUES];   // raw 64-bit payloads of the column's type; compared with wave-uniform operands
};
// what a mask pass leaves for filter_stats_kernel, the scan and filter_scatter_kernel (filter_mask_kernel and the kernels of frame_ops.hip)
struct TileRecords {
    unsigned long long *mask;            // 64 * ceil(n / kFilterTileRows) words, every one stored (rows >= n: clear bits)
    uint32_t *tile_counts;               // ceil(n / kFilterTileRows)
    uint32_t *tile_spans;                // ... per tile: lowest | highest << 16 selected row of the tile (tile-relative)
    uint32_t *stats;                     // 4 words zeroed by the host (filter_stats_kernel)
    uint32_t *host_stats;                // registered host memory: receives [0] selected rows, [1] lowest, [2] highest selected row
};
struct FilterMaskArgs {
    int64_t n;
    int32_t npreds, _pad;
    const uint8_t *and_mask;             // nullable: bit i (LSB first) of byte i / 8; any alignment
    TileRecords t;
    FilterPredDev preds[BOWGPU_FILTER_MAX_PREDS];
};
struct FilterScatterArgs {
    MoveCols cols;                       // out_valid: ceil(selected / 64) words, zeroed by the host
    int64_t n;
    const unsigned long long *mask;      // as filter_mask_kernel left it
    const uint32_t *tile_base;           // the scanned tile counts
};
int launch_filter_mask(Ctx *c, const FilterMaskArgs &a);
int launch_filter_stats(Ctx *c, const TileRecords &t, int64_t ntiles);   // (launch_filter_mask ends with it)
int launch_filter_scatter(Ctx *c, const FilterScatterArgs &a);
// filter_api.cpp: the bitmap of one call, its tile records and the columns staged for the mask pass (kept for the scatter that follows)
struct MaskWork {
    DevBuf mask, tiles, spans, sums, staged_mask;
    StagedCols pcols;
    const uint32_t *back = nullptr;      // where filter_stats_kernel stores the three numbers
    int64_t selected = 0, first = -1, last = -1;
};
int mask_work_prepare(Ctx *c, int64_t n, MaskWork *w, TileRecords *t);   // the buffers of a mask pass over n rows, its stats words zeroed
int mask_work_collect(Ctx *c, MaskWork *w);                              // synchronises; selected / first / last
// frame_ops_api.cpp: the rows of one column that hold a value, as a finished mask pass: its own validity through valid_mask_kernel,
// the stats (w->selected), the tile counts scanned in place.  *t: the mask and the scanned counts, for the caller's scatter or split
int valid_rows_scanned(Ctx *c, const DevCol &dk, MaskWork *w, TileRecords *t);
int scatter_device(Ctx *c, const bowgpu_col *cols, int32_t ncols, int64_t n, MaskWork *w, bowgpu_out *outs);
int mask_work_compact(Ctx *c, const bowgpu_col *cols, int32_t ncols, int64_t n, MaskWork *w, const char *mask_kernel, bowgpu_out *outs,
                      int64_t *first, int64_t *count, int32_t *contiguous);

// frame_ops.hip: Bow.DropNils / Bow.Diff / Bow.Distinct - the three kernels in front of the scan, the scatter and the sort
// (host side: frame_ops_api.cpp)
constexpr int kValidMaskCols = 8;       // bitmaps ANDed per launch of valid_mask_kernel
struct ValidMaskArgs {
    int64_t n;
    int32_t ncols, accumulate;           // accumulate: AND into the mask words an earlier launch of the same call left
    const uint8_t *and_mask;             // nullable, as in FilterMaskArgs
    const uint32_t *vbits[kValidMaskCols];
    int64_t vbit0[kValidMaskCols], vwords[kValidMaskCols];
    TileRecords t;
};
int launch_valid_mask(Ctx *c, const ValidMaskArgs &a);   // (without the stats kernel: the caller launches it after the last group)
struct DiffArgs {
    MoveCols cols;                       // out_valid: ceil(n / 64) words, every one stored whole
    int64_t n;
    uint32_t float_mask, _pad;           // bit c: column c is Float64
};
int launch_diff(Ctx *c, const DiffArgs &a);
// s: n keys in non-descending order of Buffer.Less (raw Int64 / Float64 payloads, no NaN); flags the last row of each group of equals
int launch_distinct_tail(Ctx *c, const uint64_t *s, int64_t n, int is_float, const TileRecords &t);

// convert.hip: Bow.Convert among Int64, Float64 and Boolean (host side: convert_api.cpp).  One launch takes up to kMoveCols columns,
// each with its own length and its own (source, target) pair.
constexpr int kConvertShards = 64;       // a column's count of valid rows is added up in this many words: thousands of waves adding
                                         // into ONE word are served one after the other, ~10 ns each, and that tail outlasts a bitmap copy
struct ConvertCol {
    const void *src;                     // row 0 of the 8-byte values; a Boolean source: the aligned words of its value bits
    int64_t sbit0, swords;               // a Boolean source: bit index (from src) of row 0, readable 32-bit words at src
    const uint32_t *vbits;               // nullptr: no nulls
    int64_t vbit0, vwords;
    void *out_values;                    // 8-byte slots; a Boolean target: ceil(n / 64) 64-bit words, every one stored whole
    unsigned long long *out_valid;       // ceil(n / 64) words, every one stored whole (the working copy of devout_prepare)
    int64_t n;
    int32_t from, to;                    // BOWGPU_INT64 | BOWGPU_FLOAT64 | BOWGPU_BOOLEAN
};
struct ConvertArgs {
    ConvertCol col[kMoveCols];
    unsigned long long *valid_counts;    // [kMoveCols][kConvertShards], zeroed by the host: valid rows of each column, to be summed
    int64_t max_n;                       // the longest column of the launch
    int32_t ncols, _pad;
};
int launch_convert(Ctx *c, const ConvertArgs &a);

// append.hip: AppendBows / Bow.Find - the concatenation of the pieces of a frame and the linear search of a column (host side:
// append_api.cpp)
struct AppendPiece {                     // one piece of one column, addressed by OUTPUT row
    const uint64_t *values;              // values[row] is output row `row` (the piece's element 0 minus the piece's start row)
    const uint32_t *vbits;               // nullptr: no nulls to look at
    int64_t vadj;                        // bit (vadj + row) of vbits is output row `row`'s
};
struct AppendArgs {
    MoveCols cols;                       // ncols, out_values, out_valid (ceil(n / 64) words, every one stored whole); the inputs are the pieces'
    int64_t n;                           // rows of the result
    int32_t npieces;
    uint32_t bitmap_mask;                // bit c: some piece of column c has a bitmap to read
    const uint32_t *starts;              // [npieces + 1] first output row of each piece; starts[npieces] = n
    const AppendPiece *pieces[kMoveCols];   // [npieces] per column of the launch
};
size_t append_table_bytes(int32_t npieces);   // starts + kMoveCols piece arrays, each 16-byte aligned, in one block
int launch_append(Ctx *c, const AppendArgs &a);
// append_api.cpp (also the destination side of the sharded sort).
// the piece table of one launch group in host memory, laid out as the device block is: starts, then kMoveCols arrays of pieces
struct PieceTable {
    std::vector<char> bytes;
    size_t pieces_at = 0;
    int32_t npieces = 0;
    explicit PieceTable(int32_t n) : bytes(append_table_bytes(n), 0), pieces_at(((((size_t)n + 1) * 4) + 15) & ~(size_t)15), npieces(n) {}
    uint32_t *starts() { return reinterpret_cast<uint32_t *>(bytes.data()); }
    AppendPiece *pieces(int i) { return reinterpret_cast<AppendPiece *>(bytes.data() + pieces_at) + (size_t)i * (size_t)npieces; }
    size_t pieces_offset(int i) const { return pieces_at + (size_t)i * (size_t)npieces * sizeof(AppendPiece); }
};
// one group of up to kMoveCols columns of the pieces frames[f][g0 ..]: every piece staged (copies of BOWGPU_HOST pieces are kept in
// *staged until the group is done), the table built and uploaded, one append launch into g's outputs, and the counts of valid rows of
// the columns marked in count_on_device on their way to valid[kMoveCols] (no synchronise)
int append_launch(Ctx *c, const bowgpu_col *const *frames, int32_t nframes, int32_t g0, int64_t total, const MoveGroup &g,
                  std::vector<DevCol> *staged, PieceTable *t, const bool *count_on_device, unsigned long long *valid);
constexpr uint32_t kFindNone = 0xFFFFFFFFu;
struct FindArgs {
    const uint64_t *values;              // nullptr: the search for the first null (bitmaps only)
    const uint32_t *vbits;
    int64_t vbit0, vwords;
    int64_t n, row_start;
    uint64_t value;                      // raw payload of the column's type
    int32_t is_float, _pad;
    uint32_t *result;                    // device word, kFindNone on entry: lowered to the lowest matching row
    uint32_t *host_result;               // registered host memory: receives *result behind the search
};
int launch_find(Ctx *c, const FindArgs &a);   // presets *result, searches, hands the word to host_result

// equal.hip: the per-row half of Bow.Equal and the Prev / Next valid-row getters (host side: equal_api.cpp)
struct BitsAt {                          // n bits read where they lie, as stage_bits gives them
    const uint32_t *words;               // nullptr: nothing to read
    int64_t bit0, nwords;
};
enum : int32_t { kEqualBits = 0, kEqualIeee = 1, kEqualBool = 2 };
struct EqualCol {                        // one column of both frames: [0] left, [1] right
    const uint64_t *values[2];           // 8-byte values (kEqualBits / kEqualIeee)
    BitsAt truth[2];                     // kEqualBool: the value bits
    BitsAt valid[2];                     // words == nullptr: no nulls to look at
    int32_t kind, col;                   // how valid rows compare; the column's index in the frame
};
constexpr uint64_t kEqualNone = ~0ull;
struct EqualArgs {
    int32_t ncols, _pad;
    int64_t n;
    unsigned long long *result;          // device word, kEqualNone on entry of the CALL: lowered to (row << 32) | column of the first difference
    EqualCol col[kMoveCols];
};
int launch_equal_preset(Ctx *c, unsigned long long *result);
int launch_equal(Ctx *c, const EqualArgs &a);   // one group of columns; the word is kept
int launch_equal_result(Ctx *c, const unsigned long long *result, unsigned long long *host_result);
struct ValidRowArgs {
    int32_t ncols, direction;            // +1: the first row >= row_start, -1: the last row <= row_start, where every bitmap has its bit set
    int64_t n, row_start;                // 0 <= row_start < n
    BitsAt valid[BOWGPU_VALID_ROW_MAX_COLS];
    uint32_t *result;                    // device word, kFindNone (-1 as a signed row) on entry
    uint32_t *host_result;               // registered host memory
};
int launch_valid_row(Ctx *c, const ValidRowArgs &a);   // presets *result, searches, hands the word to host_result

// join.hip: Bow.InnerJoin / OuterJoin - the left-ordered lookup join on one probe key per side: a call's one key pair, or the surrogates
// of several (join_keys.hip, join_host.h).  Host side: join_api.cpp
struct JoinStats {                       // one device block of a call, zeroed by the host
    unsigned long long pairs;            // length of the reference's commonRows
    unsigned long long matched_left;     // left rows with at least one match
    uint32_t nan, left_null;             // a NaN among the valid left keys; a null left key
    uint32_t _pad[2];
};
// the rows of a mask pass as 32-bit row numbers, in row order: set bits -> set_rows (and values[row] -> set_values), clear bits of rows
// below n -> clear_rows; each of the three may be nullptr.  mask / tile_base: as filter_scatter_kernel takes them (scanned counts)
int launch_join_split_rows(Ctx *c, const unsigned long long *mask, const uint32_t *tile_base, int64_t n, const uint64_t *values, uint32_t *set_rows,
                           uint64_t *set_values, uint32_t *clear_rows);
struct JoinRightArgs {
    const uint32_t *perm;                // nullptr: the keys are in order as they lie
    const uint32_t *vrows;               // nullptr: the key has no null - position p is row p
    const uint64_t *keys;                // the valid keys in row order (read when img_out is given)
    uint64_t *img_out;                   // nullptr: the sort left the images
    uint32_t *index;                     // [rn + rv]: the second part is written here
    int64_t rn, rv;
    int32_t is_float, _pad;
};
int launch_join_right_index(Ctx *c, const JoinRightArgs &a);
struct JoinProbeArgs {
    const uint64_t *keys;                // the left key
    const uint32_t *vbits;               // nullptr: no nulls
    int64_t vbit0, n;
    const uint64_t *simg;                // [rv] sorted images of the right key's values
    int64_t rn, rv;
    uint32_t *first, *count, *out_count; // [n]: range in the right index; rows the left row becomes (the scan's input)
    uint8_t *head;                       // [rv], zeroed: 1 at the first position of every matched group of equals
    JoinStats *stats;
    int32_t is_float, outer;
};
int launch_join_probe(Ctx *c, const JoinProbeArgs &a);
// bit `row` of bits (zeroed, 32-bit words) |= the right row occurs in no pair; index / simg / head as above
int launch_join_unmatched(Ctx *c, const uint32_t *index, const uint64_t *simg, const uint8_t *head, const JoinStats *stats, int64_t rn, int64_t rv,
                          uint32_t *bits);
struct JoinExpandArgs {
    const uint32_t *starts;              // [n_left] scanned out_count; nullptr: left row i is output row i, without a right row
    const uint32_t *first, *count, *index;
    const uint32_t *tail_rows;           // [rows - rows_left] right rows of the tail; nullptr: 0, 1, 2, ...
    int64_t n_left, rows_left, rows;
    int32_t *out_l, *out_r;              // [rows]: -1 = no row
    int32_t outer, _pad;
};
int launch_join_expand(Ctx *c, const JoinExpandArgs &a);

// sort_shard.hip: Bow.SortByCol over row-range shards - the splitter search over a rank's sorted key and the stable merge of the
// sorted runs a destination rank has pulled (host side: sort_shard_api.cpp)
constexpr int kShardMaxWorld = 64;
constexpr int kMergeTileRows = 2048;   // output rows per workgroup of merge_runs_kernel (also what one merge_partition_kernel thread answers for)
// how a sorted key is read: raw Int64 / raw Float64 payloads of a key that lies in order (imaged on the fly, key_image.h), or images
enum : int32_t { kKeyRawInt = 0, kKeyRawFloat = 1, kKeyImages = 2 };
struct SplitBoundsArgs {
    const uint64_t *keys;                // n sorted keys, read as `mode` says
    int64_t n;
    int32_t mode, ncand;
    uint64_t cand[kShardMaxWorld];       // candidate images
    uint32_t *out;                       // [2 * ncand]: rows with an image below cand[j], rows with an image <= cand[j]
};
int launch_split_bounds(Ctx *c, const SplitBoundsArgs &a);
struct ImageAtArgs {
    const uint64_t *keys;
    int32_t mode, npos;
    uint32_t pos[2 * kShardMaxWorld + 2];   // rows of keys, each below the key's length
    uint64_t *out;                          // [npos] their images
};
int launch_image_at(Ctx *c, const ImageAtArgs &a);
// img[i] = image of keys[i] (raw payloads, no NaN), idx[i] = i: the runs of a staging frame before their first merge round
int launch_merge_init(Ctx *c, const uint64_t *keys, int64_t n, int is_float, uint64_t *img, uint32_t *idx);
// one round: adjacent runs merged pairwise, stable (on equal images the left run's rows come first).  start[0 .. nruns]: first row of
// each run, start[nruns] = rows in all; an unpaired last run is copied.  part: one word per tile of scratch
struct MergeRoundArgs {
    const uint64_t *img_in;
    const uint32_t *idx_in;
    uint64_t *img_out;
    uint32_t *idx_out;
    uint32_t *part;                      // [tiles of the round <= rows / kMergeTileRows + pairs]: rows of the LEFT run among the outputs in front of the tile
    int32_t npairs, ntiles;
    uint32_t start[kShardMaxWorld + 1];          // start[2j], start[2j + 1], start[2j + 2]: pair j
    uint32_t tile0[kShardMaxWorld / 2 + 1];      // first tile of pair j; tile0[npairs] = ntiles
};
int launch_merge_round(Ctx *c, MergeRoundArgs *a, int nruns);  // fills npairs / ntiles / tile0 from start[0 .. nruns], launches both kernels and the copy

// generate.hip
int launch_gen_dense(Ctx *c, int64_t row0, int64_t n, uint64_t seed, int64_t *ts, double *val);
int launch_gen_sparse(Ctx *c, int64_t row0, int64_t n, uint64_t seed, int64_t *ts, double *val, uint8_t *validity);
int launch_checksum64(Ctx *c, const void *dev, int64_t n, uint64_t *d_out2, uint64_t index_base = 0);

}  // namespace bowgpu

// ---------------------------------------------------------------- the two per-thread blocks: their layouts, and the way into them
#include "ctx_blocks.h"

namespace bowgpu {

// *p = region r of the calling thread's scratch block / registered block.  Nothing else hands out a pointer into either
template <class T> int scratch_at(Ctx *c, Region r, T **p) {
    void *base;
    BG_TRY(ctx_scratch(c, r.end(), &base));
    *p = reinterpret_cast<T *>(static_cast<char *>(base) + r.offset);
    return 0;
}
template <class T> int registered_at(Ctx *c, Region r, T **p) {
    void *base;
    BG_TRY(ctx_pinned(c, &base));
    *p = reinterpret_cast<T *>(static_cast<char *>(base) + r.offset);
    return 0;
}

}  // namespace bowgpu
