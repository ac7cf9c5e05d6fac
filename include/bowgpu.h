/*
 * bowgpu.h — C ABI of the MI355X-native rolling-window aggregation path for Metronlab/bow.
 *
 * This is the drop-in boundary: the entry points a cgo shim inside the
 * reference's `rolling` package would bind (INTEGRATION.md shows that shim).  Plain C99,
 * plain pointers and sizes, no exceptions, no torch / HIP types.  Every function returns
 * 0 on success or a negative BOWGPU_ERR_* code; bowgpu_last_error() gives the message
 * (thread-local).  Nothing here ever falls back to a CPU implementation: if the HIP
 * runtime or a GPU is missing the call fails with BOWGPU_ERR_NO_DEVICE.
 *
 * Column layout is Arrow's, exactly as bow holds it (reference bowseries.go:59-83,
 * bowgetters.go:46-63): values = Data().Buffers()[1], validity = Data().Buffers()[0]
 * (LSB-first bits, bit i <-> buf[i>>3] & (1<<(i&7)); NULL => all valid), both indexed
 * from Data().Offset().  Buffers are borrowed for the duration of the call only.
 */
#ifndef BOWGPU_H
#define BOWGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (round 4): bowgpu_options' former padding word is `strict_order` (a caller that left it uninitialised now gets the row-order forms),
 * bowgpu_stream_rw_ceiling became bowgpu_stream_rw_probe, the BOWGPU_ROUTE_* bits moved.  A binding checks bowgpu_abi_version()
 * against the value it was written for when it loads the library (bow_amd/capi.py lib(); shim/go/rolling/gpu_cgo.go init()). */
/* 5 (round 5): bowgpu_rolling_interpolate_aggregate added; bowgpu_last_kernel_name() spells rolling_simple_kernel with its template
 * arguments; bowgpu_agg_info gained nothing (same layout). */
/* 6 (round 6): bowgpu_set_devices / bowgpu_get_devices / bowgpu_set_fanout_min_rows added (one call over several devices); no struct
 * changed. */
/* 7: the one-call-per-phase shard entry points bowgpu_shard_{span, aggregate, carry_only, fix_first, first_row} and the
 * bowgpu_shard_carry struct removed (the shard record protocol is the one sharded Aggregate); no remaining struct changed. */
/* 8: bowgpu_rolling_aggregate_sharded added (one Rolling.Aggregate over row-range shards held on several devices); no struct
 * changed. */
/* 9: bowgpu_argsort / bowgpu_take / bowgpu_sort_by_col added (Bow.SortByCol on the device) and BOWGPU_ERR_SORT_NULLS with them; no struct
 * changed. */
/* 10: bowgpu_filter_mask / bowgpu_compact / bowgpu_filter and the bowgpu_filter_pred struct added (Bow.Filter on the device); no existing
 * struct changed. */
/* 11: bowgpu_valid_mask / bowgpu_drop_nils / bowgpu_diff / bowgpu_distinct added; 12: bowgpu_append / bowgpu_find_next added; 13: bowgpu_join_rows /
 * bowgpu_join added (Bow.InnerJoin / OuterJoin on the device); no existing struct changed. */
/* 14: bowgpu_sort_by_col_sharded and bowgpu_sort_by_col_sharded_info (with the bowgpu_sort_shard_info struct) added: Bow.SortByCol over
 * row-range shards held on several devices; no existing struct changed. */
/* (still 14): bowgpu_parquet_write, with the bowgpu_parquet_write_options and bowgpu_parquet_write_info structs, added under the same
 * version: a new entry point and two new structs, nothing existing changed its layout or meaning. */
/* (still 14): bowgpu_convert (Bow.Convert among Int64, Float64 and Boolean) added under the same version: a new entry point, no struct
 * added or changed. */
/* (still 14): bowgpu_parquet_write_codec (the writer with a compression codec, SNAPPY compressed on the device) added under the same
 * version: a new entry point beside bowgpu_parquet_write, whose options struct and behaviour stay as they are. */
/* (still 14): bowgpu_join_keys_rows / bowgpu_join_keys and BOWGPU_JOIN_MAX_KEYS (the join on several common columns) added under the same
 * version: two new entry points beside bowgpu_join_rows / bowgpu_join, no struct added or changed. */
/* (still 14): bowgpu_equal (with the bowgpu_equal_info struct), bowgpu_valid_row and bowgpu_is_col_empty (Bow.Equal's rows, the Prev / Next
 * valid-row getters, IsColEmpty) added under the same version: three new entry points and one new struct, nothing existing changed. */
/* (still 14): bowgpu_parquet_read_bool_column and bowgpu_parquet_bool_column_check (a Parquet BOOLEAN column decoded on the device into a
 * bit-packed Boolean column) added under the same version: two new entry points beside bowgpu_parquet_read_column /
 * bowgpu_parquet_column_check, which keep declining a BOOLEAN column as before; BOWGPU_PARQUET_ENC_RLE added to the encoding bits. */
/* (still 14): bowgpu_parquet_write_bool (the writer with BOWGPU_BOOLEAN columns admitted, written as Parquet BOOLEAN columns) added under
 * the same version: a new entry point beside bowgpu_parquet_write / bowgpu_parquet_write_codec, which keep declining a Boolean column as
 * before; no struct added or changed. */
#define BOWGPU_ABI_VERSION 14

/* bow.Type (reference bowtypes.go:17-32) */
enum {
    BOWGPU_UNKNOWN = 0,
    BOWGPU_FLOAT64 = 1,
    BOWGPU_INT64 = 2,
    BOWGPU_BOOLEAN = 3,            /* Arrow bit-packed values.  Accepted as a VALUE column of bowgpu_rolling_aggregate and
                                      bowgpu_rolling_aggregate_planned (see there), as source or target of bowgpu_convert and as a
                                      column of bowgpu_equal (bowgpu_valid_row / bowgpu_is_col_empty read bitmaps alone) and of
                                      bowgpu_parquet_write_bool; what bowgpu_parquet_read_bool_column gives; every other entry point
                                      declines it */
    BOWGPU_STRING = 4,             /* not accepted by the device path */
    BOWGPU_INPUT_DEPENDENT = 5,
    BOWGPU_ITERATOR_DEPENDENT = 6
};

/* where a buffer lives */
enum {
    BOWGPU_HOST = 0,   /* ordinary (pageable) host memory - Go heap / malloc: staged through HBM by the call */
    BOWGPU_DEVICE = 1, /* HBM of the current device (bowgpu_malloc or any hipMalloc'd pointer) */
    BOWGPU_HOST_PINNED = 2  /* host memory page-locked and mapped for the device with bowgpu_host_register (or hipHostMalloc /
                               hipHostRegister): INPUT columns are read by the kernels where they lie - zero-copy over PCIe, no staging
                               copy, no HBM footprint; OUTPUT columns are produced in HBM and leave by one asynchronous DMA each */
};

/* error codes; the Go shim maps them back to the reference's error strings */
enum {
    BOWGPU_OK = 0,
    BOWGPU_ERR_INTERVAL = -1,        /* "strictly positive interval required"            rolling/rolling.go:115-117 */
    BOWGPU_ERR_TS_TYPE = -2,         /* "impossible to create a new intervalRolling ..."  rolling/rolling.go:70-73 */
    BOWGPU_ERR_FIRST_TS_NULL = -3,   /* "the first value of the column should be ..."     rolling/rolling.go:89-93 */
    BOWGPU_ERR_NO_AGG = -4,          /* "at least one column aggregation is required"    rolling/aggregation.go:148-150 */
    BOWGPU_ERR_KEEP_INTERVAL = -5,   /* "must keep interval column '%s'"                 rolling/aggregation.go:163-166 */
    BOWGPU_ERR_BAD_COL = -6,         /* "no column '%s'"                                 bowgetters.go:323 */
    BOWGPU_ERR_TYPE = -7,            /* type whitelist                                   rolling/interpolation.go:82-93 */
    BOWGPU_ERR_NOT_SORTED = -8,      /* FillLinear: "refColIndex '%d' is empty or not sorted" bowfill.go:39-42 */
    BOWGPU_ERR_UNSUPPORTED = -9,     /* input outside the device path's contract (see each function) */
    BOWGPU_ERR_ARG = -10,
    BOWGPU_ERR_NO_DEVICE = -11,      /* no HIP device / runtime: the product path has no CPU fallback */
    BOWGPU_ERR_HIP = -12,            /* a HIP call failed; message has the hipError string */
    BOWGPU_ERR_TS_NULLS = -13,       /* interval column has nulls AND the call has Mode, reads a Boolean column or is sharded (or, Rolling.Interpolate on inclusive
                                        windows: a row on a window start has null timestamps behind it and then an EQUAL timestamp, or sits on
                                        -1): the device path declines (caller keeps the reference path); Aggregate and Interpolate are served
                                        otherwise. */
    BOWGPU_ERR_TS_UNSORTED = -14,    /* interval column not ascending: device path declines.  The remedy on the device is bowgpu_sort_by_col
                                        (Bow.SortByCol, what the reference's users run in front of a Rolling); no rolling call sorts on its own */
    BOWGPU_ERR_OOM = -15,
    BOWGPU_ERR_SORT_NULLS = -16      /* "column to sort by has %d nil values"            bowsort.go:11-15 */
};

/* One Arrow array as bow holds it.  Replaces per-element Bow.GetInt64/GetFloat64/GetValue
 * (reference bowgetters.go:155-247) with bulk buffer access. */
typedef struct bowgpu_col {
    const void *values;       /* int64 / float64 little-endian, 8-byte aligned; BOWGPU_BOOLEAN: the Arrow bit-packed buffer (bit offset + i,
                                 LSB first), addressed like `validity`: any byte alignment */
    const uint8_t *validity;  /* may be NULL (all valid) */
    int64_t offset;           /* arrow Data.Offset(): slices share buffers (bow.go:279-283) */
    int64_t length;           /* Data.Len() */
    int64_t null_count;       /* Data.NullN(); -1 = unknown (the library counts) */
    int32_t type;             /* BOWGPU_FLOAT64 | BOWGPU_INT64 | BOWGPU_BOOLEAN (Rolling.Aggregate value columns, bowgpu_convert) */
    int32_t residency;        /* BOWGPU_HOST | BOWGPU_DEVICE | BOWGPU_HOST_PINNED */
} bowgpu_col;

/* Output column: caller-owned storage for `length` slots — what bow.NewBuffer(W, typ)
 * (bowbuffer.go:22-40) would allocate: 8*length value bytes and ceil(length/8) validity
 * bytes.  The call fills both (null slots hold 0, as in the reference) and sets
 * null_count so the shim can wrap them with bow.NewSeries(name, typ, data, validity)
 * (bowseries.go:27-29).
 * A BOOLEAN result (First / Last / Mode over a Boolean column) is bit-packed like its validity: `values` holds ceil(length / 8)
 * bytes, bit k is slot k's value, null slots hold 0, and the padding bits of the last byte of both buffers are clear.  No byte
 * past ceil(W / 8) is written in either buffer, whatever the residency or the alignment (device pointers need no alignment). */
typedef struct bowgpu_out {
    void *values;
    uint8_t *validity;
    int64_t length;           /* in: capacity in slots (>= W); out: slots produced */
    int64_t null_count;       /* out */
    int32_t type;             /* out: resolved return type (rolling/aggregation.go:110-121) */
    int32_t residency;        /* in */
} bowgpu_out;

/* Built-in reducers: one per constructor of reference rolling/aggregation/<name>.go */
enum {
    BOWGPU_AGG_WINDOW_START = 0,       /* windowstart.go:8-13 */
    BOWGPU_AGG_SUM = 1,                /* sum.go:8-25 */
    BOWGPU_AGG_MEAN = 2,               /* arithmeticmean.go:8-30 */
    BOWGPU_AGG_MIN = 3,                /* minmax.go:8-31 */
    BOWGPU_AGG_MAX = 4,                /* minmax.go:33-56 */
    BOWGPU_AGG_COUNT = 5,              /* count.go:8-20 */
    BOWGPU_AGG_FIRST = 6,              /* firstlast.go:8-21 */
    BOWGPU_AGG_LAST = 7,               /* firstlast.go:23-36 */
    BOWGPU_AGG_INTEGRAL_STEP = 8,      /* integral.go:40-69 */
    BOWGPU_AGG_INTEGRAL_TRAPEZOID = 9, /* integral.go:8-38, NeedInclusiveWindow */
    BOWGPU_AGG_WAVG_STEP = 10,         /* weightedmean.go:8-20 */
    BOWGPU_AGG_WAVG_LINEAR = 11,       /* weightedmean.go:22-34, NeedInclusiveWindow */
    BOWGPU_AGG_NUM_ROWS = 12,          /* float64(w.Bow.NumRows()): the closure of aggregation_test.go:28-31 */
    BOWGPU_AGG_MODE = 13,              /* mode.go:8-32 (not mergeable: unsharded calls only) */
    BOWGPU_AGG__COUNT = 14
};

#define BOWGPU_MAX_FACTORS 4

/* One rolling.ColAggregation (rolling/aggregation.go:40-50) restricted to the built-in
 * kinds, with its transformation.Factor chain (rolling/transformation/factor.go:7-20). */
typedef struct bowgpu_agg {
    int32_t kind;
    int32_t col;                         /* input column index: what SetInputIndex receives (aggregation.go:181) */
    int32_t n_factors;                   /* 0..BOWGPU_MAX_FACTORS */
    int32_t _pad;
    double factors[BOWGPU_MAX_FACTORS];  /* applied in order to the reducer's result (aggregation.go:216-221) */
} bowgpu_agg;

/* rolling.Options (rolling/rolling.go:49-53); PrevRow travels with the interpolators. */
typedef struct bowgpu_options {
    int64_t offset;
    int32_t inclusive;
    int32_t strict_order;       /* not in the reference.  != 0: every window is reduced in the reference's left-to-right row order - no
                                   order-free form, Sum / ArithmeticMean / Integral* / WeightedAverage* bit for bit, and
                                   bowgpu_agg_info.long_windows is 0 on success.  Windows that a tile cannot hold (longer than its
                                   128-row look-ahead) are walked by one lane each (round 4; round 3 declined them): 0.25 - 0.48 of
                                   the HBM peak at 1000-row windows.  A window of more than 2^20 rows makes the call
                                   BOWGPU_ERR_UNSUPPORTED (one lane per window: beyond that it would take milliseconds each).
                                   Honoured by bowgpu_rolling_aggregate[_planned], by bowgpu_rolling_interpolate_aggregate and (round 5) by
                                   the shard record protocol - bowgpu_shard_begin / _pass_begin / _finish: a window shared by TWO ranks
                                   is re-walked by the right rank seeded with the left rank's running state, i.e. in row order across
                                   the boundary; a window spread over three or more ranks, or a boundary window of more than 2^20
                                   rows, is BOWGPU_ERR_UNSUPPORTED.  0: see bowgpu_agg_info.long_windows for the bound that
                                   applies */
} bowgpu_options;

/* Diagnostics of one aggregate call */
typedef struct bowgpu_agg_info {
    int64_t s0;                 /* first window start (rolling.go:95-99) */
    int64_t num_windows;        /* W (rolling.go:143-154) */
    int32_t new_interval_col;   /* index of the LAST aggregator reading the interval column (aggregation.go:152-161) */
    int32_t inclusive;          /* effective Options.Inclusive after validateAggregation (aggregation.go:183-185) */
    int64_t long_windows;       /* windows reduced in an ORDER-FREE form instead of the reference's left-to-right walk: windows longer
                                   than a tile's look-ahead (128 rows), and every window of a call whose windows average >= 129 rows (128 for calls with both kinds of integral).  THE STATED TOLERANCE, for the float sums
                                   of those windows (u = 2^-53, n = the window's rows, x = its valid values, T = its time-weighted
                                   terms):   |Sum - ref| <= 2 (n + 2) u SUM|x_i|;   ArithmeticMean: that / count + 2 u |ref|;
                                   Integral*: 4 (n + 2) u SUM|T_i| (a Factor scales it);   WeightedAverage*: that / (t_last - t_first)
                                   + 2 u |ref|.  A bound on SUM|x|, not on |ref|: a window whose values cancel may differ from the
                                   reference in every digit of a result near zero (tests/tolerance.py states and asserts it, a
                                   cancelling window included).  The summation tree is fixed: equal inputs give equal bits.  Every
                                   other reducer, and every window when this is 0, is bit-exact.  bowgpu_options.strict_order
                                   walks those windows in row order instead.
                                   WHAT "BIT-EXACT" EXCLUDES, everywhere in this header: the sign and payload of a NaN that the
                                   arithmetic itself GENERATES (inf - inf, 0 * inf, 0 / 0 in a Sum, a mean, an integral, an
                                   interpolated value).  gfx950 produces the positive default NaN 0x7FF8000000000000 where x86 - the
                                   reference's Go on amd64 - produces the negative "real indefinite" 0xFFF8000000000000; Go prints
                                   both as NaN and no operation on this path tells them apart.  A NaN that comes FROM THE INPUT keeps
                                   its bits (payload and sign) through First / Last / Min / Max / fills / interpolation copies, and a
                                   NaN operand propagates through an addition as on x86 (quieted, payload kept). */
    double kernel_ms;           /* device time of the kernels of this call (HIP events on the library stream) */
} bowgpu_agg_info;

/* ---- library / device ------------------------------------------------------------- */
int bowgpu_abi_version(void);
const char *bowgpu_last_error(void);
int bowgpu_device_count(int *count);
int bowgpu_set_device(int device);          /* per calling thread; default device 0 */
int bowgpu_device_name(char *buf, int cap);
/* ONE call, N devices (reference rolling/aggregation.go:123-145 - the user makes one Aggregate call).  Process-wide:
 * after bowgpu_set_devices(ids, n >= 2) every bowgpu_rolling_aggregate / _planned / _interpolate_aggregate call of any thread whose interval
 * column holds at least 2 x min_rows rows is cut into up to n row ranges (multiples of 4096 rows; never fewer than min_rows rows each), one per
 * listed device, and runs as the shard record protocol below (bowgpu_shard_begin -> records -> bowgpu_shard_finish, the carry-in stitch in
 * row order) on one persistent library thread per list entry.  The records are exchanged in host memory - one process holds them all: no
 * collective, no transport.  Each rank puts the windows it owns at their places in the caller's buffers, so the outputs, null counts and
 * bowgpu_agg_info are what the one-device call gives, bit for bit (info.kernel_ms: the slowest rank's; info.long_windows: the ranks' sum).
 *   Served: HOST columns (each rank stages its own rows once, over its own device's host link) and HOST_PINNED columns (each device reads
 * its range in place) with host-resident outputs, on any list of devices; DEVICE-resident columns or outputs only when every listed device is
 * the calling thread's device (the same id may be listed several times - which is also how a one-GPU box exercises the path).  Calls the
 * record protocol declines - aggregation.Mode, more than 16 aggregators, an interval column with nulls, strict_order with a window over
 * three ranks - and calls with too few rows take the one-device path of the calling thread as before; so does everything else in this
 * header.  Fanned-out calls are serialised process-wide (the devices are busy with one anyway).
 *   n <= 1 (or ids == NULL, n == 0) switches the fan-out off.  min_rows: default 2^20 (bowgpu_set_fanout_min_rows).  A process that never
 * calls bowgpu_set_devices starts with the list BOWGPU_DEVICES="0,1,..." names (and BOWGPU_FANOUT_MIN_ROWS), read once - for running an
 * unmodified program through the fan-out; nothing on the call path reads the environment. */
int bowgpu_set_devices(const int *ids, int n);
int bowgpu_get_devices(int *ids, int cap, int *n);   /* the list in force (n = 0: off); ids may be NULL */
int bowgpu_set_fanout_min_rows(int64_t rows);
/* row ranges (= library threads, = entries of the device list) that served the calling thread's last bowgpu_rolling_aggregate / _planned /
 * _interpolate_aggregate call; 1: the one-device path */
int bowgpu_last_call_ranks(int *ranks);
/* process-wide since load: Rolling.Aggregate calls that arrived while a list of two or more devices was in force, and how many of them ran as
 * row ranges (the rest: what the fan-out declines, served by the one-device path) */
int bowgpu_fanout_counts(int64_t *calls, int64_t *served);
/* Use an externally owned hipStream_t (e.g. torch's current stream) for all work of this
 * thread; NULL restores the library's own stream. */
int bowgpu_set_stream(void *hip_stream);
int bowgpu_synchronize(void);
/* Device state is per calling thread (stream, pools, a cache of freed scratch blocks: at most 24 blocks / 24 GB per thread);
 * a thread that exits releases its own.  bowgpu_trim frees cached scratch blocks now: the calling thread's (all_threads = 0)
 * or every thread's.  A failed allocation inside the library trims every thread's cache itself before reporting BOWGPU_ERR_OOM. */
int bowgpu_trim(int32_t all_threads, int64_t *bytes_freed /* nullable */);
/* free / total HBM of the calling thread's device (hipMemGetInfo): lets a host size its shards (288 GB per MI355X) */
int bowgpu_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* device time (HIP events on the stream) of the tile kernel of this thread's last aggregate call */
int bowgpu_last_kernel_ms(double *ms);
/* Rows of this thread's last Rolling.Aggregate / Rolling.Interpolate (_fill) call that were served by one of the two kernels the
 * library keeps for the shapes its fast kernels decline - rolling_agg_kernel (window ids beyond 32 bits inside one tile, tiles denser
 * than a head list, intervals >= 2^32 with time-weighted reducers: about 0.3 of the HBM peak where the wave-tile kernels reach
 * 0.6 - 0.7) and interp_tile_kernel (64-bit window ids, dropped rows, the -1 sentinel window, a trip whose lists overflow: half the
 * rate of interp_wave3_kernel).  0 for the usual call; the results are the same bits either way.  A caller that finds this non-zero on
 * its hot path is on a route 2 - 3x slower than the figures the documentation quotes. */
int bowgpu_last_call_slow_rows(int64_t *rows);
/* ... and which tile kernel that was ("rolling_wave_kernel", "rolling_agg_kernel", "long_stream_kernel", ...; "" before
 * any call; Rolling.Interpolate: "interp_wave3_kernel" or "interp_tile_kernel", the one whose outputs the call returned; the fills:
 * "fill_kernel").  rolling_simple_kernel, rolling_tw_kernel and rolling_twc_kernel come with their template arguments, spelled as
 * rocprofv3 prints them ("rolling_simple_kernel<0, false, false, false, false, false, false>", "rolling_twc_kernel<false, false, 128>"):
 * the text up to '<' is the kernel, the whole string the instantiation that ran - which says, among other things, which head list a
 * tile had (tests/tile_shapes.py instance_cap) - and what bench.py matches against the committed counter files (profiles/) and the per-kernel code hashes
 * the build leaves next to the library (libbowgpu.kernel_sha.json) */
const char *bowgpu_last_kernel_name(void);

/* ---- HBM buffers (so callers can keep columns resident between calls) ------------- */
int bowgpu_malloc(void **ptr, int64_t bytes);
int bowgpu_free(void *ptr);
int bowgpu_memcpy_h2d(void *dst, const void *src, int64_t bytes);
int bowgpu_memcpy_d2h(void *dst, const void *src, int64_t bytes);
int bowgpu_memset(void *dst, int value, int64_t bytes);

/* Page-lock `bytes` of host memory at `ptr` and map them for the device, so that columns inside the range may be passed with
 * residency BOWGPU_HOST_PINNED (reference bowseries.go:59-83 hands Go-heap slices: a cgo shim registers the Arrow buffers of a Bow
 * it keeps using - Bows are immutable - once, e.g. from a finalizer-paired constructor).  Registration costs about a millisecond
 * per 4 MB (every page is touched and locked): do it per buffer, not per call.  The range must stay valid until unregistered. */
int bowgpu_host_register(void *ptr, int64_t bytes);
int bowgpu_host_unregister(void *ptr);

/* ---- stream timers (HIP events on the stream the kernels are launched on) --------- */
int bowgpu_timer_create(void **timer);
int bowgpu_timer_start(void *timer);
int bowgpu_timer_stop(void *timer);
int bowgpu_timer_elapsed_ms(void *timer, double *ms); /* synchronises on the stop event */
int bowgpu_timer_destroy(void *timer);

/* ---- rolling.IntervalRolling ------------------------------------------------------- */

/* enforceIntervalAndOffset — reference rolling/rolling.go:114-128 */
int bowgpu_enforce_interval_and_offset(int64_t interval, int64_t offset, int64_t *offset_out);

/* newIntervalRolling + countWindows — reference rolling/rolling.go:69-112, :143-154.
 * `offset` is the raw Options.Offset.  Outputs the first window start and numWindows. */
int bowgpu_plan_windows(const bowgpu_col *ts, int64_t interval, int64_t offset, int64_t *s0,
                        int64_t *num_windows);

/* The same plan as one record, for hosts that keep it: the reference computes it ONCE, in the constructor
 * (newIntervalRolling, rolling/rolling.go:69-112, stores the first window start and numWindows in the intervalRolling), and
 * every later Aggregate / Interpolate on that Rolling uses it.  first_ts / last_ts are the two scalars the plan was made from.
 * With device-resident columns the plan costs one round trip to the GPU; bowgpu_rolling_aggregate_planned skips it. */
typedef struct bowgpu_plan {
    int64_t s0, num_windows;
    int64_t first_ts, last_ts;
    int64_t interval, offset;      /* offset: normalised (enforceIntervalAndOffset) */
    int64_t nrows;                 /* of the interval column the plan was made for */
} bowgpu_plan;
int bowgpu_plan_windows_ex(const bowgpu_col *ts, int64_t interval, int64_t offset, bowgpu_plan *plan);

/* Rolling.Aggregate — reference rolling/aggregation.go:123-238 (indexedAggregations,
 * validateAggregation, aggregateWindows) fused with the reducers of rolling/aggregation/.
 * One pass over the interval column buckets rows into windows; every aggregator of every
 * value column is reduced in that same pass (any number of aggregators and columns: beyond 16 outputs /
 * 8 column passes the call is cut into launches internally; aggregation.Mode runs as a pass of its own).
 *   cols[ncols]   the Bow's columns (only those referenced by ts_col / aggs are touched)
 *   outs[naggs]   one output column per aggregator, in aggregator order (A.7)
 * Device-path contract: interval column Int64, its valid values ascending (else BOWGPU_ERR_TS_UNSORTED: the caller keeps the
 * reference's own path); value columns Float64 or Int64.  Nulls in the interval column (rolling.go:190-193: such a row neither
 * ends nor extends a window, yet lies inside its window's slice when rows of the same window surround it) are served for
 * exclusive and inclusive iterations alike (incl. rolling.go:214-218's `rowIndex - 1` when a null follows an inclusive row);
 * with Mode the call is BOWGPU_ERR_TS_NULLS.  Cost of such a call: one extra pass over the interval column (16 bytes per row) that
 * writes a forward-filled copy of it (8 bytes per row) and n / 8 bytes per rewritten validity class (up to three per value column on
 * an inclusive iteration); every output goes through a device temporary (W * 8 bytes each) before it reaches the caller's buffer;
 * NumRows is counted as Count over the rows that belong to a window and converted to float64 in a pass of its own.
 *
 * BOOLEAN value columns (bowgpu_col.type == BOWGPU_BOOLEAN; the interval column stays Int64).  `values` is the Arrow bit-packed
 * buffer - bit offset + i, LSB first - addressed exactly as `validity` is: any byte alignment, any offset, read as aligned 32-bit
 * words (the 8-byte alignment rule is for 8-byte columns).  The three residencies are served; validity may be NULL, null_count -1.
 * Result types (rolling/aggregation.go:110-121): Sum / ArithmeticMean / Min / Max, the four time-weighted reducers and NumRows
 * Float64; Count Int64; First / Last / Mode BOOLEAN (bit-packed outputs: see bowgpu_out).  Values, bit for bit the reference's
 * with ToFloat64(true) = 1.0: for a window with nv valid rows of which nt are true - Sum float64(nt); ArithmeticMean
 * float64(nt) / float64(nv); Min 0.0 if a valid false exists, else 1.0; Max 1.0 if a valid true exists, else 0.0; Count nv;
 * First / Last the first / last valid row's bit; Mode the majority and, on a tie, the negation of the last valid value
 * (mode.go:18-27: the value whose count reaches the maximum first); all nil at nv == 0 but Sum (0.0) and Count (0).  The
 * windows are the ones Mode sees (an inclusive call does not change them: Window.UnsetInclusive).  These eight run as ONE pass per
 * Boolean column over the windows' bit ranges, after the other reducers of the call: integer arithmetic, exact at any window
 * length, no tolerance and no order question (long_windows is untouched by it; kernel_ms includes it).  Cost: the first-rows
 * pass Mode uses (8 bytes read per row, 8 written per window, once per call) + 8 bytes read per window + 8 bytes written per
 * window and Float64 / Int64 output (2 bits per window for a Boolean output); workspace 8 * (W + 1) bytes + the outputs'
 * bitmaps.  transformation.Factor applies to the Float64 / Int64 results as ever; on a BOOLEAN result it is the reference's
 * error "factor: invalid type bool": BOWGPU_ERR_UNSUPPORTED, before the device is touched.
 * The time-weighted reducers over a Boolean column are served by WIDENING: the column is expanded once per call into a
 * Float64 device temporary of 0.0 / 1.0 (8 bytes of workspace per row, + n / 8 for its validity) and takes the ordinary path as
 * that Float64 column - exactness, long_windows, strict_order and the stated tolerance are those of a Float64 column holding
 * the same values.
 * Declined with a Boolean column (the caller keeps the reference path): an interval column with nulls (BOWGPU_ERR_TS_NULLS, as
 * Mode); bowgpu_shard_* and bowgpu_rolling_aggregate_sharded (BOWGPU_ERR_UNSUPPORTED); under bowgpu_set_devices such a call is
 * not fanned out and is served by the caller's device, as a call with Mode is.  Interpolate, the fills,
 * bowgpu_rolling_interpolate_aggregate, bowgpu_aggregate_whole, the frame operations and the Parquet loader decline Boolean. */
int bowgpu_rolling_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col,
                             int64_t interval, const bowgpu_options *opts,
                             const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                             bowgpu_agg_info *info);

/* ... with the plan the host already holds (bowgpu_plan_windows_ex on THIS interval column; a plan whose nrows differs from the
 * column's length is rejected).  opts->offset is ignored in favour of the plan's. */
int bowgpu_rolling_aggregate_planned(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_plan *plan,
                                     const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs,
                                     bowgpu_out *outs, bowgpu_agg_info *info);

/* intervalRolling.Next for every window at once — reference rolling/rolling.go:177-239.
 * For window k: first_index[k] = Window.FirstIndex, [slice_begin[k], slice_end[k]) = the rows
 * of Window.Bow (0,0 when empty), is_inclusive[k] = Window.IsInclusive.  Arrays hold W
 * entries and may be NULL; residency applies to all of them. */
int bowgpu_window_bounds(const bowgpu_col *ts, int64_t interval, const bowgpu_options *opts,
                         int64_t *first_index, int64_t *slice_begin, int64_t *slice_end,
                         uint8_t *is_inclusive, int32_t residency);

/* aggregation.Aggregate (whole frame) — reference rolling/aggregation/whole.go:12-93.
 * outs[i].length is 1 (0 for an empty Bow).  At most 64 reducers per call (BOWGPU_ERR_UNSUPPORTED beyond); an Int64 interval
 * column without nulls, Int64 / Float64 value columns.
 * Bit-exact: type, length, validity and null_count of every output (SetOrDropStrict: WindowStart naming a Float64 column is nil,
 * a nil slot holds zero); WindowStart, NumRows, Count; Min / Max (float64(v); a NaN seed sticks, the earliest of equal extremes);
 * First / Last / Mode (the row's own 8 bytes: an Int64 beyond 2^53 is not carried through a double); a Factor chain on these.
 * Sum, ArithmeticMean, IntegralStep / IntegralTrapezoid and WeightedAverageStep / WeightedAverageLinear are summed ORDER-FREE -
 * per lane, wavefront, workgroup, then a fixed tree over the workgroups' records: equal inputs give equal bits, and they differ
 * from the reference's left-to-right loop by at most THE STATED TOLERANCE (bowgpu_agg_info.long_windows above) of ONE window of
 * n = all the frame's rows.  Where every term is an integer and SUM|T_i| < 2^53 (2^52 for the trapezoid terms, multiples of one
 * half) every partial sum is exact and the result is the reference's, bit for bit.  tests/whole_model.py,
 * tests/test_gpu_whole_fuzz.py assert all of this. */
int bowgpu_aggregate_whole(const bowgpu_col *cols, int32_t ncols, int32_t ts_col,
                           const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs);

/* ---- Rolling.Interpolate ----------------------------------------------------------- */
enum {
    BOWGPU_INTERP_WINDOW_START = 0,  /* interpolation/windowstart.go:8-14 */
    BOWGPU_INTERP_LINEAR = 1,        /* interpolation/linear.go:8-38 */
    BOWGPU_INTERP_STEP_PREVIOUS = 2, /* interpolation/stepprevious.go:8-26 */
    BOWGPU_INTERP_NONE = 3,          /* interpolation/none.go:7-13 */
    BOWGPU_INTERP_CONST = 4          /* constant-valued closure (interpolation_test.go:16-19) */
};

/* One rolling.ColInterpolation (rolling/interpolation.go:10-28) of a built-in kind plus what
 * it reads from Options.PrevRow (linear.go:14-18, stepprevious.go:13-15). */
typedef struct bowgpu_interp {
    int32_t kind;
    int32_t col;
    double const_value;
    int32_t has_prev_row;
    int32_t prev_t_valid;
    int32_t prev_v_valid;
    int32_t _pad;
    double prev_t;      /* prevRow.GetFloat64(intervalCol, last) */
    double prev_v;      /* prevRow.GetFloat64(col, last) */
    int64_t prev_v_i64; /* prevRow.GetValue(col, last) for Int64 columns (StepPrevious) */
} bowgpu_interp;

/* Rolling.Interpolate — reference rolling/interpolation.go:30-161.  Two calls: _count gives
 * the number of output rows (N + windows missing their start), _fill writes them.
 * interps must list the Bow's columns in order (bowappend.go:11-13 needs equal schemas).
 * CONTRACT between the two calls: a _fill that directly follows the _count of the same DEVICE-resident interval column (same
 * pointer, offset, length, interval, options, calling thread) reuses what the count pass learnt about it and does not scan it
 * again - the column must not be modified or freed in between (Bows are immutable in the reference; a cgo shim makes the two
 * calls back to back inside Rolling.Interpolate).  Writes and frees made THROUGH this library (bowgpu_free, bowgpu_memcpy_h2d,
 * bowgpu_memset, the generators) drop the reuse by themselves; a buffer rewritten by the caller's own kernels is the caller's to
 * keep unchanged.  As a last line the fill compares the number of rows it produces with the count: a mismatch is
 * BOWGPU_ERR_ARG and the outputs are to be discarded.
 * _fill does not NEED a preceding _count: called on its own it sizes the outputs itself against bowgpu_out.length (in: capacity;
 * rows + windows always suffice; too small is BOWGPU_ERR_ARG naming the size).  Inclusive windows then take one pass over the rows
 * (n_out = n + W - [row 0 on its window's start] needs no count); exclusive windows make their own count pass first.
 * DEVICE-resident outputs are written in place - no working copy of their bitmaps, no launch that zeroes or counts them - when each
 * validity pointer is 4-byte aligned and the capacity (bowgpu_out.length on entry) reaches the end of the 32-bit word that holds row
 * n_out - 1, i.e. ceil(length / 8) >= 4 * ceil(n_out / 32): allocate a multiple of 32 rows (Arrow's allocators pad to 64 bytes, 512
 * rows).  Outputs that do not qualify cost one more small launch and a copy of the bitmaps (0.03 ms per 1e8 rows), nothing else.
 * Input columns whose value pointers are not all 16-byte aligned (a slice at an odd row offset) take 8-byte loads in the kernel's
 * general instantiation.
 * An interval column WITH NULLS: the output is the windows' slices - rows that belong to no window vanish (rolling.go:190-193,
 * :224-228), null-timestamp rows inside a slice are copied as they are; inclusive windows too (incl. rolling.go:214-218's
 * `rowIndex - 1` after a null), except for two shapes that are BOWGPU_ERR_TS_NULLS (see the error code).  Any number
 * of columns (round 6: beyond 16 the value columns go in groups of 15, each with the interval column).  Cost: the call is made on the
 * KEPT rows, compacted into device temporaries (8 bytes per row and column + n / 8 bytes per bitmap); a _fill that follows its _count on
 * the same DEVICE-resident columns (the contract above) uses what the count built, any other _fill builds it itself.
 */
int bowgpu_rolling_interpolate_count(const bowgpu_col *cols, int32_t ncols, int32_t ts_col,
                                     int64_t interval, const bowgpu_options *opts,
                                     const bowgpu_interp *interps, int32_t ninterps,
                                     int64_t *n_out);
int bowgpu_rolling_interpolate_fill(const bowgpu_col *cols, int32_t ncols, int32_t ts_col,
                                    int64_t interval, const bowgpu_options *opts,
                                    const bowgpu_interp *interps, int32_t ninterps,
                                    bowgpu_out *outs);

/* Row-range sharded Rolling.Interpolate: a shard of the frame plus what lies beyond its two ends.
 * Synthetic rows sit in front of a window's first row, so the shard holding that row emits them - including the empty windows
 * since the last row on the shards to its left (has_left / left_last_ts).  A Linear / StepPrevious interpolator whose nearest
 * valid point lies on another shard gets it from the caller: the point to the LEFT through bowgpu_interp.prev_* (the reference's
 * own Options.PrevRow mechanism), the point to the RIGHT through next_*.  Shards concatenated in rank order = the unsharded
 * result, for exclusive and for inclusive windows (opts->inclusive: a row on its window's start is preceded by the copy of itself
 * that closes the window before - the copy travels with its row).  Negative timestamps: negative window starts are served (the
 * window that starts at -1, the reference's "no first value" sentinel, by the shard that accounts for it); rows below the first
 * window start (rolling.go:96-99) by the frame's first shard when the first row at or above s0 is its own - a first shard of nothing
 * but such rows is declined (BOWGPU_ERR_UNSUPPORTED). */
typedef struct bowgpu_interp_edge {
    int32_t has_left;         /* a shard to the left holds rows */
    int32_t _pad;
    int64_t left_last_ts;     /* the last of them */
    int32_t next_valid[8];    /* per column of the Bow: nearest valid point on the shards to the right (Linear) */
    double next_t[8], next_v[8];
} bowgpu_interp_edge;
/* a shard's own first / last valid point per column: what its neighbours fill their edges from (all_gather'ed as bytes) */
typedef struct bowgpu_interp_points {
    int64_t nrows, first_ts, last_ts;
    int32_t first_valid[8], last_valid[8];
    double first_t[8], first_v[8], last_t[8], last_v[8];
    int64_t last_v_i64[8];    /* raw payload of the last valid value of an Int64 column (StepPrevious keeps the integer) */
} bowgpu_interp_points;
int bowgpu_shard_interp_points(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, bowgpu_interp_points *out);
int bowgpu_shard_interpolate_count(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                                   const bowgpu_options *opts, int64_t global_s0, const bowgpu_interp *interps, int32_t ninterps,
                                   const bowgpu_interp_edge *edge, int64_t *n_out);
int bowgpu_shard_interpolate_fill(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                                  const bowgpu_options *opts, int64_t global_s0, const bowgpu_interp *interps, int32_t ninterps,
                                  const bowgpu_interp_edge *edge, bowgpu_out *outs);

/* ---- Rolling.Interpolate(...).Aggregate(...) without the interpolated frame ---------- */

/* r.Interpolate(interps...).Aggregate(aggs...) - reference rolling/interpolation.go:30-69 (returns a Rolling over the interpolated
 * Bow with the same interval and options) + rolling/aggregation.go:123-145 (consumes it) - when the caller wants only the aggregated
 * Bow: the interpolated frame (rows + one synthetic row per window that does not start on its first row, interpolation.go:98-161) is
 * never handed back and, where the shape allows it, never written.  interps: one per column of the Bow, in column order (as for
 * bowgpu_rolling_interpolate_*); aggs[i].col indexes those same columns - the interpolated Bow has the input's columns and types
 * (interpolation.go:139-155).  outs / info: as bowgpu_rolling_aggregate on the Rolling Interpolate returns.
 *   ONE pass over the rows (rolling_fused.hip: a window's synthetic value - linear.go:34-35's expression on the nearest both-valid
 * rows either side of the window's FirstIndex - is fed as the window's first row to the same left-to-right walk) for: exclusive
 * windows; WindowStart / Sum / ArithmeticMean / Min / Max / Count / First / Last / NumRows; an interval column without nulls under
 * interpolation.WindowStart; value columns under Linear / StepPrevious / None (/ WindowStart); a frame that starts at or above 0 and
 * spans less than 2^32 from its first window start; windows of 4 .. 128 rows on average, none longer than 128 rows.
 *   Everything else (and any call some tile of which the fused kernel cannot describe): bowgpu_rolling_interpolate_count + _fill into
 * device temporaries, then bowgpu_rolling_aggregate on them - what the two calls give, bit for bit, including their declines
 * (BOWGPU_ERR_TS_UNSORTED, ...).  Errors: newIntervalRolling's first, then Interpolate's (BOWGPU_ERR_TYPE "accepts types ...",
 * BOWGPU_ERR_KEEP_INTERVAL), then Aggregate's.  Both forms are bit-identical to the two calls made one after the other
 * (tests/test_gpu_fused.py: every window against oracle interpolate -> aggregate, and against the two-call path). */
int bowgpu_rolling_interpolate_aggregate(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                                         const bowgpu_options *opts, const bowgpu_interp *interps, int32_t ninterps,
                                         const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs, bowgpu_agg_info *info);

/* ---- Bow.FillLinear / IsColSorted -------------------------------------------------- */

/* Bow.FillLinear — reference bowfill.go:14-103.  out receives the filled copy of
 * cols[fill_col]; *unchanged = 1 where the reference returns the receiver itself
 * (bowfill.go:35-37, :53-55). */
int bowgpu_fill_linear(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col,
                       bowgpu_out *out, int32_t *unchanged);
/* The same for a caller whose own checks have run - reference bowfill.go:35-42: the ref column holds a value and IsColSorted says
 * yes (the cgo shim's hook sits behind them; its IsColSorted is bowgpu_is_col_sorted): the pass over the ref column that establishes
 * both (a quarter of the call at 1e8 rows) is not made a second time.  On a ref column that is NOT sorted the filled values are
 * whatever linear.go's expression gives between the neighbours found - no error, no out-of-bounds access. */
int bowgpu_fill_linear_sorted(const bowgpu_col *cols, int32_t ncols, int32_t ref_col, int32_t fill_col,
                              bowgpu_out *out, int32_t *unchanged);

/* Bow.FillPrevious / Bow.FillNext (LOCF / NOCB) — reference bowfill.go:162-253 — and Bow.FillMean — reference
 * bowfill.go:105-160 — of ONE Int64 / Float64 column (the reference loops over the selected columns, one goroutine each;
 * call once per column).  out receives the filled copy; *unchanged = 1 when the column has no nulls (the reference
 * passes such a column through, bowfill.go:130-133, :176-179).  Boolean / String columns: BOWGPU_ERR_UNSUPPORTED. */
#define BOWGPU_FILL_PREVIOUS 0
#define BOWGPU_FILL_NEXT 1
#define BOWGPU_FILL_MEAN 2
int bowgpu_fill(const bowgpu_col *col, int32_t method, bowgpu_out *out, int32_t *unchanged);

/* Bow.IsColSorted — reference bowassertion.go:15-81 (ascending OR descending, nulls skipped,
 * empty => false). */
int bowgpu_is_col_sorted(const bowgpu_col *col, int32_t *sorted);

/* ---- Bow.SortByCol ----------------------------------------------------------------- */

/* Bow.SortByCol - reference bowsort.go:10-41 - as three calls: the permutation (bowgpu_argsort), its application to one column
 * (bowgpu_take), and the whole frame in one call (bowgpu_sort_by_col).  ONE device, any residency, Int64 / Float64 columns:
 * BOWGPU_HOST inputs are staged through HBM as bowgpu_rolling_aggregate stages them, BOWGPU_HOST_PINNED inputs are read where they lie,
 * BOWGPU_DEVICE inputs are used where they lie; outputs may have any residency.  Per-thread contexts and streams as for every other
 * call (callable from several OS threads at once).  bowgpu_set_devices does not apply.  A sort ACROSS row-range shards on several
 * devices is a different algorithm (exact splitters, an exchange, a merge) and a call of its own: bowgpu_sort_by_col_sharded below.
 *   THE KEY COLUMN: Int64 or Float64, else BOWGPU_ERR_TYPE.  A key with nulls (null_count as given; counted when -1) is
 * BOWGPU_ERR_SORT_NULLS with the reference's message.  key_col out of range: BOWGPU_ERR_BAD_COL.  Columns of unequal length:
 * BOWGPU_ERR_ARG.  For host-resident columns these are decided before the device is touched (as bowgpu_plan_windows does), so they
 * are answered on a box without a GPU; a valid call of two or more rows without a GPU is BOWGPU_ERR_NO_DEVICE - no CPU fallback.
 *   THE ORDER: ascending by the reference's Buffer.Less (bowbuffer.go:126-139), STABLE: rows with equal keys keep their input order.
 * The reference uses sort.Sort, which promises nothing for equal keys; the stable order is one of the results it may give, the one
 * its own test table expects (bowsort_test.go:133-157), and the only one that makes the result a function of the input.  On keys
 * without duplicates the result is the reference's, bit for bit.  Float64: -0.0 and +0.0 are equal under Less and keep their input
 * order (each output value keeps its own bits: values are gathered from the input).  A Float64 key holding a NaN is
 * BOWGPU_ERR_UNSUPPORTED (Less is not an order there; the caller keeps the reference path).
 *   ALREADY SORTED means what sort.IsSorted means: no row i with key[i] < key[i-1] (ties included).  It is found in the one read of the
 * key that also builds the digit histograms; such a call costs that read and nothing else, and writes nothing.
 *   VALUE COLUMNS: Int64 / Float64 with or without validity, any Arrow offset (bit offsets that are no multiple of 8 included), moved
 * as raw 64-bit payloads - a NaN's payload and sign survive.  Other types: BOWGPU_ERR_UNSUPPORTED.  Outputs: value, validity bit and
 * null_count; null slots hold 0 and the padding bits of the last validity byte are clear (what Buffer.SetOrDropStrict leaves,
 * bowsort.go:33-36).
 *   SIZE: fewer than 2^31 rows (row indices inside the sort are 32 bits wide); more is BOWGPU_ERR_UNSUPPORTED naming the limit.
 * HBM WORKSPACE, taken from the calling thread's scratch cache like every other call's (exhaustion: BOWGPU_ERR_OOM): 24 bytes per row
 * (a 64-bit key image and a 32-bit row index, double-buffered) + 1 KB per 4096 rows of digit counts; + 8 bytes per row for the
 * widened permutation when bowgpu_argsort's perm is host-resident; + the staged copies of BOWGPU_HOST columns and the device
 * temporaries of host-resident outputs, at most 4 columns at a time.  A key that is already sorted takes none of it.
 *   THE METHOD (bow_amd/csrc/sort.hip): least-significant-digit radix sort over 8-bit digits of the key image (x ^ 2^63 for Int64; the
 * sign-flip map for Float64 with -0 folded onto +0); a digit that is the same in every key costs no pass (timestamps rarely use all
 * eight bytes).  The result does not depend on scheduling: the same call gives the same bytes. */

/* perm[j] = row of `key` that comes j-th in ascending order; key->length entries, residency as given.
 * *sorted = 1: the column is already in order (bowsort.go:19-21; 0 or 1 rows included) and perm is NOT written. */
int bowgpu_argsort(const bowgpu_col *key, int64_t *perm, int32_t perm_residency, int32_t *sorted);

/* out[j] = col[idx[j]] for j < n_idx: value, validity bit, null_count (out->length = n_idx; capacity on entry >= n_idx).  Indices may
 * repeat and n_idx may differ from col->length.  An index outside [0, col->length) is BOWGPU_ERR_ARG (nothing is read through it; the
 * output is then undefined). */
int bowgpu_take(const bowgpu_col *col, const int64_t *idx, int64_t n_idx, int32_t idx_residency, bowgpu_out *out);

/* Bow.SortByCol.  outs[ncols]: one output per column of the Bow, in column order, capacity >= rows.  *unchanged = 1 where the
 * reference returns the receiver itself (already sorted, or fewer than 2 rows): the outputs are then not written - neither their
 * buffers nor their length / null_count / type. */
int bowgpu_sort_by_col(const bowgpu_col *cols, int32_t ncols, int32_t key_col, bowgpu_out *outs, int32_t *unchanged);

/* Bow.SortByCol over a frame held as row-range shards on several devices - the remedy for BOWGPU_ERR_TS_UNSORTED of
 * bowgpu_rolling_aggregate_sharded, whose frame no single device holds.
 *   FRAME, RESIDENCY, ORDERING, SERIALISATION as for bowgpu_rolling_aggregate_sharded: cols_by_rank[r] holds ncols columns, rank r's
 * rows, on device_ids[r]; an id may repeat (how a one-GPU box runs the path); 1 <= world <= 64; ranks may be empty, all of them too;
 * any residency, a BOWGPU_DEVICE buffer of rank r must live on device_ids[r] (BOWGPU_ERR_ARG naming the rank); inputs must be complete
 * at the call (the calling thread's stream is synchronised first), outputs are complete on return; calls are serialised process-wide
 * (with bowgpu_rolling_aggregate_sharded's: one pool of library threads serves both); independent of bowgpu_set_devices.
 *   THE GUARANTEE.  outs_by_rank[r][i]: column i of output rank r, capacity (length on entry) >= rank r's row count.  Output rank r
 * gets exactly the row count of input rank r - the sorted frame keeps the caller's shard layout - and the outputs concatenated in rank
 * order are, bit for bit, what bowgpu_sort_by_col gives for the inputs concatenated in rank order: values, validity, null slots
 * holding 0, clear padding bits.  Ascending by Buffer.Less and STABLE: equal keys keep their (rank, row) order.  null_count of an
 * output counts that output's own rows.  Each rank holds fewer than 2^31 rows; the total is not bounded by that.
 *   *unchanged = 1 and nothing is written (buffers, length, null_count, type), as in the one-device call, when the whole frame is in
 * order: every rank is (sort.IsSorted, ties included) and no non-empty rank's first key is below the last key of the non-empty rank
 * before it; fewer than 2 rows in total are in order.
 *   ERRORS are those of bowgpu_sort_by_col for the concatenated frame: BOWGPU_ERR_SORT_NULLS with the reference's message and the
 * null count summed over the ranks; a Float64 key with a NaN on any rank BOWGPU_ERR_UNSUPPORTED; a key that is not Int64 / Float64
 * BOWGPU_ERR_TYPE; Boolean / String columns BOWGPU_ERR_UNSUPPORTED; key_col out of range BOWGPU_ERR_BAD_COL.  A rank whose columns
 * differ in length, or whose types differ from rank 0's: BOWGPU_ERR_ARG.  A capacity too small: BOWGPU_ERR_ARG naming rank and size,
 * nothing written.  world out of range or a NULL list: BOWGPU_ERR_ARG.  A rank of 2^31 rows or more: BOWGPU_ERR_UNSUPPORTED naming
 * the limit.  For host-resident columns all of these are decided before a device is touched; a valid call of two or more rows without
 * a GPU is BOWGPU_ERR_NO_DEVICE.  The first error is the call's; on an error the outputs are undefined.  An error on one rank never
 * leaves another waiting: every rank reaches every barrier of the call, whatever its status.
 *   THE METHOD (bow_amd/csrc/sort_shard_api.cpp, sort_shard.hip): each rank sorts its key (the radix argsort above); the
 * host bisects the 64-bit key image for the image of the row at every rank boundary of the global order - at most 65 rounds, each one
 * launch per rank and one small read back - and cuts ties there in rank order; a rank that was not in order gathers its columns into
 * sorted order; every destination pulls its pieces in source-rank order (hipMemcpyPeerAsync, or a device-to-device copy on one
 * device; no peer access is enabled, no device setting changed) and puts them together with bowgpu_append's kernel - straight into
 * its outputs when the pulled runs do not interleave, else into a staging frame whose runs a stable two-run merge (left run first on
 * equal keys, ceil(log2 runs) rounds) turns into one permutation for the gather.  The sorted images are NOT pulled with the pieces:
 * the destination forms them again from the staging frame's key column (one more kernel and one more read of that column there,
 * against 8 bytes per row not copied between devices; which of the two costs less has not been measured).  The same call gives the
 * same bytes.
 *   HBM WORKSPACE per rank, transient, from the rank thread's scratch cache (exhaustion: BOWGPU_ERR_OOM): the sort's 24 bytes per
 * row; one sorted copy of the shard (values + validity of every column) unless the rank was in order; the pulled pieces of at most 4
 * columns at a time; when a merge runs, the staging frame (values + validity of every column) and 24 bytes per row for the merge
 * (12 bytes - image and row - double-buffered); the staged copies of BOWGPU_HOST columns and the device temporaries of host-resident
 * outputs as in the one-device call. */
int bowgpu_sort_by_col_sharded(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world, int32_t ncols,
                               int32_t key_col, bowgpu_out *const *outs_by_rank, int32_t *unchanged);

/* What the calling thread's last bowgpu_sort_by_col_sharded did and where its time went (all 0 after a call that returned before
 * its ranks ran: an error found on the host, fewer than 2 rows).  A measurement aid: scratch/sort_sharded_wall.py. */
typedef struct bowgpu_sort_shard_info {
    int32_t splitter_rounds;   /* rounds of the splitter search (0: the frame was in order, or a rank failed before it) */
    int32_t merge_rounds;      /* most merge rounds on any destination rank (0: no rank had to merge) */
    int32_t sort_passes;       /* most radix passes in any rank's local sort (of 8) */
    int32_t merged_ranks;      /* destination ranks whose pulled runs interleaved */
    double local_sort_ms;      /* slowest rank: the kernels of its local sort, the read of the key included (device events) */
    double splitter_ms;        /* slowest rank: wall time of the splitter search, its launches, read backs and barriers */
    double merge_ms;           /* slowest rank: merge_init_kernel + the merge rounds (device events) */
} bowgpu_sort_shard_info;
int bowgpu_sort_by_col_sharded_info(bowgpu_sort_shard_info *info);

/* ---- Bow.Filter -------------------------------------------------------------------- */

/* Bow.Filter - reference bowsetters.go:58-132 - as three calls: the predicates evaluated into a row bitmap (bowgpu_filter_mask), the
 * rows of a bitmap moved together in row order (bowgpu_compact), and both in one call (bowgpu_filter).  The conventions are those of the
 * sort entry points: ONE device, any residency for inputs and outputs (BOWGPU_HOST staged through HBM, BOWGPU_HOST_PINNED and
 * BOWGPU_DEVICE read where they lie), per-thread contexts and streams; bowgpu_set_devices does not apply.  A filter ACROSS row-range
 * shards on several devices is not offered: filter each shard.
 *   PREDICATES.  One bowgpu_filter_pred is one MakeFilterValues(col, values...) (bowsetters.go:114-132) after the caller has run
 * Type.Convert on the values: the row is kept when its value equals one of `values`.  Equality is Go's == on the boxed value: Int64
 * exactly; Float64 by IEEE == (a NaN in the column or in the set matches nothing; -0.0 equals +0.0).  A null row matches only through
 * match_null (a value Convert turned into nil: GetValue gives nil, nil == nil).  n_values == 0 with match_null == 0 selects nothing.
 * Several predicates are ANDed (matchRowCmps), and so is the caller's bitmap and_mask (what a shim evaluates user closures
 * into), bit i of byte i / 8, LSB first, no offset, any alignment; NULL: none.
 *   NO SELECTOR: npreds == 0 without and_mask is the reference's "empty filter": every row is selected, which is
 * contiguous; bowgpu_filter then needs no device.
 *   COLUMNS: predicate and value columns are Int64 / Float64, with or without validity, at any Arrow offset (bit offsets that are no
 * multiple of 8 included).  Boolean / String anywhere: BOWGPU_ERR_UNSUPPORTED.  More than BOWGPU_FILTER_MAX_VALUES values or
 * BOWGPU_FILTER_MAX_PREDS predicates: BOWGPU_ERR_UNSUPPORTED naming the limit.  pred.col out of range: BOWGPU_ERR_BAD_COL.  Columns of
 * unequal length: BOWGPU_ERR_ARG.  Fewer than 2^31 rows; more is BOWGPU_ERR_UNSUPPORTED naming the limit.  For host-resident
 * arguments all of this is decided before the device is touched; a valid call that has rows to look at is BOWGPU_ERR_NO_DEVICE on a box
 * without a GPU - no CPU fallback.
 *   THE CONTIGUOUS CASE.  Where the reference returns a slice of the receiver or the empty slice (bowsetters.go:74-82) - the selected
 * rows are consecutive, or there are none - *contiguous = 1, *first / *count say which rows (*first = 0 when there are none), and the
 * outputs are NOT written: neither their buffers nor length / null_count / type.  It is known after the predicate pass, which is
 * then the whole cost of the call.
 *   OUTPUTS otherwise are what Buffer.SetOrDropStrict leaves and what bowgpu_take leaves: values moved as raw 64-bit payloads (a NaN's
 * bits survive), validity bit and null_count set, null slots 0, padding bits of the last validity byte clear, length = *count.
 * Nothing is written past slot *count - 1 or past validity byte ceil(*count / 8) - 1.  CAPACITY: bowgpu_out.length on entry; the
 * number of rows always suffices; too small is BOWGPU_ERR_ARG naming the size needed, and nothing is written.  A caller who wants
 * exact buffers calls bowgpu_filter_mask first (*selected) and then bowgpu_compact.
 *   HBM WORKSPACE, from the calling thread's scratch cache (exhaustion: BOWGPU_ERR_OOM): 1/8 byte per row (the bitmap) + 8 bytes
 * per 4096 rows (tile records, + 4 per 4096 of those for the scan of the counts); + the staged copy of a BOWGPU_HOST and_mask / mask, the staged
 * copies of BOWGPU_HOST columns and the device temporaries of host-resident outputs - the predicate columns for the whole call, the
 * others at most 4 columns at a time.
 *   THE METHOD (bow_amd/csrc/filter.hip): a predicate pass that reads only the predicate columns and stores one 64-bit word per 64
 * rows; an exclusive scan of the per-tile counts; a scatter pass in which lanes load only the rows they keep and a tile that keeps
 * nothing reads nothing but its 64 mask words.  No workgroup waits on another; the same call gives the same bytes. */
#define BOWGPU_FILTER_MAX_VALUES 32
#define BOWGPU_FILTER_MAX_PREDS  8
typedef struct bowgpu_filter_pred {
    int32_t col;
    int32_t n_values;
    int32_t match_null;   /* a value Convert turned into nil: the predicate then holds on null rows */
    int32_t _pad;
    const void *values;   /* HOST memory, n_values items of the column's type; may be NULL when n_values == 0 */
} bowgpu_filter_pred;

/* mask_out bit i (LSB first, no offset) = all preds hold on row i AND (and_mask == NULL or its bit i); ceil(rows / 8) bytes, the padding
 * bits of the last byte clear.  *selected = set bits; *first / *last = lowest / highest selected row (-1 / -1 when none).  cols may
 * hold the whole frame: only the predicate columns are read (with no predicate, cols[0] gives the number of rows). */
int bowgpu_filter_mask(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds,
                       const uint8_t *and_mask, int32_t and_mask_residency, uint8_t *mask_out, int32_t mask_residency,
                       int64_t *selected, int64_t *first, int64_t *last);

/* outs[c] = the rows of cols[c] whose mask bit is set, in row order (mask: ceil(rows / 8) bytes as bowgpu_filter_mask writes them; bits
 * past the last row are ignored).  The contiguous case: see above. */
int bowgpu_compact(const bowgpu_col *cols, int32_t ncols, const uint8_t *mask, int32_t mask_residency,
                   bowgpu_out *outs, int64_t *first, int64_t *count, int32_t *contiguous);

/* Bow.Filter in one call: the predicates, an optional caller mask ANDed in (NULL: none), the compaction.  The bitmap stays in the
 * workspace between the two passes (1/8 byte per row written and read, against 8 or more per row to evaluate the predicates twice). */
int bowgpu_filter(const bowgpu_col *cols, int32_t ncols, const bowgpu_filter_pred *preds, int32_t npreds,
                  const uint8_t *and_mask, int32_t and_mask_residency,
                  bowgpu_out *outs, int64_t *first, int64_t *count, int32_t *contiguous);

/* ---- Bow.DropNils / Bow.Diff / Bow.Distinct ------------------------------------------ */

/* The three steps the reference's users run between a Parquet read and a rolling call: Bow.DropNils (bow.go:188-224), Bow.Diff
 * (bowdiff.go:8-73) and Bow.Distinct (bowgetters.go:333-358).  The conventions are those of the sort and filter entry points: ONE device,
 * any residency for inputs and outputs (BOWGPU_HOST staged through HBM at most 4 columns at a time, BOWGPU_HOST_PINNED and BOWGPU_DEVICE
 * read where they lie), per-thread contexts and streams; bowgpu_set_devices does not apply.  Int64 / Float64 columns with or without
 * validity at any Arrow offset (bit offsets that are no multiple of 8 included); Boolean / String anywhere in the frame:
 * BOWGPU_ERR_UNSUPPORTED.  Columns of unequal length: BOWGPU_ERR_ARG.  Fewer than 2^31 rows; more is BOWGPU_ERR_UNSUPPORTED naming the
 * limit.  For host-resident arguments all of this is decided before the device is touched; a valid call that has rows to look at is
 * BOWGPU_ERR_NO_DEVICE on a box without a GPU - no CPU fallback.  Outputs are what Buffer.SetOrDropStrict leaves: null slots hold 0, the
 * padding bits of the last validity byte are clear, nothing is written past the slots produced.
 *   COLUMN SELECTION is selectCols (bowfill.go:268-288): col_idx[n_idx] names the columns, n_idx == 0 means every column, an index
 * outside the frame is BOWGPU_ERR_BAD_COL, a repeated index is the same as naming it once.
 *   A COLUMN HAS NO NULLS TO LOOK AT when its validity is NULL or its null_count is stated as 0; null_count == -1 means the bitmap is
 * read (it is not counted first).
 *   THE METHOD (bow_amd/csrc/frame_ops.hip): one small streaming kernel per operation in front of the layers of Bow.Filter and
 * Bow.SortByCol - a pass over validity bitmaps alone (1/8 byte per row and selected column, no value byte), a difference pass (8 bytes
 * read and written per row and column), a pass that flags the last row of each group of equal sorted keys.  No workgroup waits on
 * another; the same call gives the same bytes. */

/* mask_out bit i (LSB first, no offset) = every selected column is valid at row i AND (and_mask == NULL or its bit i).  The byte layout
 * and *selected / *first / *last are exactly those of bowgpu_filter_mask, so the result can be handed to bowgpu_compact or passed as the
 * and_mask of bowgpu_filter (a Filter and a DropNils then cost one compaction).  mask_out may be NULL: only the three numbers are wanted.
 * When no selected column has nulls to look at and there is no and_mask, every row is selected and a host-resident mask_out is filled
 * (all ones, padding clear) without the device.  HBM WORKSPACE: that of bowgpu_filter_mask (1/8 byte per row + 8 bytes per 4096 rows)
 * + the staged bitmaps (never the values) of BOWGPU_HOST columns, 1/8 byte per row each, + the staged copy of a BOWGPU_HOST and_mask. */
int bowgpu_valid_mask(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx,
                      const uint8_t *and_mask, int32_t and_mask_residency, uint8_t *mask_out, int32_t mask_residency,
                      int64_t *selected, int64_t *first, int64_t *last);

/* Bow.DropNils in one call: the mask above, kept in the workspace, then the scan and the scatter of bowgpu_filter.  outs[ncols]: one
 * output per column of the frame; the contract is bowgpu_filter's, capacity rule included (bowgpu_out.length on entry; the number of
 * rows always suffices; too small is BOWGPU_ERR_ARG naming the size needed, and nothing is written).  THE CONTIGUOUS CASE: nothing is
 * dropped, or the kept rows are consecutive, or there are none: *contiguous = 1 with *first / *count (*first = 0 when there are none),
 * and the outputs are NOT written.  The reference returns the receiver itself only when nothing is dropped (bow.go:210-212) and
 * materialises a new frame otherwise; the values of that frame are those of the slice [*first, *first + *count) of the inputs.  When no
 * selected column has nulls to look at the answer is contiguous, *first = 0, *count = rows, without the device.  HBM WORKSPACE: that of
 * bowgpu_valid_mask + that of bowgpu_filter's scatter (4 bytes per 4096 * 4096 rows for the scan; the staged copies of BOWGPU_HOST columns
 * and the device temporaries of host-resident outputs, at most 4 columns at a time). */
int bowgpu_drop_nils(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx,
                     bowgpu_out *outs, int64_t *first, int64_t *count, int32_t *contiguous);

/* Bow.Diff.  outs: one output per SELECTED column, in ascending column order (unselected columns pass through the reference untouched
 * and are not the library's business); capacity >= rows.  out[i] = col[i] - col[i-1], valid when both rows are valid; row 0 is always
 * null.  Int64 differences wrap as Go's do; Float64 is one IEEE subtraction (nothing contracted or reassociated); the sign and
 * payload of a NaN the subtraction GENERATES (inf - inf) are the device's.  length = rows, null_count is set.  Zero rows: length 0,
 * nothing written, no device.  An output that overlaps an input is not supported.  HBM WORKSPACE: none beyond the staged copies of
 * BOWGPU_HOST columns, the device temporaries of host-resident outputs and the validity working copies (1/8 byte per row), at most 4
 * columns at a time. */
int bowgpu_diff(const bowgpu_col *cols, int32_t ncols, const int32_t *col_idx, int32_t n_idx, bowgpu_out *outs);

/* Bow.Distinct: the non-null values of one column, each once, ascending by Buffer.Less (bowbuffer.go:126-139).  The output has no nulls:
 * length = *n_distinct, null_count = 0, validity all set, padding clear.  CAPACITY: bowgpu_out.length on entry; the column's count of
 * valid rows always suffices; too small is BOWGPU_ERR_ARG naming the size needed, and nothing is written (the count is known before the
 * compaction).  A Float64 column holding a NaN among its valid rows is BOWGPU_ERR_UNSUPPORTED, as for the sort: the reference's map makes
 * every NaN a key of its own, and Less is no order there.  -0.0 and +0.0 are ONE value (Go's == on the map key); the survivor is the LAST
 * zero in row order, because Go's map assignment rewrites the stored key when an equal float or interface key is assigned again.  That
 * rests on a reading of the Go runtime (map assignment with needkeyupdate), not on a run of the reference; it is the contract here.
 * All null, or zero rows: *n_distinct = 0 and nothing is written - neither the buffers nor length / null_count / type.
 *   HBM WORKSPACE: a column with nulls is first compacted by its own validity (8 bytes per valid row + bowgpu_valid_mask's); a column
 * that is not already in order takes bowgpu_argsort's 24 bytes per row and 8 bytes per row for the keys gathered through the
 * permutation; then bowgpu_filter_mask's workspace for the flags.  A column in order (sort.IsSorted) and without nulls takes only that
 * last part: it is read twice and nothing is sorted. */
int bowgpu_distinct(const bowgpu_col *col, bowgpu_out *out, int64_t *n_distinct);

/* ---- Bow.Convert ---------------------------------------------------------------------- */

/* Bow.Convert (bowsetters.go:52-56; Type.Convert, bowtypes.go:64-81; bowconvert.go) for ncols columns in one call:
 * outs[i] = cols[i] converted to to_types[i].  Source and target type are each BOWGPU_INT64, BOWGPU_FLOAT64 or BOWGPU_BOOLEAN - all nine
 * pairs, a different pair per column if wanted; this is the entry point that takes a Boolean column from, and brings one to, the
 * entry points that decline it.  The conventions are those of the other frame entry points: ONE device, any residency per column and
 * per output (BOWGPU_HOST staged through HBM at most 4 columns at a time, BOWGPU_HOST_PINNED and BOWGPU_DEVICE read where they lie),
 * per-thread contexts and streams; bowgpu_set_devices does not apply.  Any Arrow offset, bit offsets that are no multiple of 8
 * included, for the validity and for a Boolean column's value bits; validity NULL, or null_count 0 (the bitmap is not read) or -1.  The
 * columns need not have equal lengths (Convert has no frame rule); each outs[i].length on entry is a capacity >= cols[i].length.
 * outs[i] must not overlap cols[i]: an output that overlaps an input is not supported.
 *   THE RESULT is what Apply builds - NewBuffer, then SetOrDropStrict(i, t.Convert(GetValue(i))) per row.  A null row stays null and
 * its slot holds 0 (a clear bit), whatever the input's slot held; a valid row stays valid (among these three types Convert cannot
 * fail): the output's validity is the input's re-based to bit 0, null_count the input's count of nulls (counted in the same pass),
 * type the target, length the column's.  A BOOLEAN output follows bowgpu_out's rule: ceil(n / 8) bytes of values, padding bits clear
 * in both buffers, no byte past ceil(n / 8) written.  Per valid row:
 *     Int64   -> Float64  Go's float64(v): round to nearest, ties to even          Int64 -> Boolean    v != 0
 *     Float64 -> Int64    Go's int64(v) AS gc/amd64 GIVES IT: truncation toward zero where -2^63 <= v < 2^63; for NaN, +-Inf and
 *                         everything outside that range 0x8000000000000000 (INT64_MIN).  Go leaves the out-of-range result
 *                         implementation-defined; the project follows gc on amd64, as it does for -ffp-contract.
 *     Float64 -> Boolean  v != 0.0: a NaN is true, -0.0 is false                    Boolean -> Int64    1 / 0
 *     Boolean -> Float64  1.0 / 0.0                                                 same type           the same bits (a NaN keeps its payload)
 *   ERRORS, all before any device is touched: a source or target of BOWGPU_STRING is BOWGPU_ERR_UNSUPPORTED (the reference's own loop
 * serves those); any other type code, a null argument with ncols > 0, a negative length or offset, an unknown residency or a
 * capacity below the column's length is BOWGPU_ERR_ARG.  ncols == 0 returns 0; columns without rows give empty outputs of the target
 * types without a device; a well-formed call with rows is BOWGPU_ERR_NO_DEVICE on a box without a GPU - no CPU fallback.
 *   THE METHOD (bow_amd/csrc/convert.hip): one streaming pass, up to 4 columns a launch; 16-byte loads and stores of the 8-byte values,
 * bits read and written as whole words, the valid rows counted on the way.  No workgroup waits on another; the same call gives the
 * same bytes.  HBM WORKSPACE: none beyond the staged copies of BOWGPU_HOST columns, the device temporaries of host-resident outputs
 * and the working copies of the output bitmaps (1/8 byte per row; a Boolean output's values likewise), at most 4 columns at a time. */
int bowgpu_convert(const bowgpu_col *cols, const int32_t *to_types, int32_t ncols, bowgpu_out *outs);

/* ---- AppendBows / Bow.Find / FindNext / Contains -------------------------------------- */

/* Putting a frame together from pieces and finding a row by value: AppendBows (bowappend.go:11-103) and Bow.Find / FindNext / Contains
 * (bowfind.go:3-32).  The conventions are those of the sort, filter and frame-ops entry points: ONE device, any residency per piece and
 * per output (BOWGPU_HOST staged through HBM at most 4 columns at a time, BOWGPU_HOST_PINNED and BOWGPU_DEVICE read where they lie),
 * per-thread contexts and streams; bowgpu_set_devices does not apply.  Int64 / Float64 columns with or without validity at any Arrow
 * offset (bit offsets that are no multiple of 8 included); Boolean / String anywhere: BOWGPU_ERR_UNSUPPORTED.  Fewer than 2^31 rows (in
 * total, for the append); more is BOWGPU_ERR_UNSUPPORTED naming the limit.  For host-resident arguments all of this is decided before the
 * device is touched; a valid call that has rows to move or to look at is BOWGPU_ERR_NO_DEVICE on a box without a GPU - no CPU fallback.
 *   A COLUMN HAS NO NULLS TO LOOK AT when its validity is NULL or its null_count is stated as 0 (the rule of the block above).
 *   THE METHOD (bow_amd/csrc/append.hip): the append divides the OUTPUT rows over workgroups; a row finds its piece by a search in the
 * prefix array of the pieces' start rows (once per row for up to 4 columns; wave-uniform, and then free, when the 1024 rows of a wave
 * lie in one piece), and a wave stores the 64-bit validity word of its 64 rows whole - however many pieces meet inside it.  The search
 * lowers one device word to the lowest matching row by an integer atomic min, and a wave whose rows lie above that word leaves without
 * loading.  Every output byte has one writer; the same call gives the same bytes and the same row. */

/* AppendBows.  frames[f] points at the ncols columns of piece f; outs[ncols] receives the concatenation in piece order.  Every piece
 * must have ncols columns of equal length within the piece (unequal: BOWGPU_ERR_ARG); a column's type must be the same in every piece,
 * else BOWGPU_ERR_TYPE with the reference's text, "incompatible types 'int64' and 'float64'" (bowappend.go:40-42), and nothing is
 * written.  nframes < 1: BOWGPU_ERR_ARG.  More than 2^18 = 262144 pieces: BOWGPU_ERR_UNSUPPORTED naming the limit.
 *   nframes == 1 is where the reference returns its argument (bowappend.go:19-21): *unchanged = 1 and the outputs are NOT written -
 * neither the buffers nor length / null_count / type.  Zero rows in total: length = 0, null_count = 0, type set, nothing else written,
 * no device.  Pieces of zero rows are legal anywhere and contribute nothing (bowappend_test.go:29-55).
 *   Otherwise outs[c].length is the total and type is set.  Values move as raw 64-bit payloads (a NaN's bits survive).  The validity bit
 * of every row is set from the source, a source without a bitmap being all valid; NULL SLOTS HOLD 0 whatever the source held there; the
 * padding bits of the last validity byte are clear; nothing is written past slot total - 1 or validity byte ceil(total / 8) - 1.
 * null_count is set: when every piece of a column states its null_count (or has no nulls to look at, or is host-resident) the sum is the
 * answer and nothing is counted on the device; otherwise the finished bitmap is counted.
 *   CAPACITY: bowgpu_out.length on entry; too small is BOWGPU_ERR_ARG naming the size needed, and nothing is written.  An output that
 * overlaps an input is not supported.
 *   HBM WORKSPACE: the piece table (4 bytes a piece + 24 bytes a piece and column, at most 4 columns at a time), the staged copies of
 * BOWGPU_HOST pieces, the device temporaries of host-resident outputs and the validity working copies (1/8 byte per row), at most 4
 * columns at a time. */
int bowgpu_append(const bowgpu_col *const *frames, int32_t nframes, int32_t ncols, bowgpu_out *outs, int32_t *unchanged);

/* Bow.FindNext.  value is HOST memory: one item of the column's type (8 bytes), after the caller's type check - a value boxed as another
 * type than the column's finds nothing and needs no call (bowfind_test.go:31-32).  *row is the first row >= row_start that is valid and
 * whose value equals *value by Go's == on the boxed value: Int64 exactly; Float64 by IEEE == (a NaN in the column or as the value matches
 * nothing, -0.0 equals +0.0); -1 when there is none.  row_start < 0: BOWGPU_ERR_ARG; row_start >= length: -1.
 *   value == NULL is Go's nil: *row is the first NULL row of the column COUNTED FROM ROW 0 - row_start is ignored.  That is the
 * reference's behaviour (bowfind.go:12-19 loops from 0 whatever rowIndex is), kept as it is.  The search reads bitmaps only.
 *   Bow.Find is row_start = 0; Bow.Contains is *row != -1.
 *   No device is needed for zero rows, a row_start past the end, a NaN value, and nil on a column with no nulls to look at.
 *   HBM WORKSPACE: none beyond the staged copy of a BOWGPU_HOST column (for nil: of its bitmap alone). */
int bowgpu_find_next(const bowgpu_col *col, int64_t row_start, const void *value, int64_t *row);

/* ---- Bow.Equal, the Prev / Next valid-row getters, IsColEmpty --------------------------- */

/* Asking whether two frames are the same, and where the nearest valid row is, where the data lies: the per-row half of Bow.Equal
 * (bow.go:227-275), the search of GetPrevRowIndex / GetNextRowIndex / GetPrevValue(s) / GetNextValue(s) (bowgetters.go:65-151) and
 * IsColEmpty (bowassertion.go:84-86).  The conventions are those of the append / find block above: ONE device, any residency per column
 * (BOWGPU_HOST staged through HBM - for bowgpu_equal at most 4 column pairs at a time -, BOWGPU_HOST_PINNED and BOWGPU_DEVICE read where
 * they lie), any Arrow offset (bit offsets that are no multiple of 8 included), per-thread contexts and streams; bowgpu_set_devices does
 * not apply.  A COLUMN HAS NO NULLS TO LOOK AT when its validity is NULL or its null_count is stated as 0.  Fewer than 2^31 rows; more is
 * BOWGPU_ERR_UNSUPPORTED naming the limit.  For host-resident arguments every decision that needs no data is made before the device is
 * touched; a well-formed call that has rows to look at is BOWGPU_ERR_NO_DEVICE on a box without a GPU - no CPU fallback.
 *   THE METHOD (bow_amd/csrc/equal.hip): a wave compares 64 rows of a column pair at a time - both sides' validity words (and a Boolean
 * column's value words) funnel-shifted onto row alignment, each with its own bit offset, the values by plain coalesced loads - into one
 * 64-bit "differs" word, and the lowest set bit lowers ONE device word by an unsigned 64-bit atomic min of (row << 32) | column; a wave
 * whose rows lie above that word leaves without loading.  The valid-row search ANDs the 64-row words of its columns and lowers (raises)
 * one word the same way, starting at the tile of row_start and moving away from it.  Nothing is written but those words; the same call
 * gives the same answer. */

/* how valid rows compare in bowgpu_equal */
enum {
    BOWGPU_EQUAL_GO = 0,     /* the reference's rule, reflect.DeepEqual on the boxed values of GetRow (bow.go:269): Int64 exactly; Float64 by
                                IEEE == (-0.0 equals +0.0, a NaN differs from everything, ITSELF INCLUDED: a frame with a valid NaN is not
                                equal to itself, also when both sides are the same pointers); Boolean by the bit */
    BOWGPU_EQUAL_BITS = 1    /* "bit for bit": valid rows compare by their 64-bit pattern (a NaN equals a NaN of the same payload, -0.0
                                differs from +0.0); Boolean by the bit */
};
typedef struct {
    int32_t equal;           /* 1: no row differs (first_col = -1, first_row = -1) */
    int32_t first_col;       /* the lowest column that differs at first_row; for a type mismatch: the lowest column whose types differ */
    int64_t first_row;       /* the lowest row at which any column differs; -1 for a type or a length mismatch */
} bowgpu_equal_info;

/* The per-row half of Bow.Equal: column i of `left` against column i of `right`, ncols columns each.  Names and metadata are the
 * caller's to compare; the ABI has neither.  Column types: Int64, Float64, Boolean (`values` is the Arrow bit-packed buffer, read at bit
 * offset + i).  Row r of column c DIFFERS when exactly one side is valid there, or when both are valid and the values differ under
 * `mode`.  A null row's slot is never compared: garbage under a null differs from nothing.  Bits of a bitmap or of a Boolean buffer
 * outside [offset, offset + length) do not count.  A column with a bitmap of all ones equals one without a bitmap.
 *   ANSWERED WITHOUT A DEVICE: ncols == 0: equal.  Column c of different types on the two sides (the reference's Schema().Equal):
 * equal = 0, first_col = the lowest such c, first_row = -1.  Frames of different lengths: equal = 0, first_col = -1, first_row = -1.
 * Zero rows on both sides, types matching: equal.
 *   ERRORS: columns of unequal length within one frame, an unknown mode, ncols < 0, a NULL info: BOWGPU_ERR_ARG.  A String column (or any
 * other type than the three) on either side: BOWGPU_ERR_UNSUPPORTED.  2^31 rows or more: BOWGPU_ERR_UNSUPPORTED.
 *   No output.  HBM WORKSPACE: none beyond the staged copies of BOWGPU_HOST columns (at most 4 column pairs at a time) and one word. */
int bowgpu_equal(const bowgpu_col *left, const bowgpu_col *right, int32_t ncols, int32_t mode, bowgpu_equal_info *info);

/* The nearest row at which EVERY one of the ncols columns is valid: for direction == -1 the largest r <= row_start, for direction == +1
 * the smallest r >= row_start; *row = -1 when there is none.  Only bitmaps are read, so every column type is accepted, Boolean and String
 * included; the caller fetches the value(s) at the returned row itself (device-resident: one bowgpu_memcpy_d2h).
 *   ncols = 1 is GetPrevRowIndex / GetNextRowIndex (bowgetters.go:127-151), the row half of GetPrevValue / GetNextValue (:67-91).
 *   ncols = 2 is GetPrevValues / GetNextValues (:95-123).  Why: GetPrevValues' loop holds a row index i (<= the start).  Each turn moves
 * i down to p1 = the largest row <= i where column 1 is valid, then finds p2 = the largest row <= p1 where column 2 is valid; p2 == p1
 * ends it, otherwise i = p1 - 1.  No row in (p1, i] is valid in column 1, and p1 itself is rejected only when column 2 is null there, so
 * the loop never steps over a row where both are valid and ends on the first such row it meets going down: the largest row <= the start
 * where both are valid - or -1 when column 1 runs out (p1 = -1 makes p2 = -1: "equal") or i falls below row 0.  GetNextValues mirrors it.
 *   row_start outside [0, length) gives -1 without a device: the guard of the reference's loops; a negative start is no error here.
 * Columns with no nulls to look at drop out; if none is left the answer is row_start, without a device.
 *   ERRORS: ncols < 1, ncols > BOWGPU_VALID_ROW_MAX_COLS (the message names the limit), a direction other than +1 / -1, columns of unequal
 * length: BOWGPU_ERR_ARG.  2^31 rows or more: BOWGPU_ERR_UNSUPPORTED.
 *   HBM WORKSPACE: the staged bitmaps of BOWGPU_HOST columns (all of the call's at once: 1/8 byte per row and column) and one word. */
#define BOWGPU_VALID_ROW_MAX_COLS 8
int bowgpu_valid_row(const bowgpu_col *cols, int32_t ncols, int64_t row_start, int32_t direction, int64_t *row);

/* IsColEmpty: *empty = (NullN() == Len()); zero rows is empty (0 == 0).  A stated null_count (or no bitmap) answers without a device;
 * null_count = -1 with a bitmap: the bitmap is counted on the device.  Any column type. */
int bowgpu_is_col_empty(const bowgpu_col *col, int32_t *empty);

/* ---- Bow.InnerJoin / Bow.OuterJoin ----------------------------------------------------- */

/* Two frames that share one column put into one frame: Bow.InnerJoin (bowjoin.go:12-62, the fill :188-277) and Bow.OuterJoin
 * (bowjoin.go:66-125, the fills :279-574) on ONE key column per side - the reference's single common column.  The conventions are those of
 * the sort, filter, frame-ops and append entry points: ONE device, any residency per column and per output (BOWGPU_HOST staged through HBM
 * at most 4 columns at a time, BOWGPU_HOST_PINNED and BOWGPU_DEVICE read where they lie), per-thread contexts and streams;
 * bowgpu_set_devices does not apply.  Int64 / Float64 columns with or without validity at any Arrow offset (bit offsets that are no
 * multiple of 8 included); Boolean / String anywhere: BOWGPU_ERR_UNSUPPORTED.  Columns of unequal length within a frame: BOWGPU_ERR_ARG.  A
 * key index outside its frame: BOWGPU_ERR_BAD_COL.  Left rows, right rows and output rows are each fewer than 2^31; more is
 * BOWGPU_ERR_UNSUPPORTED naming the limit (for the output rows: known after the probe, before anything is written).  For host-resident
 * arguments every check above is made before the device is touched.
 *   THE PAIR LIST is getCommonRows (bowjoin.go:161-186): every pair (l, r) of a left and a right row whose keys are equal, ordered by l,
 * then by r.  KEY EQUALITY is Go's == on the boxed GetValue: Int64 exactly; Float64 by IEEE == (-0.0 equals +0.0); a null key equals a
 * null key (nil == nil: bowjoin_test.go:418-463 and :626-668, "with only nils in common rows") and never a value.  A Float64 key with a NaN
 * among its valid rows, on either side, is BOWGPU_ERR_UNSUPPORTED as for the sort and bowgpu_distinct: the reference matches it with
 * nothing, and the caller keeps the reference path.  Key types that differ: BOWGPU_ERR_TYPE, "left and right bow on join columns are of
 * incompatible types" (the reference's text up to the column name: the library knows no names).
 *   BOWGPU_JOIN_INNER: one output row per pair, in pair order.  BOWGPU_JOIN_OUTER: every left row in left order - a left row with m >= 1
 * matches becomes m rows, one per matching right row in ascending right row, a left row without a match one row whose right columns are
 * null - then every right row that occurs in no pair, in right row order, its left columns null.  Row count = L + (pairs - distinct l in
 * pairs) + (R - distinct r in pairs) (bowjoin.go:98-99).
 *   COLUMNS of the result: every left column in order, then every right column except the key, in order.  The key column holds the left
 * row's value; on a right-only row it takes the RIGHT key's value and validity (bowjoin.go:397: a right-only row with a null key keeps a
 * null key).  NO COMMON COLUMN (left_key == right_key == -1; bowjoin_test.go:363-396 and :581-604): the pair list is empty, InnerJoin has
 * zero rows, OuterJoin is all left rows then all right rows, and the result has all left columns then ALL right columns.  MORE THAN ONE
 * COMMON COLUMN is not expressible here - one key per side: it is bowgpu_join_keys_rows / bowgpu_join_keys below.
 *   OUTPUTS are what Buffer.SetOrDropStrict leaves and what bowgpu_take leaves: values moved as raw 64-bit payloads (a NaN's bits in a
 * VALUE column survive), validity bit and null_count set, length / type set, null slots 0, the padding bits of the last validity byte
 * clear, nothing written past the slots produced.  CAPACITY is Filter's rule: bowgpu_out.length on entry; too small is BOWGPU_ERR_ARG
 * naming the size needed, and nothing is written.  No input size bounds a join's row count: bowgpu_join_rows with NULL index buffers is the
 * count that sizes the outputs.
 *   NO DEVICE IS NEEDED when both frames have zero rows, when an InnerJoin has an empty side or no common column (zero rows), and for the
 * COUNT of an OuterJoin with an empty side or no common column (L + R rows, no pair).  The ROWS of such an OuterJoin - the other side's
 * rows padded with nulls - are the gather's work and need the device.  Every other valid call has rows to look at and is
 * BOWGPU_ERR_NO_DEVICE on a box without a GPU - no CPU fallback.  The same call gives the same bytes.
 *   HBM WORKSPACE, from the calling thread's scratch cache (exhaustion: BOWGPU_ERR_OOM).  Per RIGHT row: bowgpu_argsort's 24 bytes (none
 * when the right key is already in order), 8 for the sorted key images, 4 for the index, 1 for the group-head flags, 1/4 for the two row
 * bitmaps (+ 8 bytes per 4096 rows of tile records each); a right key with nulls adds 12 per valid row (its row numbers and values, in
 * row order); an OuterJoin adds 4 per right-only row.  Per LEFT row: 12 bytes ((first, count) and the scanned start).  Per OUTPUT row: 8
 * bytes (the pair, two 32-bit rows), + 16 when bowgpu_join_rows hands host-resident index buffers out.  + the staged copies of BOWGPU_HOST
 * columns and the device temporaries of host-resident outputs: the two keys for the whole call, the others at most 4 columns at a time.
 *   THE METHOD (bow_amd/csrc/join.hip): the output keeps the LEFT frame's order, so only the right key is sorted - its null rows are set
 * aside in row order by bowgpu_valid_mask's pass, its values go through the stable radix argsort (a right key already in order, the
 * time-series case, costs the one read that finds it so).  One lane per left row then finds the lower and upper bound of its key's image
 * in the sorted images; the per-row counts are scanned; the right-only rows are the right rows whose group of equals no left row hit,
 * flagged per right ROW and brought into row order by the mask pass; an expand pass over OUTPUT rows writes the (left row, right row)
 * pairs and a gather with a "no row" index moves the columns. */
#define BOWGPU_JOIN_INNER 0
#define BOWGPU_JOIN_OUTER 1

/* The rows of the join without moving a column.  *rows: output rows; *pairs: the length of the reference's commonRows.  Row j of the
 * result comes from left row l_idx[j] and right row r_idx[j], -1 for "no row"; idx_capacity slots each (too few: BOWGPU_ERR_ARG naming
 * the size, nothing written), residency as given.  l_idx == r_idx == NULL: the call is the count that sizes the outputs and writes
 * nothing.  left_key == right_key == NULL stands for "no common column": the pair list is empty, and since the call cannot know the
 * frames' lengths *rows is 0 for both kinds - the no-common-column join, whose OuterJoin has L + R rows, is bowgpu_join with -1 / -1.  ONE
 * NULL key is BOWGPU_ERR_ARG: the rows of the side that is given alone would be a partial answer. */
int bowgpu_join_rows(const bowgpu_col *left_key, const bowgpu_col *right_key, int32_t kind, int64_t *l_idx, int64_t *r_idx,
                     int64_t idx_capacity, int32_t idx_residency, int64_t *rows, int64_t *pairs);

/* The whole join in one call: outs[n_left + n_right - 1] (n_left + n_right without a common column), *rows output rows.  The index pairs
 * stay in the workspace as 32-bit rows. */
int bowgpu_join(const bowgpu_col *left_cols, int32_t n_left, int32_t left_key, const bowgpu_col *right_cols, int32_t n_right,
                int32_t right_key, int32_t kind, bowgpu_out *outs, int64_t *rows);

/* The join on SEVERAL common columns, as the reference joins on EVERY column name two bows share (getCommonCols bowjoin.go:128-155;
 * getCommonRows :161-186 calls a row pair common when it agrees on all of them).  Key pair k joins left_keys[k] with right_keys[k]:
 * column indices into the two frames for bowgpu_join_keys, the columns themselves for bowgpu_join_keys_rows.  Everything above holds
 * with "the key" read as "the tuple of keys":
 *   THE PAIR LIST is every (l, r) for which EVERY key pair is equal, ordered by l, then by r.  Equality per column is the one-key join's:
 * Int64 exactly, Float64 by IEEE == (-0.0 equals +0.0), a null equals a null and never a value, per column - rows that are nil in every
 * common column on both sides pair up ("outer advanced", bowjoin_test.go:247-298).  A Float64 key with a NaN among its valid rows, on
 * either side, is BOWGPU_ERR_UNSUPPORTED; the message names the side and the key pair.  A NaN payload under a null is not a key.
 *   ROW ORDER AND COUNT are bowgpu_join's.  INNER: one output row per pair, in pair order.  OUTER: every left row in left order - a left
 * row with m matches becomes m rows in ascending right row - then the right rows that occur in no pair, in right row order.
 *   COLUMNS of the result: every left column in order, then every right column that is NOT one of the right keys, in order:
 * n_left + n_right - n_keys outputs.  EACH key column holds the left row's value; on a right-only row it takes the value and validity of
 * ITS OWN right key column (bowjoin.go:383-400 runs per common column).  Key columns may sit at different positions in the two frames.
 *   n_keys == 0 is the no-common-column join: exactly bowgpu_join with -1 / -1 (bowgpu_join_rows with NULL keys).  n_keys == 1 is
 * bowgpu_join / bowgpu_join_rows itself: the same code, bytes, *rows / *pairs and workspace.
 *   ERRORS, all raised before the device is touched when the arguments are host-resident: n_keys < 0 is BOWGPU_ERR_ARG; n_keys >
 * BOWGPU_JOIN_MAX_KEYS is BOWGPU_ERR_UNSUPPORTED naming the limit; a key index outside its frame BOWGPU_ERR_BAD_COL; a column listed
 * twice among one side's keys BOWGPU_ERR_ARG; key pair types that differ BOWGPU_ERR_TYPE with the one-key join's text; Boolean / String
 * anywhere BOWGPU_ERR_UNSUPPORTED; unequal lengths within a frame (for bowgpu_join_keys_rows: among one side's keys) BOWGPU_ERR_ARG.
 *   ROW LIMITS: each side and the result hold fewer than 2^31 rows, as for the one-key join.  For n_keys >= 2 also L + R < 2^31: the
 * surrogate pass sorts both sides as one column and the argsort is 31-bit.  More is BOWGPU_ERR_UNSUPPORTED naming the limit.
 *   CAPACITY, NO DEVICE and FAILURE are the one-key join's rules unchanged: bowgpu_out.length on entry, too small names the size needed
 * and writes nothing; the NULL-buffer call of bowgpu_join_keys_rows is the count; no device is needed when both frames are empty, for an
 * INNER with an empty side and for the COUNT of an OUTER with an empty side; outputs are untouched on every failure; the same call gives
 * the same bytes.  bowgpu_set_devices does not apply.
 *   THE METHOD for n_keys >= 2 (bow_amd/csrc/join_keys.hip): the key tuples of both sides are reduced to ONE Int64 surrogate column per
 * side - equal exactly when the tuples are, without nulls or NaN - and the one-key join above runs on those as it stands.  Nothing is
 * hashed; every step is an integer count.  Per key pair the left then the right key are written into one column of L + R slots (raw bits,
 * 0 under a null), bowgpu_argsort's sort runs over it (digit skipping and the "already in order" answer apply), the heads of the groups
 * of equal images are marked over the sorted order and scanned, and every original row receives 1 + its dense rank, a row with a null key
 * rank 0.  Two keys: the surrogate is rank_0 << 32 | rank_1.  More: the packed pair is ranked again the same way and packed with the next
 * rank - n_keys + (n_keys - 2) argsorts of L + R rows in front of the one-key join's own sort of R rows.
 *   HBM WORKSPACE for n_keys >= 2, on top of the one-key join's own, per row of L + R: 8 bytes for the concatenated column, the argsort's
 * 24 (none when the column is in order), 4 for the marks, two live rank arrays of 4 each, 8 for the packed column - the buffers of one key
 * pair go back before the next one's are taken.  + the staged copies of BOWGPU_HOST key columns (values and bitmap) of both sides, held for
 * the whole call: bowgpu_join_keys_rows lets them go before the join proper, bowgpu_join_keys keeps them for the gather. */
#define BOWGPU_JOIN_MAX_KEYS 8

int bowgpu_join_keys_rows(const bowgpu_col *left_keys, const bowgpu_col *right_keys, int32_t n_keys, int32_t kind, int64_t *l_idx,
                          int64_t *r_idx, int64_t idx_capacity, int32_t idx_residency, int64_t *rows, int64_t *pairs);

int bowgpu_join_keys(const bowgpu_col *left_cols, int32_t n_left, const int32_t *left_keys, const bowgpu_col *right_cols, int32_t n_right,
                     const int32_t *right_keys, int32_t n_keys, int32_t kind, bowgpu_out *outs, int64_t *rows);

/* ---- Parquet column chunk -> device column --------------------------- */

/* Reads INT64 / DOUBLE columns of a Parquet file the way the reference's NewBowFromParquet does (bowparquet.go:44-153), but
 * decodes on the device: the column's compressed pages are uploaded as they lie in the file and decompressed (Snappy), their
 * definition levels turned into an Arrow validity bitmap and their PLAIN values scattered to row slots by HIP kernels.
 * Read: flat schemas, OPTIONAL / REQUIRED columns, UNCOMPRESSED / SNAPPY, RLE definition levels, data page v1 and v2, and these
 * value encodings, which a column chunk may mix page by page: PLAIN; PLAIN_DICTIONARY / RLE_DICTIONARY (with PLAIN or delta
 * fall-back pages); DELTA_BINARY_PACKED on INT64 columns (any legal block / miniblock size); BYTE_STREAM_SPLIT on INT64 and
 * DOUBLE columns - what the reference writes (bowparquet.go:326-338), what pyarrow / pandas write by default, and what Parquet v2
 * writers (parquet-mr / Spark with writer.version=v2, pyarrow with column_encoding) choose for these two types.  Anything else -
 * other codecs, types and encodings, DELTA_BINARY_PACKED on a DOUBLE column, nested schemas: BOWGPU_ERR_UNSUPPORTED.  Damaged page
 * data: BOWGPU_ERR_ARG - a dictionary index stream or definition levels that end before the page's values or rows do included. */
typedef struct bowgpu_parquet bowgpu_parquet;
int bowgpu_parquet_open(const char *path, bowgpu_parquet **handle);
int bowgpu_parquet_close(bowgpu_parquet *handle);
int bowgpu_parquet_info(const bowgpu_parquet *handle, int64_t *num_rows, int32_t *num_columns);
/* name (NUL-terminated, truncated to name_cap), type (BOWGPU_INT64 / BOWGPU_FLOAT64 / BOWGPU_BOOLEAN / BOWGPU_STRING / -1) and
 * whether the column is OPTIONAL (may hold nulls) */
int bowgpu_parquet_column(const bowgpu_parquet *handle, int32_t i, char *name, int32_t name_cap, int32_t *type, int32_t *optional);
/* out: num_rows slots (HOST or DEVICE residency); values, validity, null_count and type are filled in */
int bowgpu_parquet_read_column(bowgpu_parquet *handle, int32_t i, bowgpu_out *out);
/* Whether bowgpu_parquet_read_column would accept column i's structure - type, codec, page types, value and level encodings,
 * sizes: the same walk over the page headers of every row group, on the host alone (no device is touched, none is needed).  0, or
 * the error code and bowgpu_last_error text bowgpu_parquet_read_column would give.  value_encodings (may be NULL): bit e set for
 * every Parquet Encoding value e found on a data page (BOWGPU_PARQUET_ENC_*). */
enum {
    BOWGPU_PARQUET_ENC_PLAIN = 1,                  /* 1 << 0 */
    BOWGPU_PARQUET_ENC_PLAIN_DICTIONARY = 4,       /* 1 << 2 */
    BOWGPU_PARQUET_ENC_RLE = 8,                    /* 1 << 3 (BOOLEAN columns: bowgpu_parquet_bool_column_check) */
    BOWGPU_PARQUET_ENC_DELTA_BINARY_PACKED = 32,   /* 1 << 5 */
    BOWGPU_PARQUET_ENC_RLE_DICTIONARY = 256,       /* 1 << 8 */
    BOWGPU_PARQUET_ENC_BYTE_STREAM_SPLIT = 512     /* 1 << 9 */
};
int bowgpu_parquet_column_check(const bowgpu_parquet *handle, int32_t i, uint32_t *value_encodings);

/* Column i, of physical type BOOLEAN in a flat schema (OPTIONAL or REQUIRED; bowgpu_parquet_column reports BOWGPU_BOOLEAN), decoded on
 * the device into a BOWGPU_BOOLEAN output in the layout bowgpu_convert and the Boolean reducers use: values bit-packed LSB first,
 * ceil(num_rows / 8) bytes, validity ceil(num_rows / 8) bytes, null_count exact; the value bit of a null row is 0 (what
 * bow.NewBuffer leaves, bowbuffer.go:22-40) and so is every bit at or past num_rows in the last byte of both buffers.  out: num_rows
 * slots, any residency; its values buffer needs ceil(num_rows / 8) bytes.
 * Read: value encodings PLAIN (one bit per non-null value, LSB first) and RLE (a 4-byte little-endian length, then the RLE /
 * bit-packed hybrid at bit width 1), also mixed page by page inside a chunk; data pages v1 and v2; UNCOMPRESSED and SNAPPY; RLE
 * definition levels; any number of row groups.
 * BOWGPU_ERR_UNSUPPORTED, with the column named and before a device is touched: a column that is not BOOLEAN (INT64 / DOUBLE go
 * through bowgpu_parquet_read_column), a nested schema, any other value encoding (dictionary pages included), codec or
 * definition-level encoding.  BOWGPU_ERR_ARG and nothing handed to the caller: malformed page data - a PLAIN values section shorter
 * than ceil(valid / 8) bytes, an RLE length prefix that runs past the page, a run stream that ends before the page's values do,
 * levels that end before the rows do, implausible page sizes. */
int bowgpu_parquet_read_bool_column(bowgpu_parquet *handle, int32_t i, bowgpu_out *out);
/* The host-only twin of bowgpu_parquet_read_bool_column (no device is touched, none is needed): 0, or the code and text it would
 * give about the column's structure.  value_encodings (may be NULL): BOWGPU_PARQUET_ENC_PLAIN and / or BOWGPU_PARQUET_ENC_RLE. */
int bowgpu_parquet_bool_column_check(const bowgpu_parquet *handle, int32_t i, uint32_t *value_encodings);

/* ---- device column -> Parquet file -------------------------------------------------- */

/* Writes a frame of Int64 / Float64 columns to a Parquet file the way the reference's Bow.WriteParquet lays one out
 * (bowparquet.go:157-253), minus its codec, with the encoding done on the device: per row group and column the validity bits are
 * cut into the pages' definition levels, the non-null values are compacted, min / max are reduced and - for
 * DELTA_BINARY_PACKED - the values are delta-packed by HIP kernels; only the encoded bytes cross the host link, once.
 *
 * The file: format version 1; flat schema with root `Schema`; every column OPTIONAL whatever its null count (bowparquet.go:190);
 * INT64 / DOUBLE; UNCOMPRESSED; data page v1; definition levels as RLE / bit-packed hybrid of bit width 1; created_by names the
 * library; key_value_metadata from the options.  One row group per row_group_rows rows (the last may be shorter), in it one
 * column chunk per column in column order, in it one page per page_rows rows (the last may be shorter).
 * Levels of a page: all rows valid - one RLE run of 1; no row valid - one RLE run of 0; otherwise one bit-packed run whose bytes
 * are the page's validity bits from bit 0, padded with zero bits to a whole group of 8.
 * PLAIN: the page's non-null values, 8 bytes each, in row order.
 * DELTA_BINARY_PACKED (Int64 columns): blocks of 128 in 4 miniblocks of 32 (parquet-mr's layout for INT64) over the page's
 * non-null values; wrapping differences; the block minimum is the true minimum; each miniblock has its minimal bit width; the
 * last miniblock that holds values is padded with zero bits; miniblocks behind it have width byte 0 and no body; a page without a
 * valid row holds the header alone (block size 128, 4 miniblocks, 0 values, first value 0).
 * RLE_DICTIONARY (encoding 8, Int64 / Float64 columns), per column chunk, over the chunk's non-null values:
 *   the dictionary holds the distinct values by 64-bit pattern (-0.0 and +0.0 are two entries, as are two NaNs of different payload;
 *   nothing is declined), ascending as unsigned 64-bit integers of the little-endian payload, for both types (negative Int64 values
 *   come last); at most BOWGPU_PARQUET_DICT_MAX entries.  A chunk with more distinct patterns, or without a valid row, is written
 *   PLAIN, byte for byte what encoding 0 gives for that chunk: the decision is per chunk, so a column may be dictionary-encoded in
 *   one row group and PLAIN in the next, and the caller learns what happened from bowgpu_parquet_column_check on the written file
 *   (its value_encodings mask).  The dictionary page comes first in the chunk (PageHeader.type = DICTIONARY_PAGE,
 *   DictionaryPageHeader{num_values = entries, encoding = PLAIN}, the entries at 8 bytes each).  The data pages are v1 with encoding 8
 *   and levels as above; a values section is one byte for the bit width w = max(1, bit_length(entries - 1)) and, where the page has
 *   k > 0 non-null values, one bit-packed run: varint((ceil(k / 8) << 1) | 1), then the k indices at w bits each, LSB first, padded
 *   with zero bits to a whole group of 8 values.  A page with k = 0 holds the width byte alone; there are no RLE runs.
 *   ColumnMetaData: encodings RLE_DICTIONARY, PLAIN, RLE; dictionary_page_offset is the chunk's first byte, data_page_offset the
 *   first data page; total_uncompressed_size / total_compressed_size include the dictionary page and its header; statistics as
 *   for every encoding.
 * Statistics (TYPE_DEFINED_ORDER): null_count always; min_value / max_value with options.statistics - Int64 signed; a NaN takes
 * no part in a Float64 min / max; both are left out when no valid non-NaN value exists; a zero minimum is written as -0.0, a
 * zero maximum as +0.0.
 *
 * Accepted: Int64 / Float64 columns of the three residencies, any Arrow offset (bit offsets that are no multiple of 8 included),
 * validity NULL or null_count 0 / -1, 0 rows (a file with a schema and no row group), up to 2^31 - 1 rows.
 * Declined, with nothing left at `path`: Boolean / String columns, an encoding other than 0 / 5 / 8 (2, PLAIN_DICTIONARY, among
 * them), encoding 5 on a Float64 column (BOWGPU_ERR_UNSUPPORTED); columns of unequal length, ncols < 1, a NULL or empty name, the same name twice, sizes that break the
 * rules below, reserved != 0 (BOWGPU_ERR_ARG) - all before any device is touched; no device (BOWGPU_ERR_NO_DEVICE: there is no CPU
 * fallback).  The file is written as `<path>.tmp` and renamed on success; on any failure the temporary is removed, a failure to
 * create or write it is BOWGPU_ERR_ARG with the errno text.  The reference's ".parquet" suffix rule is the caller's business.
 * Device workspace is bounded by row_group_rows. */
#define BOWGPU_PARQUET_DICT_MAX 65536   /* entries of one column chunk's dictionary at the most: 512 KiB, index width at most 16 */
typedef struct {
    int64_t row_group_rows;       /* 0: 1 << 24.  A multiple of page_rows, at most 1 << 27 */
    int32_t page_rows;            /* 0: 65536.  A multiple of 64, at most 1 << 20: rows (nulls included) per data page */
    int32_t statistics;           /* 1: min_value / max_value / null_count per column chunk, and column_orders in the footer; 0: null_count only */
    const int32_t *encodings;     /* NULL: PLAIN everywhere; else ncols entries, each Parquet Encoding 0 (PLAIN), 5 (DELTA_BINARY_PACKED, Int64 columns only) or 8 (RLE_DICTIONARY) */
    const char *const *meta_keys; /* n_meta key / value pairs for the footer's key_value_metadata (Bow.Metadata) */
    const char *const *meta_values;
    int32_t n_meta;
    int32_t reserved;             /* 0 */
} bowgpu_parquet_write_options;

/* what was written: the file's size, its rows, row groups and data pages, the bytes of the definition-level sections (each with
 * its 4-byte length) and of the values sections.  With RLE_DICTIONARY chunks: data_pages counts data pages only, value_bytes
 * includes the body of every dictionary page (8 bytes an entry) */
typedef struct { int64_t file_bytes, rows, row_groups, data_pages, level_bytes, value_bytes; } bowgpu_parquet_write_info;

int bowgpu_parquet_write(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                         const bowgpu_parquet_write_options *opts /* NULL: defaults */, bowgpu_parquet_write_info *info /* nullable */);

/* bowgpu_parquet_write with a compression codec (a Parquet CompressionCodec value): the file the reference's writer produces,
 * which compresses with SNAPPY (bowparquet.go:326-338).
 *   0 (UNCOMPRESSED): the file bowgpu_parquet_write writes for the same arguments, byte for byte.
 *   1 (SNAPPY): every data page's section is one raw Snappy stream of [4-byte levels length | levels | values].  The values are
 *     compressed on the device, so only the compressed bytes cross the host link: a page's values section is cut into fragments of
 *     4 KiB, one wavefront compresses one fragment on its own (back-references stay inside the fragment and use the 1- or 2-byte-offset
 *     copy forms, copies are 4 .. 64 bytes), and the fragments' element sequences follow each other behind the preamble and the
 *     literal that holds the levels, which the host writes.  The stream is a function of the page's bytes alone; a page's values
 *     never take more than 32 + n + n / 6 bytes for n bytes.  PageHeader carries uncompressed_page_size and compressed_page_size,
 *     ColumnMetaData codec = 1 and total_uncompressed_size / total_compressed_size (page headers counted in both).  Levels forms,
 *     value encodings, statistics, row groups, metadata, the temporary and its removal are those of bowgpu_parquet_write.
 *     A dictionary page's body (RLE_DICTIONARY) is a raw Snappy stream of the preamble and literal elements of at most 64 KiB,
 *     written by the host; the index sections of its data pages are compressed on the device like any other values section.
 *   any other value: BOWGPU_ERR_UNSUPPORTED, before any device or the file system is touched, as are all declines of
 *     bowgpu_parquet_write, which apply unchanged.
 * info: level_bytes / value_bytes stay the uncompressed section sizes; file_bytes is the file as written. */
int bowgpu_parquet_write_codec(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                               const bowgpu_parquet_write_options *opts /* NULL: defaults */, int32_t codec,
                               bowgpu_parquet_write_info *info /* nullable */);

/* bowgpu_parquet_write_codec with BOWGPU_BOOLEAN columns admitted next to Int64 / Float64: a Boolean column leaves as the Parquet BOOLEAN
 * column bowgpu_parquet_read_bool_column reads (the reference maps Type_BOOLEAN to Boolean, bowparquet.go:21,28).  A call without a
 * Boolean column writes, byte for byte, the file bowgpu_parquet_write_codec writes for the same arguments.
 *   A Boolean column in the file: SchemaElement of physical type BOOLEAN (0), OPTIONAL; data page v1, value encoding PLAIN (0);
 *   definition levels in the forms of bowgpu_parquet_write.  A page's values section holds the value bits of its k valid rows in row
 *   order, one bit each, LSB first, ceil(k / 8) bytes, the padding bits of the last byte 0; k = 0: an empty section.  The bits are taken
 *   out from between the null rows and packed on the device, one pass over the column's two bit ranges per row group; every byte is a
 *   function of the input alone.
 *   Input: bowgpu_col.type == BOWGPU_BOOLEAN, values and validity Arrow bit-packed (bit offset + i is row i), any byte address, any
 *   offset (no multiple of 8 included), the three residencies; validity NULL or null_count 0: every row is valid.  Value bits of null
 *   rows and bits outside the slice may hold anything: none reaches the file.
 *   options.encodings[i] of a Boolean column must be 0: 3 (RLE), 5, 8 and every other value are BOWGPU_ERR_UNSUPPORTED with the column
 *   named.  A String column stays BOWGPU_ERR_UNSUPPORTED.  Every decline and every BOWGPU_ERR_ARG rule of bowgpu_parquet_write applies
 *   unchanged, before a device or the file system is touched.
 *   Statistics of a Boolean column chunk: null_count always; with options.statistics min_value / max_value of ONE byte each (0x00 / 0x01,
 *   false < true): the minimum is false iff some valid row is false, the maximum true iff some valid row is true; both are left out when
 *   the chunk has no valid row.
 *   codec: 0 and 1 (SNAPPY) as for bowgpu_parquet_write_codec; under SNAPPY a Boolean page's values section is compressed on the device
 *   like any other.
 *   info: value_bytes counts ceil(k / 8) per Boolean page, level_bytes as before.
 * Not written: RLE value runs, data page v2. */
int bowgpu_parquet_write_bool(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                              const bowgpu_parquet_write_options *opts /* NULL: defaults */, int32_t codec,
                              bowgpu_parquet_write_info *info /* nullable */);

/* ---- row-range sharded Rolling.Aggregate across GPUs: the records the ranks exchange ------------------ */

/* Running state of one reducer over the rows a rank holds of a window that straddles a shard
 * boundary: what the reference's loops carry from one row to the next (sum.go:15-22,
 * arithmeticmean.go:15-24, minmax.go:14-28, count.go:12-18, firstlast.go).  Fixed size so a
 * rank's record travels through one RCCL all_gather; nn_min / nn_max (NaN-ignoring extrema) are
 * only consulted when more than two ranks share one window. */
typedef struct bowgpu_carry_state {
    double sum;
    double vmin, vmax;
    double nn_min, nn_max;
    uint64_t first_bits, last_bits;   /* First / Last raw 64-bit payloads */
    int64_t count;                    /* valid values */
    int64_t nrows;                    /* rows (w.Bow.NumRows() contribution) */
    /* time-weighted reducers (integral.go:14-31, :46-62): last and first both-valid point, running sums */
    double pt, pv, first_pt, first_pv;
    double integ_step, integ_trap;
    int32_t has_value;
    int32_t has_nn;
    int32_t has_point;
    int32_t has_pair;
} bowgpu_carry_state;

/* The first row of the next non-empty shard to the right, per aggregator: what an INCLUSIVE window that ends exactly where
 * this shard's rows end needs from its successor (rolling.go:201-209).  Fixed size: it rides in the rank's record
 * (bowgpu_shard_record.first_row). */
typedef struct bowgpu_next_row {
    int32_t present;                  /* 0: there is no row to the right */
    int32_t _pad;
    int64_t ts;
    uint64_t bits[16];                /* value of each aggregator's input column at that row */
    int32_t valid[16];
} bowgpu_next_row;

#define BOWGPU_CARRY_MAX_AGGS 16

/* left (earlier rows) then right: the state of the concatenation.  Pure bookkeeping on two
 * states (no column data); Sum is left.sum + right.sum, i.e. NOT the row-order association.
 * bowgpu_shard_finish applies it to the records of the ranks to the left when one window spans
 * three or more ranks (the seed of the right rank's re-walk). */
int bowgpu_carry_merge(const bowgpu_carry_state *left, const bowgpu_carry_state *right,
                       bowgpu_carry_state *out);

/* ---- the shard protocol behind the ABI: begin -> ONE exchange -> finish ------------------------------------------
 * What a host (the cgo shim inside reference rolling/aggregation.go:123-145, or bow_amd/sharded.py here) does per
 * Rolling.Aggregate over R ranks:
 *     bowgpu_shard_begin(my columns)            -> my record             (fixed size)
 *     all_gather of the records as bytes        (RCCL over xGMI / any transport: the ONLY exchange of the call)
 *     bowgpu_shard_finish(my columns, records)  -> my output slots + which global windows they are
 * All ownership rules (which rank outputs a window that straddles a boundary, who emits the empty windows between two
 * shards, whose running state seeds whose first window, who needs whose first row for an inclusive window) are decided
 * inside the library from the gathered records; every rank derives the same decisions from the same bytes. */
typedef struct bowgpu_shard_record {
    int64_t nrows, first_ts, last_ts;      /* of this rank's interval column (0 rows: the rest is zero) */
    int64_t carry_from_ts;                 /* the running states below cover this rank's rows with ts >= carry_from_ts:
                                              the start, on the offset-aligned window grid, of the window holding last_ts
                                              (INT64_MIN: all of the rank's rows) */
    int32_t naggs;
    int32_t flags;                         /* bit 0: built with the global first window start known (second attempt) */
    bowgpu_next_row first_row;             /* this rank's first row (filled when some reducer needs inclusive windows) */
    bowgpu_carry_state last[BOWGPU_CARRY_MAX_AGGS];  /* per aggregator: running state of the rank's LAST window over its rows */
} bowgpu_shard_record;

/* What bowgpu_shard_plan decides for one rank. */
typedef struct bowgpu_shard_decision {
    int64_t s0;                     /* global first window start (rolling.go:95-99 on the first row of the first non-empty rank) */
    int64_t num_windows;            /* global W (rolling.go:143-154) */
    int64_t first_window_id;        /* global id of the first / last window with a row on this rank; -1: no rows */
    int64_t last_window_id;
    int64_t lead_empty_windows;     /* empty windows in front of first_window_id that this rank outputs too */
    int64_t first_slot_window_id;   /* global window id of output slot 0 (= first_window_id - lead_empty_windows); -1: none */
    int64_t windows_local;          /* output slots this rank writes */
    int64_t windows_owned;          /* ... of which it owns the first windows_owned (a last window that continues on a rank
                                       to the right belongs to that rank) */
    int32_t holds_global_row0;
    int32_t drops_last;
    int32_t seed_first_rank;        /* ranks seed_first_rank .. rank-1 hold earlier rows of this rank's first window; -1: none */
    int32_t next_rank;              /* next rank to the right that holds rows; -1: none */
    int32_t finish_last;            /* this rank folds next_rank's first row into its last window during the pass */
    int32_t retry_with_s0;          /* 1: the records cannot settle window 0 (rows below s0, rolling.go:96-99 with negative
                                       timestamps, split across ranks): run bowgpu_shard_begin again with &s0 and exchange again */
} bowgpu_shard_decision;

#define BOWGPU_SHARD_RETRY 1   /* bowgpu_shard_finish: nothing was computed; see retry_with_s0 */
#define BOWGPU_SHARD_PASS_DECLINED 1   /* bowgpu_shard_pass_begin: nothing was enqueued (not an error); bowgpu_shard_finish runs the pass */

/* Columns and outputs of the three calls below: any residency since ABI 5.  Host-resident ones are staged through HBM per call
 * the way bowgpu_rolling_aggregate stages them (so begin + pass_begin move each column over PCIe twice, once for the record and
 * once for the pass; a pass put in flight keeps its staged copies until bowgpu_shard_finish collects it).
 * global_s0: NULL on the first attempt. */
int bowgpu_shard_begin(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                       const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs,
                       const int64_t *global_s0, bowgpu_shard_record *record);
/* The exchange off the critical path (comms row): between bowgpu_shard_begin and bowgpu_shard_finish a host may call
 *     bowgpu_shard_pass_begin(my columns, my outputs, my record)
 * which ENQUEUES the rank's pass over its rows and returns at once - the all_gather of the records then travels while the kernel
 * runs.  The pass assumes what is true of every rank but the odd one: no empty windows between its left neighbour's rows and its
 * own, no row below the frame's first window start.  bowgpu_shard_finish on the same thread collects it when the gathered records
 * agree (same columns, outputs, options, aggregators) and discards it otherwise; results are the same bytes either way.  At most
 * one pass per thread is in flight; no other bowgpu call of this thread may come between the two except bowgpu_shard_plan.
 * Returns 0, BOWGPU_SHARD_PASS_DECLINED (empty shard, negative timestamps: nothing enqueued), or a negative error. */
int bowgpu_shard_pass_begin(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                            const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                            const bowgpu_shard_record *my_record);
/* Pure host arithmetic on the gathered records (no device, no column data): usable from any process. */
int bowgpu_shard_plan(const bowgpu_shard_record *records, int32_t world, int32_t rank, int64_t interval,
                      int64_t raw_offset, bowgpu_shard_decision *out);
/* The rank's pass + stitch.  outs: any residency (the ones given to bowgpu_shard_pass_begin), capacity >= (last_ts - first_ts) / interval + 2 + lead (or simply
 * global W).  Returns 0, BOWGPU_SHARD_RETRY, or a negative error. */
int bowgpu_shard_finish(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, int64_t interval,
                        const bowgpu_options *opts, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs,
                        const bowgpu_shard_record *records, int32_t world, int32_t rank,
                        bowgpu_shard_decision *decision /* nullable */, bowgpu_agg_info *info /* nullable */);

/* ---- ONE Rolling.Aggregate over a frame held as row-range shards on several devices --------------------------------
 * The C ABI's one call (reference rolling/aggregation.go:123-145) for a frame too large for one GPU: the shard protocol above runs
 * inside the library, on one persistent library thread per list entry, with its exchange in host memory.
 *   THE FRAME.  cols_by_rank[r] holds ncols columns: rank r's rows.  Every rank has the same schema (types, ts_col); the shards
 * concatenated in rank order are the frame.  Ranks may be empty (length 0), all of them too.  1 <= world <= 64.  device_ids[r]: the
 * device rank r runs on (else BOWGPU_ERR_NO_DEVICE); an id may be listed several times - how a one-GPU box runs the path.
 *   RESIDENCY.  Columns and outputs: any residency.  A BOWGPU_DEVICE buffer of rank r must live on device_ids[r] (checked with
 * hipPointerGetAttributes: BOWGPU_ERR_ARG naming the rank).  Pageable (BOWGPU_HOST) columns are staged through HBM once per rank.
 *   LAYOUT QUERY.  outs_by_rank == NULL: only `decisions` is filled, from each rank's row count and first / last timestamp; nothing
 * else is read and no pass runs.  These are the decisions the full call takes (retry_with_s0 is 0).  Host-resident interval columns
 * make it host arithmetic, with no GPU needed (as bowgpu_plan_windows); a device-resident one is read on device_ids[r].
 *   OUTPUTS.  outs_by_rank[r][i] is output i of rank r, capacity (length on entry) >= decisions[r].windows_local, else BOWGPU_ERR_ARG
 * naming the size.  On return: length = windows_owned, slot k holds global window first_slot_window_id + k, null_count counts the
 * nulls of those slots only, type as bowgpu_rolling_aggregate resolves it.  A rank does not own a last window that continues on the
 * next non-empty rank (that rank outputs it): where the pass wrote it, its value slot ends up 0 and its validity bit 0.  Every
 * validity bit the call writes at or past length is 0.  Each rank's outputs are its own buffers: no byte is shared between ranks.
 *   THE GUARANTEE: slots [0, windows_owned) of output i concatenated over the ranks in rank order are, bit for bit, what
 * bowgpu_rolling_aggregate gives for the concatenated frame on one device - values, validity and null counts - except for the
 * generated-NaN bits this header excludes everywhere (bowgpu_agg_info.long_windows); when info.long_windows != 0 the bound stated
 * there applies instead.
 *   INFO (nullable): s0, num_windows, new_interval_col and inclusive of the one-device call; long_windows: the ranks' sum, where a
 * rank also counts the window it owns that is spread over three or more ranks (the middle ranks' running states are merged,
 * bowgpu_carry_merge: an order-free form of its Sum / ArithmeticMean / Integral* / WeightedAverage*); kernel_ms: the slowest rank's.
 *   DECLINES ARE ERRORS HERE: no single device holds the frame, so there is nothing to fall back to.  Mode or more than 16
 * aggregators: BOWGPU_ERR_UNSUPPORTED; an interval column with nulls on any rank: BOWGPU_ERR_TS_NULLS; strict_order with a window
 * spread over three or more ranks: BOWGPU_ERR_UNSUPPORTED; timestamps not ascending within a rank or across ranks:
 * BOWGPU_ERR_TS_UNSORTED.  Validation errors (INTERVAL, TS_TYPE, NO_AGG, KEEP_INTERVAL, BAD_COL, and the type whitelist's
 * UNSUPPORTED) are those bowgpu_rolling_aggregate returns for the same frame.  A rank whose columns differ from rank 0's in type, or
 * whose columns differ in length, is BOWGPU_ERR_ARG.  On any error the outputs are undefined; the first error's code and message
 * are the call's.
 *   ORDERING.  Inputs must be complete when the call is made: it first synchronises the calling thread's stream (work on other streams
 * is the caller's to finish) - the layout query too, when it reads a device-resident interval column.  On return every output is
 * complete.
 *   INDEPENDENT of bowgpu_set_devices: neither reads nor changes the device list or min_rows, does not count in bowgpu_fanout_counts,
 * leaves bowgpu_last_call_ranks alone.  Calls of this entry point are serialised process-wide. */
int bowgpu_rolling_aggregate_sharded(const bowgpu_col *const *cols_by_rank, const int32_t *device_ids, int32_t world,
                                     int32_t ncols, int32_t ts_col, int64_t interval, const bowgpu_options *opts,
                                     const bowgpu_agg *aggs, int32_t naggs,
                                     bowgpu_out *const *outs_by_rank,   /* NULL: layout query only */
                                     bowgpu_shard_decision *decisions,  /* world entries, always filled */
                                     bowgpu_agg_info *info);            /* nullable */

/* ---- synthetic inputs generated in HBM -------------------------------- */

/* cfg-dense: ts[i] = row0+i, val[i] = u01(mix64(seed, row0+i)); device pointers. */
int bowgpu_gen_dense(int64_t row0, int64_t n, uint64_t seed, int64_t *ts_dev, double *val_dev);
/* cfg-sparse: ts = 10*i + U{0..9}, val = U{0..9}+0.5, P(valid) = 0.7; validity_dev holds
 * ceil(n/8) bytes, bit i = row row0+i (row0 must be a multiple of 8). */
int bowgpu_gen_sparse(int64_t row0, int64_t n, uint64_t seed, int64_t *ts_dev, double *val_dev,
                      uint8_t *validity_dev);
/* The "achievable" line next to the 8 TB/s peak: best rate (GB/s) of a trivial streaming sum over two device
 * buffers of bytes_each bytes (16-byte aligned), tried in a few launch shapes.  Measurement aid for bench.py. */
int bowgpu_stream_read_ceiling(const void *dev_a, const void *dev_b, int64_t bytes_each, double *gb_per_s);
/* The achievable line for the benched traffic MIX: the same two 8-byte-per-row input streams read by a trivial kernel that also
 * writes two output streams of 8 bytes per `rows_per_slot` rows (out_a / out_b: device buffers of ceil(rows / rows_per_slot)
 * 8-byte slots) in the tile kernels' store pattern.  Best of plain / non-temporal loads; the rate counts the bytes READ, like
 * roofline.achieved does.  Measurement aid for bench.py ("stream_rw_probe"). */
int bowgpu_stream_rw_probe(const void *dev_a, const void *dev_b, int64_t bytes_each, void *out_a, void *out_b,
                             int64_t rows_per_slot, double *read_gb_per_s, double *ms /* nullable */);
/* Per-thread route mask.  Which kernel serves a call follows from the call's shape alone; two bits are a caller's business:
 *   BOWGPU_ROUTE_STRICT_ORDER  bowgpu_options.strict_order for every call of the thread
 *   BOWGPU_ROUTE_PINNED_STAGE  BOWGPU_HOST_PINNED inputs staged through HBM instead of read in place over the host link
 * The remaining bits (bow_amd/csrc/debug_routes.h, not part of the ABI) let the parity tests push one call through every kernel
 * that can take it; all routes give the same results where several apply.  The library never reads the environment on the call
 * path; BOWGPU_ROUTE=<mask> is read once per process as every thread's initial mask (profiling an unmodified script). */
enum {
    BOWGPU_ROUTE_PINNED_STAGE = 1024,
    BOWGPU_ROUTE_STRICT_ORDER = 2048
};
int bowgpu_debug_set_route(uint32_t mask);
int bowgpu_debug_get_route(uint32_t *mask);

/* Diagnostic builds only (kernels compiled with in-kernel stamps): words [first, first + n) of the calling thread's device
 * status block; zero_after clears them.  The product build never writes those words. */
int bowgpu_debug_status(int32_t first, int32_t n, uint32_t *out, int32_t zero_after);
/* The CPU side of the staging of pageable buffers on its own (no device involved): a memcpy split over the library's helper threads
 * (BOWGPU_COPY_THREADS).  For the sanitizer run of the host code and for measuring the host's copy rate. */
int bowgpu_debug_host_copy(void *dst, const void *src, int64_t bytes);
/* order-independent 64-bit checksum of a device buffer of n 8-byte words (xor / sum of mix) */
int bowgpu_checksum64(const void *dev, int64_t n_words, uint64_t *xor_out, uint64_t *sum_out);
/* ... of words that are words [index_base, index_base + n_words) of a larger array: the checksums of the pieces of an array
 * combine (xor with xor, sum with sum, mod 2^64) into the checksum of the whole - sharded outputs against the unsharded ones
 * without bringing either to the host */
int bowgpu_checksum64_at(const void *dev, int64_t n_words, int64_t index_base, uint64_t *xor_out, uint64_t *sum_out);

#ifdef __cplusplus
}
#endif
#endif
