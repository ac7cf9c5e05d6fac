// long_windows.hip — windows too long for one tile (more rows than a tile's look-ahead), down to ONE window over
// the whole frame.  The tile kernels queue such windows as (window id, first row); here they are reduced by a
// coalesced, multi-workgroup, ORDER-FREE formulation of the same reducers (reference rolling/aggregation/*.go):
//
//   Sum / Mean      sum and count of valid values (any association => Sum/Mean/Integral agree with the reference's
//                   left-to-right sum within 1e-12 relative; every other output is bit-exact)
//   Min / Max       minmax.go seeds with the FIRST valid value and replaces on strict < / >: equivalently
//                   "NaN iff the first valid value is NaN, else the extreme of the non-NaN values, ties (e.g. -0.0 /
//                   +0.0) resolved by the smallest row index"  -> (value, row index) pairs merge in any order
//   First / Last    smallest / largest valid row index
//   Integrals       integral.go walks consecutive both-valid points: each valid row contributes one term with its NEXT
//                   valid row (looked up forward, across chunk boundaries), so the terms sum in any order
//
// Launches: long_bounds (end row of each window by bisection + chunk counts) -> exclusive scan -> long_map ->
// long_partial (one wavefront per 4096-row chunk) -> long_final (merge in chunk order, outputs,
// empty windows after it).
#include "long_device.h"

namespace bowgpu {

__global__ __launch_bounds__(256) void long_bounds_kernel(const AggParams p, const LongListStarts starts, LongEntry *entries,
                                                          int32_t *nchunks) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= starts.start[kLongLists]) return;
    int sub = 0;
    while (starts.start[sub + 1] <= e) sub++;
    const int64_t *item = p.long_list + 2 * (sub * p.long_cap + (e - starts.start[sub]));
    const uint64_t wid = (uint64_t)item[0];
    const int64_t r0 = item[1];
    const int64_t win_start = p.s0 + (int64_t)(wid * (uint64_t)p.interval);
    // first row >= r0 with ts >= win_start + interval (rolling.go:197-209), by bisection
    const int64_t lim = win_start + p.interval;
    const bool ovf = lim < win_start;  // int64 overflow: no row can reach it
    int64_t lo = r0 + 1, hi = p.n;
    while (lo < hi && !ovf) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (p.ts[mid] >= lim) hi = mid; else lo = mid + 1;
    }
    const int64_t r1 = ovf ? p.n : lo;
    LongEntry le;
    le.wid = wid; le.r0 = r0; le.r1 = r1;
    entry_close(p, le);
    entries[e] = le;
    nchunks[e] = (int32_t)((r1 - r0 + kChunkRows - 1) / kChunkRows);
}

// Every window of the call as an entry (the "long-only" pipeline: when windows average thousands of rows the tile kernels
// would read every row just to queue almost every window here, so the host skips them): r0 / r1 by bisection.
__global__ __launch_bounds__(256) void long_bounds_all_kernel(const AggParams p, LongEntry *entries, int32_t *nchunks) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.W) return;
    const uint64_t wid = (uint64_t)(p.wid_base + k);
    const int64_t win_start = p.s0 + (int64_t)(wid * (uint64_t)p.interval);
    auto lower_bound = [&](int64_t v) {
        int64_t lo = 0, hi = p.n;
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (p.ts[mid] >= v) hi = mid; else lo = mid + 1; }
        return lo;
    };
    const int64_t lim = win_start + p.interval;
    const int64_t r0 = wid == 0 ? 0 : lower_bound(win_start);  // rows below s0 ride in window 0
    const int64_t r1 = lim < win_start ? p.n : lower_bound(lim);
    LongEntry le;
    le.wid = wid; le.r0 = r0; le.r1 = r1; le.next_wid = wid + 1;  // (empty windows are entries of their own: no run to fill behind)
    le.incl_row = (p.inclusive && r1 < p.n && p.ts[r1] == lim && lim > win_start) ? 1 : 0;
    le.dead = (p.pre_rows && wid == 0 && !((r1 > 0 && p.ts[r1 - 1] >= p.s0) || le.incl_row)) ? 1 : 0;
    entries[k] = le;
    nchunks[k] = (int32_t)((r1 - r0 + kChunkRows - 1) / kChunkRows);
}

// status[0] |= 1 when the interval column is not ascending (the tile kernels check this on their way; the long-only pipeline
// has no tile kernel)
__global__ __launch_bounds__(256) void ts_sorted_kernel(const int64_t *__restrict__ ts, int64_t n, uint32_t *status) {
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < n; i += stride) {
        const int64_t a = ts[i], b = i + 1 < n ? ts[i + 1] : a, l = i > 0 ? ts[i - 1] : a;
        bad |= l > a || a > b;
    }
    if (bad) atomicOr(&status[0], 1u);
}

// bowgpu_options.strict_order for the windows no tile holds: one LANE per window walks its rows in the reference's order - every
// reducer through the same running state the reference keeps (sum.go:16-22, minmax.go:16-28, integral.go:14-31, :46-62), so Sum /
// Mean / Integral* / WeightedAverage* come out bit for bit - and writes its outputs and the empty windows behind it.  Neighbouring
// lanes read neighbouring windows: a load touches 64 cache lines, but the next fifteen rows of each lane come out of the same lines
// (L1 / L2), so the rows are still fetched from HBM once.  Four rows of a lane are loaded before the first is consumed.  Windows
// longer than kStrictMaxRows are not walked (status[7]: the call is declined) - a single lane would take milliseconds per window.
constexpr int64_t kStrictMaxRows = 1ll << 20;
// one lane, one window: the walk in row order, the window's outputs, the empty windows behind it (fill_gaps)
// check_order (the long-only strict form, when some column pass reads the timestamps anyway): the walk of the first such pass also checks
// that the window's rows ascend - its own rows pair by pair and its first row against the row in front of it - and that the windows'
// row ranges are what bisection gives on an ascending column (r0 <= r1, the first window starts at row 0, the last one ends at row n):
// together, every adjacent pair of rows of the frame.  That replaces ts_sorted_kernel's pass over the whole interval column (0.16 ms per
// 1e8 rows in front of a 0.47 ms walk).
__device__ __forceinline__ void walk_entry(const AggParams &p, const LongEntry &le, const int fill_gaps, const int check_order = 0) {
    const int64_t gap = fill_gaps ? (int64_t)(le.next_wid - le.wid) - 1 : 0;
    bool order_pending = check_order != 0, bad = false;
    if (check_order) {
        bad = le.r1 < le.r0 || (le.wid == (uint64_t)p.wid_base && le.r0 != 0) || (le.wid == (uint64_t)(p.wid_base + p.W - 1) && le.r1 != p.n);
    }
    for (int slot = -1; slot < p.ncols; slot++) {
        if (p.pass_mask[slot + 1] == 0) continue;
        Stats st;
        stats_init(st);
        bool need_ts = false;
        if (slot >= 0 && slot_needs(p, slot, &need_ts) && !le.dead) {
            const ColDesc &cd = p.cols[slot];
            const uint64_t *vp = reinterpret_cast<const uint64_t *>(cd.values);
            const uint64_t *tp = reinterpret_cast<const uint64_t *>(p.ts);
            const bool chk = order_pending && need_ts && !bad;
            if (chk) order_pending = false;
            int64_t last_t = (chk && le.r0 > 0) ? p.ts[le.r0 - 1] : INT64_MIN;
            auto one = [&](bool ok, uint64_t raw, uint64_t traw) {
                if (chk) { bad = bad || (int64_t)traw < last_t; last_t = (int64_t)traw; }
                if (!ok) return;
                const double x = bits_to_f64(raw, cd.type);
                stats_value<false>(st, x, raw);
                if (need_ts) stats_point(st, (double)(int64_t)traw, x);
            };
            // eight rows of the lane are loaded (values, timestamps when an integral wants them, the validity bits as one or two words)
            // before the first is consumed: the chain of additions is the only thing that has to wait
            int64_t r = le.r0;
            // 16-byte loads from an even row on (a lane's eight rows are one 64-byte line of each column: four load instructions per
            // column instead of eight - neighbouring lanes read lines far apart, so what a load instruction costs is its count of lines:
            // 1000-row windows, WeightedAverageStep, 0.706 -> 0.602 ms per 1e8 rows.  A second batch of eight rows in flight behind the
            // first - tried in round 6 - made it 0.652.  Also tried and not kept: the wavefront fetching its 64 windows' lines TOGETHER - four
            // neighbouring lanes per line, every line asked for once, 16 lines per load instruction - and handing each window's lane its
            // eight rows through LDS: every test green, 0.470 -> 0.757 ms for the same call, Mean 0.43 -> 0.61 (the load, the LDS round trip
            // and the chain of additions then run strictly one after the other in a kernel that has one or two wavefronts per SIMD))
            const bool vec = ((reinterpret_cast<uintptr_t>(vp) | (need_ts ? reinterpret_cast<uintptr_t>(tp) : 0)) & 15) == 0;
            if (vec && (r & 1) && r < le.r1) { one(col_valid(cd, r), vp[r], need_ts ? tp[r] : 0ull); r++; }
            for (; r + 8 <= le.r1; r += 8) {
                uint64_t q[8], t[8];
                if (vec) {
#pragma unroll
                    for (int i = 0; i < 4; i++) { const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(vp + r + 2 * i); q[2 * i] = x.x; q[2 * i + 1] = x.y; }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) q[i] = vp[r + i];
                }
                if (need_ts && vec) {
#pragma unroll
                    for (int i = 0; i < 4; i++) { const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(tp + r + 2 * i); t[2 * i] = x.x; t[2 * i + 1] = x.y; }
                } else if (need_ts) {
#pragma unroll
                    for (int i = 0; i < 8; i++) t[i] = tp[r + i];
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) t[i] = 0;
                }
                uint32_t bits = 0xFFu;
                if (cd.vbits) {
                    const int64_t bit = cd.vbit0 + r;
                    const uint32_t lo = cd.vbits[bit >> 5];
                    const int sh = (int)(bit & 31);
                    bits = lo >> sh;
                    if (sh > 24) bits |= cd.vbits[(bit >> 5) + 1] << (32 - sh);
                }
#pragma unroll
                for (int i = 0; i < 8; i++) one((bits >> i) & 1u, q[i], t[i]);
            }
            for (; r < le.r1; r++) one(col_valid(cd, r), vp[r], need_ts ? tp[r] : 0ull);
        }
        emit_stats(p, slot, le, st, nullptr);
        if (gap > 0) emit_empties(p, slot, le, gap, 1, 1);
    }
    if (check_order && (bad || order_pending)) {   // (order_pending: no pass of this window read the timestamps - the host only asks when one does)
        if (!__hip_atomic_load(&p.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&p.status[0], 1u);
    }
}

__global__ __launch_bounds__(256) void long_strict_kernel(const AggParams p, const int64_t n_long, const LongEntry *entries, const int fill_gaps, const int check_order) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_long) return;
    const LongEntry le = entries[e];
    if (le.r1 - le.r0 > kStrictMaxRows) {
        if (!__hip_atomic_load(&p.status[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&p.status[7], 1u);
        return;
    }
    walk_entry(p, le, fill_gaps, check_order);
}

// The queued windows of a tile pass served WITHOUT the host in between (reference rolling/aggregation.go:190-238 is one loop): launched
// behind the tile kernel with a grid sized from the queue's CAPACITY; how many windows were queued is read here, from the sub-lists'
// counters in the status block.  One lane per queued window: its end row (galloping from its first row - these windows are a few
// hundred rows long, not the log2(n) probes of a bisection over the frame), then by its LENGTH either the walk in row order right
// here (exact, like long_strict_kernel: up to walk_max_rows rows) or an entry of the compact list `big` for the chunked order-free
// machinery, which the host runs only when status[kQueueBigWord] comes back non-zero.  strict != 0: nothing goes to the list - a window
// beyond walk_max_rows raises status[7] (the call is declined).
__global__ __launch_bounds__(256) void long_queue_kernel(const AggParams p, LongEntry *big, int32_t *big_nchunks, const int64_t walk_max_rows,
                                                         const int strict) {
    __shared__ int64_t s_start[kLongLists + 1];
    if (threadIdx.x < 64) {   // prefix sums of the 64 sub-list counters (every workgroup: 64 loads, one wave scan)
        const uint32_t cnt = p.status[kLongCountWord + threadIdx.x];
        uint32_t incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if ((int)threadIdx.x >= o) incl += up;
        }
        s_start[threadIdx.x + 1] = (int64_t)incl;
        if (threadIdx.x == 0) s_start[0] = 0;
    }
    __syncthreads();
    const int64_t n_long = s_start[kLongLists];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_long) return;
    int sub = 0;
    while (s_start[sub + 1] <= e) sub++;
    const int64_t *item = p.long_list + 2 * (sub * p.long_cap + (e - s_start[sub]));
    LongEntry le;
    le.wid = (uint64_t)item[0];
    le.r0 = item[1];
    const int64_t win_start = p.s0 + (int64_t)(le.wid * (uint64_t)p.interval);
    const int64_t lim = win_start + p.interval;
    int64_t r1 = p.n;
    if (lim >= win_start) {   // (else int64 overflow: no row can reach the window's end)
        // gallop: the first probe at the look-ahead the window outgrew, doubling until a row beyond the window is found
        int64_t lo = le.r0 + 1, step = 128, hi = p.n;
        for (;;) {
            const int64_t probe = le.r0 + step;
            if (probe >= p.n) break;
            if (p.ts[probe] >= lim) { hi = probe; break; }
            lo = probe + 1;
            step <<= 1;
        }
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (p.ts[mid] >= lim) hi = mid; else lo = mid + 1;
        }
        r1 = lo;
    }
    le.r1 = r1;
    entry_close(p, le);
    if (le.r1 - le.r0 <= walk_max_rows) {
        walk_entry(p, le, 1);
    } else if (strict) {
        if (!__hip_atomic_load(&p.status[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&p.status[7], 1u);
    } else {
        const uint32_t at = atomicAdd(&p.status[kQueueBigWord], 1u);
        big[at] = le;
        big_nchunks[at] = (int32_t)((le.r1 - le.r0 + kChunkRows - 1) / kChunkRows);
    }
}

// chunk -> window map: work_entry[w] = e for the chunks [offsets[e], offsets[e+1]) of queued window e
__global__ __launch_bounds__(256) void long_map_kernel(const int64_t n_long, const int64_t *offsets, int32_t *work_entry) {
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per window
    if (e >= n_long) return;
    for (int64_t w = offsets[e] + (threadIdx.x & 63); w < offsets[e + 1]; w += 64) work_entry[w] = (int32_t)e;
}

// one workgroup per chunk of one long window; partials[(work * ncols) + slot]
// one WAVEFRONT per chunk of one window (four independent wavefronts per workgroup, no barrier): lanes stride the chunk's rows,
// four rows per lane in flight per trip; partials[(work * ncols) + slot]
__global__ __launch_bounds__(256) void long_partial_kernel(const AggParams p, const int64_t n_long, const LongEntry *entries,
                                                           const int64_t *offsets /* n_long + 1 */, const int32_t *work_entry,
                                                           Part *partials) {
    const int lane = threadIdx.x & 63;
    const int64_t work = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (work >= offsets[n_long]) return;
    const int64_t s_e = work_entry[work];
    const LongEntry le = entries[s_e];
    const int64_t c0 = le.r0 + (work - offsets[s_e]) * kChunkRows;
    const int64_t c1 = (c0 + kChunkRows < le.r1) ? c0 + kChunkRows : le.r1;

    for (int slot = 0; slot < p.ncols; slot++) {
        bool need_ts;
        const bool need_vals = slot_needs(p, slot, &need_ts);
        Part acc;
        part_init(acc);
        if (need_vals && !le.dead) {
            const ColDesc &cd = p.cols[slot];
            const uint64_t *vp = reinterpret_cast<const uint64_t *>(cd.values);
            auto one = [&](int64_t r, uint64_t raw) {
                const double x = bits_to_f64(raw, cd.type);
                acc.sum += x;
                acc.count++;
                if (acc.first_idx < 0) acc.first_idx = r;
                acc.last_idx = r;
                if (x == x) {
                    if (acc.min_idx < 0 || x < acc.vmin) { acc.vmin = x; acc.min_idx = r; }
                    if (acc.max_idx < 0 || x > acc.vmax) { acc.vmax = x; acc.max_idx = r; }
                }
                if (need_ts) {  // the term of the pair (this point, next both-valid point inside the window)
                    const int64_t rn = col_next_valid(cd, r + 1, le.r1);
                    if (rn >= 0) {
                        const double t0 = (double)p.ts[r], t1 = (double)p.ts[rn];
                        const double x1 = bits_to_f64(vp[rn], cd.type);
                        acc.trap += (x + x1) / 2 * (t1 - t0);   // integral.go:24
                        acc.step += x * (t1 - t0);              // integral.go:55
                    }
                }
            };
            int64_t r = c0 + lane;
            for (; r + 192 < c1; r += 256) {  // four independent loads per lane before any of them is consumed
                const uint64_t q0 = vp[r], q1 = vp[r + 64], q2 = vp[r + 128], q3 = vp[r + 192];
                if (col_valid(cd, r)) one(r, q0);
                if (col_valid(cd, r + 64)) one(r + 64, q1);
                if (col_valid(cd, r + 128)) one(r + 128, q2);
                if (col_valid(cd, r + 192)) one(r + 192, q3);
            }
            for (; r < c1; r += 64)
                if (col_valid(cd, r)) one(r, vp[r]);
        }
        for (int o = 32; o > 0; o >>= 1) {  // wavefront reduction in a fixed shape
            Part other;
            other.sum = __shfl_down(acc.sum, o); other.trap = __shfl_down(acc.trap, o); other.step = __shfl_down(acc.step, o);
            other.vmin = __shfl_down(acc.vmin, o); other.vmax = __shfl_down(acc.vmax, o);
            other.count = __shfl_down((long long)acc.count, o);
            other.min_idx = __shfl_down((long long)acc.min_idx, o); other.max_idx = __shfl_down((long long)acc.max_idx, o);
            other.first_idx = __shfl_down((long long)acc.first_idx, o); other.last_idx = __shfl_down((long long)acc.last_idx, o);
            if (lane + o < 64) part_merge(acc, other);
        }
        if (lane == 0) partials[work * p.ncols + slot] = acc;
    }
}

// One LANE per long window: the usual long window has a handful of chunk partials and no run of empty windows behind it, and
// finishing it (rebuild the reference's running state from the order-free partial, evaluate the reducers, write the slot) is
// work for one lane - 64 windows per wavefront instead of one workgroup each.  Windows with more partials or a longer run of
// empty windows are left to long_final_block_kernel (lane_finishes is the split).
constexpr int kLaneParts = 8, kLaneGap = 8;
__device__ __forceinline__ bool lane_finishes(const LongEntry &le, int64_t nparts) {
    return nparts <= kLaneParts && (int64_t)(le.next_wid - le.wid) - 1 <= kLaneGap;
}

__global__ __launch_bounds__(256) void long_final_kernel(const AggParams p, const int64_t n_long, const LongEntry *entries,
                                                         const int64_t *offsets, const Part *partials, int32_t *leftover,
                                                         unsigned long long *n_leftover) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool have = e < n_long;
    LongEntry le;
    le.wid = 0; le.r0 = 0; le.r1 = 0; le.next_wid = 1; le.incl_row = 0; le.dead = 1;
    int64_t w0 = 0, w1 = 0;
    if (have) { le = entries[e]; w0 = offsets[e]; w1 = offsets[e + 1]; }
    const int64_t my_gap = have ? (int64_t)(le.next_wid - le.wid) - 1 : 0;
    const bool simple = have && lane_finishes(le, w1 - w0);
    if (have && !simple) leftover[atomicAdd(n_leftover, 1ull)] = (int32_t)e;  // (rare) for long_final_block_kernel
    (void)lane;

    for (int slot = -1; slot < p.ncols; slot++) {
        const unsigned my_mask = p.pass_mask[slot + 1];
        if (my_mask == 0) continue;
        const bool need_vals = slot >= 0 && (p.pass_flags[slot + 1] & kPassNeedVals);

        if (simple) {
            Part acc;
            part_init(acc);
            if (need_vals)
                for (int64_t w = w0; w < w1; w++) part_merge(acc, partials[w * p.ncols + slot]);  // (at most kLaneParts, in order)
            emit_window(p, slot, le, acc);
            emit_empties(p, slot, le, my_gap, 1, 1);
        }
    }
}

// The windows the lane-per-window kernels leave (many chunk partials, or a long run of empty windows behind them): one workgroup
// per window merges its chunk partials in a fixed shape, writes the outputs, then the empty windows that follow it.
// leftover: indices into entries / off0 / off1 (nullptr: the lists are compact, entry i).  stream_chunks > 0: the entries come
// from stream_final_kernel - windows that ran past its look-ahead; their end is found here by bisection, their partials are
// [off0, 2 * (chunk of the end) + 1) of the chunk grid, and the empty windows are not theirs to write.
__global__ __launch_bounds__(256) void long_final_block_kernel(const AggParams p, const LongEntry *entries, const int64_t *off0,
                                                               const int64_t *off1, const Part *partials, const int32_t *leftover,
                                                               const unsigned long long *n_leftover, const int64_t stream_chunks, const int lite) {
    __shared__ Part red[4];
    __shared__ LongEntry s_le;
    __shared__ int64_t s_w1;
    const int64_t nleft = (int64_t)*n_leftover;  // (usually 0: the launch then costs a few microseconds)
    for (int64_t i = blockIdx.x; i < nleft; i += gridDim.x) {
        const int64_t e = leftover ? leftover[i] : i;
        const int lane = threadIdx.x;
        if (lane == 0) {
            LongEntry le = entries[e];
            int64_t w1 = off1[e];
            if (stream_chunks > 0) {
                le.r1 = window_end_row(p, le.wid, le.r0 + 1);
                entry_close(p, le);
                le.next_wid = le.wid + 1;
                w1 = 2 * (le.r1 / kStreamRows) + 1;
                if (w1 > 2 * stream_chunks) w1 = 2 * stream_chunks;
            }
            s_le = le;
            s_w1 = w1;
        }
        __syncthreads();
        const LongEntry le = s_le;
        const int64_t w0 = off0[e], w1 = s_w1;
        const int64_t gap = (int64_t)(le.next_wid - le.wid) - 1;
        for (int slot = -1; slot < p.ncols; slot++) {
            if (p.pass_mask[slot + 1] == 0) continue;
            Part acc;
            part_init(acc);
            if (slot >= 0 && (p.pass_flags[slot + 1] & kPassNeedVals)) {
                if (w1 - w0 == 1) {  // the common medium-sized window: nothing to merge
                    if (lane == 0) acc = part_at(partials, w0 * p.ncols + slot, lite);
                } else {
                    for (int64_t w = w0 + lane; w < w1; w += 256) part_merge(acc, part_at(partials, w * p.ncols + slot, lite));
                    block_reduce(acc, red, lane);
                    __syncthreads();
                }
            }
            if (lane == 0) emit_window(p, slot, le, acc);
            emit_empties(p, slot, le, gap, 1 + lane, 256);
        }
        __syncthreads();  // (red[], s_le are reused by the next entry)
    }
}

// stream_final_kernel belongs to the streaming form (long_stream.hip) and is compiled HERE, next to long_final_block_kernel, which
// takes over its longest windows: in long_stream.hip's translation unit the compiler emits other instructions for it (the word index
// of the deferred bitmap stores), and the split of the two forms changes no kernel (profiles/wave_ops_kernel_identity.txt).
// One lane per window of the call: the empty ones (no record), the ones inside one chunk (their partial is ready), and the ones
// over a few chunks (walk the heads that follow the chunk they start in, merge the range of partials).  Windows that run
// further than kStreamScan chunks are queued for long_final_block_kernel: entries / off0 / off1 [i], i < *n_leftover.
__global__ __launch_bounds__(256) void stream_final_kernel(const AggParams p, const int64_t nchunks, const ChunkMeta *meta,
                                                           const Part *parts, const WinRec *recs, const Part *wparts,
                                                           LongEntry *entries, int64_t *off0, int64_t *off1,
                                                           unsigned long long *n_leftover, const int lite) {
    // A lane's life here is a chain of dependent loads (record -> partials -> the first / last value of the window): what can be
    // loaded early is (the next two records with the lane's own; up to four partials at once), and the validity bits do not go
    // through atomics - lane k is window k, so the ballots of a wavefront ARE two words of every output's bitmap.
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = k < p.W;
    const bool defer_bits = !p.bits_preset;      // (bitmaps preset to all-null: whole words can be stored)
    uint32_t vbits = 0;                          // bit i: the output of aggregation i is valid for this lane's window
    if (in) {
        const WinRec rec = recs[k];
        const int64_t rn1 = k + 1 < p.W ? recs[k + 1].r0 : p.n, rn2 = k + 2 < p.W ? recs[k + 2].r0 : p.n;   // (behind the last window: the end of the rows)
        LongEntry le;
        le.wid = (uint64_t)(p.wid_base + k); le.r0 = rec.r0; le.r1 = -1; le.next_wid = le.wid + 1; le.incl_row = 0; le.dead = 0;
        bool done = false;
        if (rec.r0 < 0) {   // no rows: the reducers' values for an empty window (window k itself: "0 windows behind it")
            for (int slot = -1; slot < p.ncols; slot++)
                if (p.pass_mask[slot + 1]) emit_empties(p, slot, le, 0, 0, 1);
            done = true;
        }
        const int64_t g = rec.chunk;
        int64_t w0 = 2 * g + 1, w1 = w0;
        if (!done) {
            if (rec.rows >= 0) le.r1 = rec.r0 + rec.rows;
            else {
                // the window ends where the next window that has rows starts (rows are ascending, the windows partition them) ...
                if (rn1 >= 0) le.r1 = rn1;
                else if (rn2 >= 0) le.r1 = rn2;
                else
                    for (int64_t kk = k + 3; kk <= k + 8; kk++) {
                        if (kk >= p.W) { le.r1 = p.n; break; }
                        const int64_t rs = recs[kk].r0;
                        if (rs >= 0) { le.r1 = rs; break; }
                    }
                if (le.r1 >= 0) w1 = 2 * ((le.r1 - 1) / kStreamRows) + 1;    // (its last row's chunk: the head partial of that chunk is its last partial)
                // ... or, behind a run of empty windows, where the first chunk head ends that does not cover its chunk
                else for (int64_t c = g + 1; c <= g + kStreamScan; c++) {
                    if (c >= nchunks) { le.r1 = p.n; w1 = 2 * nchunks; break; }
                    const int64_t rows_c = p.n - c * kStreamRows < kStreamRows ? p.n - c * kStreamRows : kStreamRows;
                    const int64_t hr = meta[c].head_rows;
                    if (hr < rows_c) { le.r1 = c * kStreamRows + hr; w1 = 2 * c + 1; break; }
                }
                if (le.r1 < 0) {       // (long_final_block_kernel finishes it, validity bits included: this lane's stay 0 here)
                    const unsigned long long i = atomicAdd(n_leftover, 1ull);
                    entries[i] = le;
                    off0[i] = w0;
                    off1[i] = w1;
                    done = true;
                }
            }
        }
        if (!done) {
            if (p.inclusive || p.pre_rows) entry_close(p, le);   // (the row behind the window / rows below s0 matter only then)
            for (int slot = -1; slot < p.ncols; slot++) {
                if (p.pass_mask[slot + 1] == 0) continue;
                Part acc;
                part_init(acc);
                if (slot >= 0 && (p.pass_flags[slot + 1] & kPassNeedVals)) {
                    if (rec.rows >= 0) acc = part_at(wparts, k * p.ncols + slot, lite);
                    else {
                        // four partials at a time (a 1000-row window has three to five): their loads go out together
                        for (int64_t w = w0; w < w1; w += 4) {
                            const int64_t wl = w1 - 1;
                            const Part q0 = part_at(parts, w * p.ncols + slot, lite), q1 = part_at(parts, (w + 1 < wl ? w + 1 : wl) * p.ncols + slot, lite),
                                       q2 = part_at(parts, (w + 2 < wl ? w + 2 : wl) * p.ncols + slot, lite), q3 = part_at(parts, (w + 3 < wl ? w + 3 : wl) * p.ncols + slot, lite);
                            part_merge(acc, q0);
                            if (w + 1 < w1) part_merge(acc, q1);
                            if (w + 2 < w1) part_merge(acc, q2);
                            if (w + 3 < w1) part_merge(acc, q3);
                        }
                    }
                }
                emit_window(p, slot, le, acc, defer_bits ? &vbits : nullptr);
            }
        }
    }
    if (defer_bits) {
        // (every lane of the wavefront arrives here: windows 64 w .. 64 w + 63 = bitmap words 2 w, 2 w + 1 of every output)
        const int64_t k0 = k - lane;
        for (int a = 0; a < p.naggs; a++) {
            uint32_t *bits = p.aggs[a].out_valid;
            const uint64_t m = __ballot((vbits >> a) & 1u);
            if (!bits) continue;
            if (lane == 0 && k0 < p.W) bits[k0 >> 5] = (uint32_t)m;
            if (lane == 32 && k0 + 32 < p.W) bits[(k0 + 32) >> 5] = (uint32_t)(m >> 32);
        }
    }
}

size_t long_entry_size() { return sizeof(LongEntry); }
size_t long_part_size() { return sizeof(Part); }

// The last two launches of the streaming form (long_stream.hip launch_long_stream, windows that average less than 8 chunks): a lane per
// window, then long_final_block_kernel for the windows that run past a lane's look-ahead.  meta / recs / parts / wparts / entries: the
// ChunkMeta / WinRec / Part / LongEntry arrays of long_stream_workspace.
int launch_stream_final(Ctx *c, const AggParams &p, int64_t nchunks, const void *meta, const void *parts, const void *recs, const void *wparts,
                        void *entries, int64_t *off0, int64_t *off1, unsigned long long *n_leftover, int lite) {
    LongEntry *le = reinterpret_cast<LongEntry *>(entries);
    const Part *pt = reinterpret_cast<const Part *>(parts);
    hipLaunchKernelGGL(stream_final_kernel, dim3((unsigned)((p.W + 255) / 256)), dim3(256), 0, c->stream, p, nchunks,
                       reinterpret_cast<const ChunkMeta *>(meta), pt, reinterpret_cast<const WinRec *>(recs), reinterpret_cast<const Part *>(wparts),
                       le, off0, off1, n_leftover, lite);
    hipLaunchKernelGGL(long_final_block_kernel, dim3((unsigned)(nchunks < 2048 ? nchunks : 2048)), dim3(256), 0, c->stream, p, le, off0, off1,
                       pt, (const int32_t *)nullptr, n_leftover, nchunks, lite);
    BG_HIP(hipGetLastError());
    return 0;
}

// starts == nullptr: every window of the call is an entry (long-only pipeline), preceded by the order check of the interval column
int launch_long_queue(Ctx *c, const AggParams &p, int64_t capacity, void *big_entries, int32_t *big_nchunks, int64_t walk_max_rows, bool strict) {
    if (capacity <= 0) return 0;
    hipLaunchKernelGGL(long_queue_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, c->stream, p,
                       reinterpret_cast<LongEntry *>(big_entries), big_nchunks, walk_max_rows, strict ? 1 : 0);
    BG_HIP(hipGetLastError());
    return 0;
}

// n_given > 0: entries / nchunks [0, n_given) are already there (long_queue_kernel's compact list of the windows it did not walk)
int launch_long_windows_v2(Ctx *c, const AggParams &p, const LongListStarts *starts, void *entries, int32_t *nchunks,
                           int64_t *offsets, int64_t *block_sums, int64_t *d_total, int32_t *work_entry, void *partials,
                           int64_t max_work, bool strict, int64_t n_given) {
    const int64_t n_long = n_given > 0 ? n_given : starts ? starts->start[kLongLists] : p.W;
    if (n_long <= 0) return 0;
    bool walk_checks = false;
    if (n_given > 0) {
    } else if (starts) {
        hipLaunchKernelGGL(long_bounds_kernel, dim3((unsigned)((n_long + 255) / 256)), dim3(256), 0, c->stream, p, *starts,
                           reinterpret_cast<LongEntry *>(entries), nchunks);
    } else {
        // the order check of the interval column: its own pass - or, under strict_order when some column pass walks the timestamps anyway and
        // no row lies below s0 (no window is skipped as dead), the walks themselves (walk_entry check_order)
        for (int sl = 0; sl < p.ncols; sl++) walk_checks = walk_checks || (p.pass_mask[sl + 1] && p.cols[sl].need_ts);
        walk_checks = walk_checks && strict && !p.pre_rows;
        if (!walk_checks) {
            int64_t g = (p.n / 2 + 255) / 256;
            if (g > 256 * 32) g = 256 * 32;
            if (g < 1) g = 1;
            hipLaunchKernelGGL(ts_sorted_kernel, dim3((unsigned)g), dim3(256), 0, c->stream, p.ts, p.n, p.status);
        }
        hipLaunchKernelGGL(long_bounds_all_kernel, dim3((unsigned)((n_long + 255) / 256)), dim3(256), 0, c->stream, p,
                           reinterpret_cast<LongEntry *>(entries), nchunks);
    }
    if (strict) {   // every window in row order, one lane each (queued windows: + the empty windows behind them)
        hipLaunchKernelGGL(long_strict_kernel, dim3((unsigned)((n_long + 255) / 256)), dim3(256), 0, c->stream, p, n_long,
                           reinterpret_cast<const LongEntry *>(entries), starts ? 1 : 0, walk_checks ? 1 : 0);
        BG_HIP(hipGetLastError());
        return 0;
    }
    BG_TRY(launch_exclusive_scan(c, nchunks, n_long, offsets, block_sums, d_total));
    hipLaunchKernelGGL(long_map_kernel, dim3((unsigned)((n_long + 3) / 4)), dim3(256), 0, c->stream, n_long, offsets, work_entry);
    hipLaunchKernelGGL(long_partial_kernel, dim3((unsigned)((max_work + 3) / 4)), dim3(256), 0, c->stream, p, n_long,
                       reinterpret_cast<const LongEntry *>(entries), offsets, work_entry, reinterpret_cast<Part *>(partials));
    // the chunk -> window map has served long_partial_kernel: its buffer now lists the windows left to the workgroup kernel
    unsigned long long *n_leftover = reinterpret_cast<unsigned long long *>(d_total);
    BG_HIP(hipMemsetAsync(n_leftover, 0, 8, c->stream));
    hipLaunchKernelGGL(long_final_kernel, dim3((unsigned)((n_long + 255) / 256)), dim3(256), 0, c->stream, p, n_long,
                       reinterpret_cast<const LongEntry *>(entries), offsets, reinterpret_cast<const Part *>(partials), work_entry, n_leftover);
    hipLaunchKernelGGL(long_final_block_kernel, dim3((unsigned)(n_long < 2048 ? n_long : 2048)), dim3(256), 0, c->stream, p,
                       reinterpret_cast<const LongEntry *>(entries), offsets, offsets + 1, reinterpret_cast<const Part *>(partials),
                       (const int32_t *)work_entry, n_leftover, (int64_t)0, 0);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
