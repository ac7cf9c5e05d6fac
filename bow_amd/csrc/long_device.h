// long_device.h — what the two forms of the long-window reducers share (long_windows.hip: the entry-list form; long_stream.hip: the
// streaming form): the LongEntry / Part vocabulary, the validity and chunk helpers, and the emit helpers that turn an order-free
// partial into a window's outputs.
#pragma once

#include <type_traits>
#include "agg_device.h"
#include "bitmap_device.h"

namespace bowgpu {

// (an unnamed namespace in a header, on purpose: these types are arguments of the kernels of both translation units, whose symbols -
// what the profiles and scratch/kernel_diff.py know them by - spell it; everything here is inlined into those kernels)
namespace {

constexpr int kChunkRows = kLongChunkRows;
constexpr int kStreamRows = kLongStreamRows;   // the streaming form's chunk (one wavefront)

struct LongEntry {
    uint64_t wid;
    int64_t r0, r1;
    uint64_t next_wid;
    int32_t incl_row;   // the row r1 sits exactly on the window's end and windows are inclusive
    int32_t dead;       // window 0 made only of rows below s0 (an empty slice in the reference)
};

struct Part {
    double sum, trap, step;
    double vmin, vmax;
    int64_t count;
    int64_t min_idx, max_idx;     // -1: no non-NaN value
    int64_t first_idx, last_idx;  // -1: no valid value
};

__device__ __forceinline__ void part_init(Part &p) {
    p.sum = 0.0; p.trap = 0.0; p.step = 0.0; p.vmin = 0.0; p.vmax = 0.0; p.count = 0;
    p.min_idx = -1; p.max_idx = -1; p.first_idx = -1; p.last_idx = -1;
}

__device__ __forceinline__ void part_merge(Part &a, const Part &b) {
    a.sum += b.sum; a.trap += b.trap; a.step += b.step; a.count += b.count;
    if (b.min_idx >= 0 && (a.min_idx < 0 || b.vmin < a.vmin || (b.vmin == a.vmin && b.min_idx < a.min_idx))) { a.vmin = b.vmin; a.min_idx = b.min_idx; }
    if (b.max_idx >= 0 && (a.max_idx < 0 || b.vmax > a.vmax || (b.vmax == a.vmax && b.max_idx < a.max_idx))) { a.vmax = b.vmax; a.max_idx = b.max_idx; }
    if (b.first_idx >= 0 && (a.first_idx < 0 || b.first_idx < a.first_idx)) a.first_idx = b.first_idx;
    if (b.last_idx > a.last_idx) a.last_idx = b.last_idx;
}

__device__ __forceinline__ bool col_valid(const ColDesc &cd, int64_t r) {
    if (!cd.vbits) return true;
    const int64_t bit = cd.vbit0 + r;
    return (cd.vbits[bit >> 5] >> (bit & 31)) & 1u;
}

// next valid row of the column in [r, lim), or -1
__device__ __forceinline__ int64_t col_next_valid(const ColDesc &cd, int64_t r, int64_t lim) {
    if (r >= lim) return -1;
    if (!cd.vbits) return r;
    int64_t b = cd.vbit0 + r;
    const int64_t bend = cd.vbit0 + lim;
    while (b < bend) {
        const int64_t w = b >> 5;
        const uint32_t x = cd.vbits[w] & (~0u << (b & 31));
        if (x) {
            const int64_t rr = (w << 5) + (__ffs((int)x) - 1) - cd.vbit0;
            return rr < lim ? rr : -1;
        }
        b = (w + 1) << 5;
    }
    return -1;
}

__device__ __forceinline__ bool slot_needs(const AggParams &p, int slot, bool *need_ts) {
    const unsigned m = p.pass_mask[slot + 1];
    *need_ts = false;
    for (unsigned mm = m; mm; mm &= mm - 1) {
        const int k = p.aggs[__ffs(mm) - 1].kind;
        if (k >= BOWGPU_AGG_INTEGRAL_STEP && k <= BOWGPU_AGG_WAVG_LINEAR) *need_ts = true;
    }
    return (p.pass_flags[slot + 1] & kPassNeedVals) != 0;
}

// workgroup (256 threads) reduction in a fixed shape: lanes by shuffle, then the four waves in order; result in thread 0
__device__ __forceinline__ void block_reduce(Part &acc, Part *red /* [4], LDS */, int tid) {
    for (int o = 32; o > 0; o >>= 1) {
        Part other;
        other.sum = __shfl_down(acc.sum, o); other.trap = __shfl_down(acc.trap, o); other.step = __shfl_down(acc.step, o);
        other.vmin = __shfl_down(acc.vmin, o); other.vmax = __shfl_down(acc.vmax, o);
        other.count = __shfl_down((long long)acc.count, o);
        other.min_idx = __shfl_down((long long)acc.min_idx, o); other.max_idx = __shfl_down((long long)acc.max_idx, o);
        other.first_idx = __shfl_down((long long)acc.first_idx, o); other.last_idx = __shfl_down((long long)acc.last_idx, o);
        if ((tid & 63) + o < 64) part_merge(acc, other);
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        acc = red[0];
        part_merge(acc, red[1]); part_merge(acc, red[2]); part_merge(acc, red[3]);
    }
}

// partial `i` of an array of Part, or - lite - of {sum, count} pairs (what Sum / Mean / Count need: the streaming form's
// storage when no reducer of the call wants more)
struct PartLite { double sum; int64_t count; };
__device__ __forceinline__ Part part_at(const Part *base, int64_t i, int lite) {
    if (!lite) return base[i];
    const PartLite l = reinterpret_cast<const PartLite *>(base)[i];
    Part q;
    part_init(q);
    q.sum = l.sum; q.count = l.count;
    return q;
}

// window id of a row's timestamp (rows below s0 ride in window 0: SURVEY A.5)
__device__ __forceinline__ uint64_t row_wid(const AggParams &p, int64_t t) {
    return (p.pre_rows && t < p.s0) ? 0ull : magic_div((uint64_t)t - (uint64_t)p.s0, p.magic);
}

// wid, r0 and r1 known: what follows the window (rolling.go:197-209) - the next non-empty window, whether the row at r1 sits
// exactly on the window's end (an inclusive window takes it), whether window 0 is made of rows below s0 only
__device__ __forceinline__ void entry_close(const AggParams &p, LongEntry &le) {
    uint64_t next_wid = (uint64_t)(p.wid_base + p.W);
    bool at_start = false;
    if (le.r1 < p.n) {
        const int64_t t = p.ts[le.r1];
        next_wid = magic_div((uint64_t)t - (uint64_t)p.s0, p.magic);
        at_start = (t == p.s0 + (int64_t)(next_wid * (uint64_t)p.interval));
    }
    le.next_wid = next_wid;
    le.incl_row = (p.inclusive && le.r1 < p.n && at_start && next_wid == le.wid + 1) ? 1 : 0;
    le.dead = (p.pre_rows && le.r0 == 0 && !(p.ts[le.r1 - 1] >= p.s0 || le.incl_row)) ? 1 : 0;
}

// first row >= lo whose timestamp reaches the end of window `wid` (p.n when none), by bisection in global memory
__device__ __forceinline__ int64_t window_end_row(const AggParams &p, uint64_t wid, int64_t lo) {
    const int64_t win_start = p.s0 + (int64_t)(wid * (uint64_t)p.interval);
    const int64_t lim = win_start + p.interval;
    if (lim < win_start) return p.n;  // int64 overflow: no row can reach it
    int64_t hi = p.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (p.ts[mid] >= lim) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void emit_stats(const AggParams &p, int slot, const LongEntry &w, const Stats &st, uint32_t *valid_out);

// The outputs of one column pass (slot; -1: the reducers that need no column) for window `w`, from its merged order-free partial
// (valid_out != nullptr: the validity bitmaps are not touched; bit i of *valid_out is set when the output of aggregation i is valid -
// the caller assembles whole bitmap words from its lanes)
__device__ __forceinline__ void emit_window(const AggParams &p, int slot, const LongEntry &w, const Part &acc, uint32_t *valid_out = nullptr) {
    const ColDesc *cd = slot >= 0 ? &p.cols[slot] : nullptr;
    const int col_type = cd ? cd->type : BOWGPU_INT64;
    const uint64_t *vp = cd ? reinterpret_cast<const uint64_t *>(cd->values) : nullptr;
    const int64_t oslot = (int64_t)(w.wid - (uint64_t)p.wid_base);
    if ((uint64_t)oslot >= (uint64_t)p.W) return;
    // rebuild the reference's running state from the order-free partial
    // (window 0 made only of rows below s0 is an empty slice in the reference, rolling.go:194-228: the streaming form merges its chunks'
    // partials before it knows - entry_close - so they are left out here)
    Stats st;
    stats_init(st);
    if (!w.dead) { st.sum = acc.sum; st.count = acc.count; st.has_value = acc.first_idx >= 0; }
    if (st.has_value) {
        st.first_bits = vp[acc.first_idx]; st.last_bits = vp[acc.last_idx];
        const double f = bits_to_f64(st.first_bits, col_type);
        // minmax.go:16-28: seeded by the first valid value; a NaN seed is never replaced
        st.vmin = (f != f) ? f : (acc.min_idx >= 0 ? acc.vmin : f);
        st.vmax = (f != f) ? f : (acc.max_idx >= 0 ? acc.vmax : f);
        st.has_point = 1; st.pt = (double)p.ts[acc.last_idx]; st.pv = bits_to_f64(st.last_bits, col_type);
        st.integ_trap = acc.trap; st.integ_step = acc.step; st.has_pair = acc.count >= 2;
    }
    emit_stats(p, slot, w, st, valid_out);
}

// ... from the reference's running state itself (emit_window rebuilds it from an order-free partial; long_strict_kernel arrives
// with the state of a walk in row order)
__device__ __forceinline__ void emit_stats(const AggParams &p, int slot, const LongEntry &w, const Stats &st, uint32_t *valid_out) {
    const unsigned my_mask = p.pass_mask[slot + 1];
    const ColDesc *cd = slot >= 0 ? &p.cols[slot] : nullptr;
    const int col_type = cd ? cd->type : BOWGPU_INT64;
    const bool need_vals = cd && (p.pass_flags[slot + 1] & kPassNeedVals);
    const uint64_t *vp = cd ? reinterpret_cast<const uint64_t *>(cd->values) : nullptr;
    const int64_t win_start = p.s0 + (int64_t)(w.wid * (uint64_t)p.interval);
    const int64_t oslot = (int64_t)(w.wid - (uint64_t)p.wid_base);
    const int64_t len = w.dead ? 0 : w.r1 - w.r0;
    if ((uint64_t)oslot >= (uint64_t)p.W) return;
    // the state including the inclusive row, for the reducers that want it (aggregation.go:207-211)
    Stats st_incl = st;
    if (w.incl_row && need_vals && col_valid(*cd, w.r1)) {
        const uint64_t raw = vp[w.r1];
        const double x = bits_to_f64(raw, col_type);
        stats_value<false>(st_incl, x, raw);
        stats_point(st_incl, (double)p.ts[w.r1], x);
    }
    for (unsigned m = my_mask; m; m &= m - 1) {
        const AggDesc &a = p.aggs[__ffs(m) - 1];
        const bool inc = a.kind == BOWGPU_AGG_INTEGRAL_TRAPEZOID || a.kind == BOWGPU_AGG_WAVG_LINEAR;
        Val v = finish_val(reduce_val(a.kind, inc ? st_incl : st, inc ? len + w.incl_row : len, win_start, p.interval,
                                      col_type == BOWGPU_INT64), a);
        reinterpret_cast<uint64_t *>(a.out_values)[oslot] = v.bits;
        if (valid_out) { if (v.valid) *valid_out |= 1u << (__ffs(m) - 1); }
        else if (a.out_valid) {
            if (v.valid) atomicOr(&a.out_valid[oslot >> 5], 1u << (oslot & 31));
            else if (p.bits_preset) atomicAnd(&a.out_valid[oslot >> 5], ~(1u << (oslot & 31)));
        }
    }
}

// the empty windows gk = first, first + step, ... <= gap behind window `w`, same pass
__device__ __forceinline__ void emit_empties(const AggParams &p, int slot, const LongEntry &w, int64_t gap, int64_t first, int64_t step) {
    const unsigned my_mask = p.pass_mask[slot + 1];
    const int col_type = slot >= 0 ? p.cols[slot].type : BOWGPU_INT64;
    const int64_t win_start = p.s0 + (int64_t)(w.wid * (uint64_t)p.interval);
    const int64_t oslot = (int64_t)(w.wid - (uint64_t)p.wid_base);
    Stats em;
    stats_init(em);
    for (int64_t gk = first; gk <= gap; gk += step) {
        const int64_t gs = oslot + gk;
        if (gs < 0 || gs >= p.W) break;
        const int64_t gstart = win_start + gk * p.interval;
        for (unsigned m = my_mask; m; m &= m - 1) {
            const AggDesc &a = p.aggs[__ffs(m) - 1];
            Val v = finish_val(reduce_val(a.kind, em, 0, gstart, p.interval, col_type == BOWGPU_INT64), a);
            reinterpret_cast<uint64_t *>(a.out_values)[gs] = v.bits;
            if (p.bits_preset && a.out_valid && !v.valid) atomicAnd(&a.out_valid[gs >> 5], ~(1u << (gs & 31)));
        }
    }
}

}  // namespace

// ---- the streaming form's records (long_stream.hip writes them; stream_final_kernel, compiled in long_windows.hip, reads them)
struct ChunkMeta {
    int32_t head_rows;    // leading rows that belong to the window of the row before the chunk (the whole chunk: it runs through)
};
struct WinRec {
    int64_t r0;           // first row of the window; < 0: the window has no rows
    int32_t rows;         // its rows when it lies inside one chunk; -1: it runs on into the chunks after `chunk`
    int32_t chunk;
};

constexpr int kStreamScan = 64;   // chunks a lane of stream_final_kernel looks ahead for the end of its window

}  // namespace bowgpu
