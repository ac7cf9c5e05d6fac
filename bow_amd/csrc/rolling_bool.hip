// rolling_bool.hip — Rolling.Aggregate over BOOLEAN value columns (Arrow bit-packed values + validity).
//
// On a Boolean column (ToFloat64: true = 1.0, false = 0.0, bowconvert.go) every value reducer is a function of four numbers of
// the window: nv = valid rows, nt = valid rows that are true, and the bits of the first and of the last valid row:
//   Sum  float64(nt)                 (sum.go:11-24; an empty window: 0.0)
//   ArithmeticMean  float64(nt) / float64(nv)      (arithmeticmean.go:11-29: a sum of 1.0s is exact)
//   Min  0.0 when a valid false exists, else 1.0   Max  1.0 when a valid true exists, else 0.0   (minmax.go)
//   Count  nv (count.go)             First / Last  that row's bit (firstlast.go)
//   Mode  the majority; on a tie the value the LAST valid row does not have (mode.go:18-27 keeps the value whose count first
//         reaches the maximum: at a tie the other value got there one of its rows earlier)
// all nil at nv == 0 but Sum and Count.  So one pass over the windows' bit ranges - popcount(V), popcount(T & V), lowest and highest
// set bit of V - serves every requested reducer of a column: integer arithmetic, the reference's bits at any window length.
//
// bool_windows_kernel: a wavefront takes 64 consecutive windows, one per lane (window_rows.h gives the rows, the rule Mode uses).
//   <= kBoolLaneRows rows : the lane walks its window in chunks of 32 rows (two words of each bitmap per chunk; neighbouring lanes
//                           read the same or adjoining words)
//   longer                : the wavefront takes such windows one after the other, lane j the chunks j, j + 64, ..., and combines
//                           the counts by shuffles; first / last valid row from the lowest / highest lane that saw one
// The 8-byte results of the 64 windows leave as one coalesced store per output, their validity word - and the value word of a
// Boolean output - as two 32-bit halves of a __ballot, stored whole: no atomics on outputs, no preset.  The host gives word-aligned
// working copies for every bitmap and copies ceil(W / 8) bytes on to the caller.  Nullable outputs of one column are nil in the
// same windows (nv == 0): one count per launch, summed per wavefront over its grid-stride trips, one atomic add each.
//
// bool_widen_kernel: the column as Float64 0.0 / 1.0 with its validity at bit 0, for the time-weighted reducers (they need the
// timestamps and the neighbouring points: the Float64 kernels serve them).
// No MFMA, no LDS, no scratch.
#include "agg_device.h"
#include "bitmap_device.h"
#include "window_rows.h"
#include "wave_ops.h"

namespace bowgpu {

namespace {

// len (1 .. 32) bits from bit b of an aligned word array: only words that hold one of them are read
__device__ __forceinline__ uint32_t bits32(const uint32_t *w, int64_t b, int len) {
    const int64_t wi = b >> 5;
    const int sh = (int)(b & 31);
    uint32_t x = w[wi] >> sh;
    if (sh + len > 32) x |= w[wi + 1] << (32 - sh);
    return len == 32 ? x : (x & ((1u << len) - 1u));
}

struct BoolAcc {
    int64_t nv, nt;
    int64_t first, last;   // valid rows, relative to the window's first row; -1: none
    uint32_t fbit, lbit;
};
__device__ __forceinline__ void acc_init(BoolAcc &s) { s.nv = 0; s.nt = 0; s.first = -1; s.last = -1; s.fbit = 0; s.lbit = 0; }

// rows [row, row + len) of the column, len <= 32, the window's row `rel` first; chunks arrive in ascending order
__device__ __forceinline__ void acc_chunk(const BoolParams &p, int64_t row, int len, int64_t rel, BoolAcc &s) {
    const uint32_t V = p.vbits ? bits32(p.vbits, p.vbit0 + row, len) : (len == 32 ? 0xFFFFFFFFu : ((1u << len) - 1u));
    if (!V) return;
    const uint32_t T = bits32(p.tbits, p.tbit0 + row, len) & V;
    s.nv += __popc(V);
    s.nt += __popc(T);
    const int lo = __ffs((int)V) - 1, hi = 31 - __clz((int)V);
    if (s.first < 0) { s.first = rel + lo; s.fbit = (T >> lo) & 1u; }
    s.last = rel + hi;
    s.lbit = (T >> hi) & 1u;
}

// the two halves of a wavefront's 64-window word: words[2 g], words[2 g + 1]; the second only when it holds a window
__device__ __forceinline__ void store_word64(uint32_t *words, int64_t g, int64_t W, int lane, uint64_t m) {
    if (lane == 0) words[2 * g] = (uint32_t)m;
    if (lane == 32 && g * 64 + 32 < W) words[2 * g + 1] = (uint32_t)(m >> 32);
}

constexpr int kBoolThreads = 256;

__global__ __launch_bounds__(kBoolThreads) void bool_windows_kernel(BoolParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (kBoolThreads / 64);
    const int64_t groups = (p.W + 63) >> 6;
    const WindowRowsArgs wr = {p.ts, p.first_idx, p.s0, p.n, p.interval, p.pre_rows, p.inclusive};
    unsigned long long nulls = 0;   // (the same in every lane)
    for (int64_t g = (int64_t)blockIdx.x * (kBoolThreads / 64) + (threadIdx.x >> 6); g < groups; g += nwaves) {
        const int64_t k = g * 64 + lane;
        const bool in = k < p.W;
        int64_t a = 0, b = 0;
        if (in) window_rows(wr, k, &a, &b);
        BoolAcc s;
        acc_init(s);
        const bool is_long = b - a > kBoolLaneRows;
        if (!is_long)
            for (int64_t r = a; r < b; r += 32) acc_chunk(p, r, (int)(b - r < 32 ? b - r : 32), r - a, s);
        uint64_t todo = __ballot(is_long);
        while (todo) {   // (uniform: every lane holds the same mask)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t wa = (int64_t)__shfl((long long)a, src), wb = (int64_t)__shfl((long long)b, src);
            BoolAcc t;
            acc_init(t);
            for (int64_t r = wa + 32 * (int64_t)lane; r < wb; r += 32 * 64) acc_chunk(p, r, (int)(wb - r < 32 ? wb - r : 32), r - wa, t);
            // (row << 1 | bit): the smallest first row and the largest last row carry their bits along
            const int64_t fkey = wave_min64(t.first < 0 ? INT64_MAX : ((t.first << 1) | (int64_t)t.fbit));
            const int64_t lkey = wave_max64(t.last < 0 ? -1 : ((t.last << 1) | (int64_t)t.lbit));
            const int64_t nv = wave_sum64(t.nv), nt = wave_sum64(t.nt);
            if (lane == src) {
                s.nv = nv; s.nt = nt;
                if (nv > 0) { s.first = fkey >> 1; s.fbit = (uint32_t)(fkey & 1); s.last = lkey >> 1; s.lbit = (uint32_t)(lkey & 1); }
            }
        }
        const bool has = in && s.nv > 0;
        const uint64_t in_m = __ballot(in), has_m = __ballot(has);
        nulls += (unsigned long long)__popcll(in_m & ~has_m);
        for (int o = 0; o < p.nouts; o++) {
            const BoolOut &q = p.outs[o];
            bool valid = has, is_bool = false, is_int = false, bval = false;
            uint64_t bits = 0;
            switch (q.kind) {
            case BOWGPU_AGG_SUM: valid = in; bits = (uint64_t)__double_as_longlong((double)s.nt); break;
            case BOWGPU_AGG_MEAN: bits = (uint64_t)__double_as_longlong((double)s.nt / (double)s.nv); break;
            case BOWGPU_AGG_MIN: bits = (uint64_t)__double_as_longlong(s.nt < s.nv ? 0.0 : 1.0); break;
            case BOWGPU_AGG_MAX: bits = (uint64_t)__double_as_longlong(s.nt > 0 ? 1.0 : 0.0); break;
            case BOWGPU_AGG_COUNT: valid = in; is_int = true; bits = (uint64_t)s.nv; break;
            case BOWGPU_AGG_FIRST: is_bool = true; bval = s.fbit != 0; break;
            case BOWGPU_AGG_LAST: is_bool = true; bval = s.lbit != 0; break;
            default: {   // BOWGPU_AGG_MODE
                const int64_t nf = s.nv - s.nt;
                is_bool = true;
                bval = s.nt > nf ? true : s.nt < nf ? false : s.lbit == 0;
            }
            }
            if (is_bool) store_word64(reinterpret_cast<uint32_t *>(q.values), g, p.W, lane, __ballot(valid && bval));
            else if (in) reinterpret_cast<uint64_t *>(q.values)[k] = valid ? apply_factors(bits, is_int, q.nfac, q.fac) : 0ull;   // nil slots hold 0 (bowbuffer.go:22-40)
            store_word64(q.valid, g, p.W, lane, __ballot(valid));
        }
    }
    if (lane == 0 && nulls) atomicAdd(p.null_windows, nulls);
}

__global__ __launch_bounds__(kBoolThreads) void bool_widen_kernel(const uint32_t *tbits, int64_t tbit0, const uint32_t *vbits, int64_t vbit0, int64_t n,
                                                                  double *out, uint32_t *out_valid) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (kBoolThreads / 64);
    const int64_t groups = (n + 63) >> 6;
    for (int64_t g = (int64_t)blockIdx.x * (kBoolThreads / 64) + (threadIdx.x >> 6); g < groups; g += nwaves) {
        const int64_t i = g * 64 + lane;
        const bool in = i < n;
        if (in) out[i] = bit_at(tbits, tbit0, i) ? 1.0 : 0.0;
        if (out_valid) store_word64(out_valid, g, n, lane, __ballot(in && bit_at(vbits, vbit0, i)));
    }
}

unsigned bool_grid(int64_t items) {
    int64_t g = (items + kBoolThreads - 1) / kBoolThreads;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

// every reducer P.outs names over one Boolean column; *P.null_windows must be zero
int launch_bool_windows(Ctx *c, const BoolParams &P) {
    if (P.W <= 0 || P.nouts <= 0) return 0;
    hipLaunchKernelGGL(bool_windows_kernel, dim3(bool_grid(P.W)), dim3(kBoolThreads), 0, c->stream, P);
    BG_HIP(hipGetLastError());
    return 0;
}

// out[i] = 1.0 / 0.0 for i < n; out_valid (may be nullptr: the column has no nulls): whole words of the validity from bit 0
int launch_bool_widen(Ctx *c, const uint32_t *tbits, int64_t tbit0, const uint32_t *vbits, int64_t vbit0, int64_t n, double *out, uint32_t *out_valid) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(bool_widen_kernel, dim3(bool_grid(n)), dim3(kBoolThreads), 0, c->stream, tbits, tbit0, vbits, vbit0, n, out, out_valid);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
