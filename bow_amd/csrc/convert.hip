// convert.hip — Bow.Convert (reference bowsetters.go:52-56; Type.Convert, bowtypes.go:64-81; ToInt64 / ToFloat64 / ToBoolean,
// bowconvert.go) among Int64, Float64 and Boolean on the device: one streaming pass per column, hand-written for gfx950 (wave64); host
// orchestration in convert_api.cpp.
//
//   convert_kernel   one kernel over (source kind, target kind) - 8-byte values or bits in, 8-byte values or bits out - and up to
//                    kMoveCols columns (blockIdx.y), each with its own length and pair.  A wave walks trips of kTripRows rows; lane l
//                    holds rows 128 j + 2 l, + 1 of chunk j: one 16-byte load and one 16-byte store where the buffers allow them, all
//                    loads of a trip issued before any is used.  Bits - the validity, a Boolean column's values - are read wave-uniformly
//                    (load_bits128: scalar loads, re-based onto row 0) and written as whole 64-bit words by lane 0: the re-based validity
//                    word IS the output's validity word, a Boolean target's value word is the two ballots of the lanes' rows
//                    bit-interleaved.  Boolean to Boolean touches no 8-byte value: there a lane takes one 64-row word of both bitmaps
//                    (bitmap_word64) and stores value & validity and the validity.  Rows past n - 1 read as null, so the bits behind
//                    them in the last word are clear.  The valid rows of a column are counted from the same words: one atomicAdd of a
//                    64-bit integer per wave at the end of its walk, into one of kConvertShards words that the host sums.
//
// No output bit is written with an atomic and no workgroup waits on another: the bytes are a function of the input.
#include "common.h"
#include "bitmap_device.h"
#include "bitmap_word.h"
#include "wave_ops.h"

namespace bowgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunks = 4;                  // chunks of 128 rows a wave takes per trip
constexpr int kTripRows = 128 * kChunks;
constexpr int kMaxBlocks = 2048;            // per column: 8 workgroups a CU

// Go's int64(v) as gc compiles it for amd64 (CVTTSD2SQ): truncation toward zero inside [-2^63, 2^63), the "integer indefinite"
// 0x8000000000000000 for NaN, +-Inf and everything outside.  The range test is written out: (long long)double outside the range is
// undefined in C++.
__device__ __forceinline__ uint64_t go_int64(double v) {
    if (v >= -9223372036854775808.0 && v < 9223372036854775808.0) return (uint64_t)(long long)v;
    return 0x8000000000000000ull;
}

// one valid row, 8 bytes to 8 bytes
__device__ __forceinline__ uint64_t value_to_value(uint64_t x, int32_t from, int32_t to) {
    if (from == to) return x;   // the same bits: a NaN keeps its payload
    if (from == BOWGPU_INT64) return (uint64_t)__double_as_longlong(__ll2double_rn((long long)x));   // Go's float64(v): nearest, ties to even
    return go_int64(__longlong_as_double((long long)x));
}
// one valid row as a bool: v != 0 (a NaN is true, -0.0 is false)
__device__ __forceinline__ bool value_to_bool(uint64_t x, int32_t from) {
    return from == BOWGPU_FLOAT64 ? __longlong_as_double((long long)x) != 0.0 : x != 0;
}

// One trip of a wave over one column: rows [base, base + kTripRows) (kFull: all of them exist).  Returns the trip's valid rows.
template <bool kSrcBits, bool kDstBits, bool kFull>
__device__ __forceinline__ unsigned convert_trip(const ConvertCol &q, const int64_t base, const int lane, const bool vin, const bool vout) {
    static_assert(!(kSrcBits && kDstBits), "Boolean to Boolean is convert_walk_bits");
    const int64_t left = q.n - base;   // rows of the trip that exist: >= 1 (>= kTripRows when kFull)
    uint64_t a[kChunks], b[kChunks];
    if (!kSrcBits) {
        const uint64_t *src = reinterpret_cast<const uint64_t *>(q.src) + base;
#pragma unroll
        for (int k = 0; k < kChunks; k++) {
            const int r = 128 * k + 2 * lane;
            if (vin && (kFull || r + 1 < left)) {
                const u64x2_t x = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t *>(src + r));
                a[k] = x.x; b[k] = x.y;
            } else {
                a[k] = (kFull || r < left) ? __builtin_nontemporal_load(src + r) : 0;
                b[k] = (kFull || r + 1 < left) ? __builtin_nontemporal_load(src + r + 1) : 0;
            }
        }
    }
    const uint64_t one = q.to == BOWGPU_FLOAT64 ? 0x3FF0000000000000ull : 1ull;   // true as an 8-byte value
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < kChunks; k++) {
        const int64_t row0 = base + 128 * k;
        if (!kFull && row0 >= q.n) break;   // (the whole wave)
        const int r = 128 * k + 2 * lane;
        uint64_t v0, v1;   // the chunk's validity from row 0 of the chunk on; rows past n - 1: clear
        load_bits128<kFull>(q.vbits, q.vbit0, row0, q.n, &v0, &v1);
        cnt += (unsigned)(__popcll(v0) + __popcll(v1));
        const uint32_t vpair = (uint32_t)(lane < 32 ? v0 >> (2 * lane) : v1 >> (2 * lane - 64)) & 3u;   // the lane's two rows
        uint64_t o0 = 0, o1 = 0, oa = 0, ob = 0;   // a Boolean target's two words / the lane's two 8-byte results; a null slot holds 0
        if (kSrcBits) {
            uint64_t t0, t1;
            load_bits128<kFull>(reinterpret_cast<const uint32_t *>(q.src), q.sbit0, row0, q.n, &t0, &t1);
            const uint32_t tpair = (uint32_t)(lane < 32 ? (t0 & v0) >> (2 * lane) : (t1 & v1) >> (2 * lane - 64)) & 3u;
            oa = (tpair & 1u) ? one : 0;
            ob = (tpair & 2u) ? one : 0;
        } else if (kDstBits) {
            const unsigned long long e = __ballot((vpair & 1u) && value_to_bool(a[k], q.from));
            const unsigned long long o = __ballot((vpair & 2u) && value_to_bool(b[k], q.from));
            o0 = interleave32((uint32_t)e, (uint32_t)o);
            o1 = interleave32((uint32_t)(e >> 32), (uint32_t)(o >> 32));
        } else {
            oa = (vpair & 1u) ? value_to_value(a[k], q.from, q.to) : 0;
            ob = (vpair & 2u) ? value_to_value(b[k], q.from, q.to) : 0;
        }
        const bool second = kFull || row0 + 64 < q.n;   // the chunk reaches into its second 64-row word
        if (kDstBits) {
            if (lane == 0) {
                unsigned long long *w = reinterpret_cast<unsigned long long *>(q.out_values) + (row0 >> 6);
                w[0] = o0;
                if (second) w[1] = o1;
            }
        } else {
            uint64_t *dst = reinterpret_cast<uint64_t *>(q.out_values) + base;
            if (vout && (kFull || r + 1 < left)) {
                u64x2_t x;
                x.x = oa; x.y = ob;
                __builtin_nontemporal_store(x, reinterpret_cast<u64x2_t *>(dst + r));
            } else {
                if (kFull || r < left) __builtin_nontemporal_store(oa, dst + r);
                if (kFull || r + 1 < left) __builtin_nontemporal_store(ob, dst + r + 1);
            }
        }
        if (lane == 0) {
            unsigned long long *w = q.out_valid + (row0 >> 6);
            w[0] = v0;
            if (second) w[1] = v1;
        }
    }
    return cnt;
}

template <bool kSrcBits, bool kDstBits>
__device__ __forceinline__ unsigned long long convert_walk(const ConvertCol &q, const int64_t wave, const int64_t nwaves, const int lane) {
    // 16-byte accesses where row 0 lies on a 16-byte boundary (a trip starts a multiple of 512 rows behind it)
    const bool vin = !kSrcBits && (reinterpret_cast<uintptr_t>(q.src) & 15) == 0;
    const bool vout = !kDstBits && (reinterpret_cast<uintptr_t>(q.out_values) & 15) == 0;
    const int64_t ntrips = (q.n + kTripRows - 1) / kTripRows;
    unsigned long long valid = 0;
    for (int64_t t = wave; t < ntrips; t += nwaves) {
        const int64_t base = t * kTripRows;
        if (base + kTripRows <= q.n) valid += convert_trip<kSrcBits, kDstBits, true>(q, base, lane, vin, vout);
        else valid += convert_trip<kSrcBits, kDstBits, false>(q, base, lane, vin, vout);
    }
    return valid;
}

// Boolean to Boolean moves no 8-byte value: a lane takes one 64-row word of both bitmaps (three 32-bit words funnel-shifted onto row
// alignment), a wave 4096 rows a step
__device__ __forceinline__ unsigned long long convert_walk_bits(const ConvertCol &q, const int64_t wave, const int64_t nwaves, const int lane) {
    const int64_t nwords = (q.n + 63) >> 6;
    unsigned long long valid = 0;
    for (int64_t W = wave * 64 + lane; W < nwords; W += nwaves * 64) {
        const int64_t row0 = W * 64;
        unsigned long long v = q.n - row0 < 64 ? (1ull << (q.n - row0)) - 1ull : ~0ull;   // rows past n - 1: clear bits
        if (q.vbits) v &= bitmap_word64(q.vbits, q.vbit0, q.vwords, row0);
        reinterpret_cast<unsigned long long *>(q.out_values)[W] = v & bitmap_word64(reinterpret_cast<const uint32_t *>(q.src), q.sbit0, q.swords, row0);
        q.out_valid[W] = v;
        valid += (unsigned long long)__popcll(v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_xor(valid, o);
    return valid;
}

__global__ __launch_bounds__(kThreads) void convert_kernel(ConvertArgs a) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ci = (int)blockIdx.y;
    const ConvertCol &q = a.col[ci];
    const int64_t wave = (int64_t)blockIdx.x * kWaves + w, nwaves = (int64_t)gridDim.x * kWaves;
    if (wave * kTripRows >= q.n) return;   // (the whole wave; a column shorter than the launch's longest)
    const bool sbits = q.from == BOWGPU_BOOLEAN, dbits = q.to == BOWGPU_BOOLEAN;
    unsigned long long valid;
    if (sbits) valid = dbits ? convert_walk_bits(q, wave, nwaves, lane) : convert_walk<true, false>(q, wave, nwaves, lane);
    else valid = dbits ? convert_walk<false, true>(q, wave, nwaves, lane) : convert_walk<false, false>(q, wave, nwaves, lane);
    if (lane == 0 && valid) atomicAdd(a.valid_counts + ci * kConvertShards + (int)(wave & (kConvertShards - 1)), valid);
}

}  // namespace

// every column of a.col[0 .. ncols) with rows; a.valid_counts must be zero
int launch_convert(Ctx *c, const ConvertArgs &a) {
    if (a.ncols <= 0 || a.max_n <= 0) return 0;
    const int64_t ntrips = (a.max_n + kTripRows - 1) / kTripRows;
    int64_t blocks = (ntrips + kWaves - 1) / kWaves;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    hipLaunchKernelGGL(convert_kernel, dim3((unsigned)blocks, (unsigned)a.ncols), dim3(kThreads), 0, c->stream, a);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
