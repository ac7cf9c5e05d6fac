// wave_ops.h — the wave64 primitives of the kernels, once: magic division, DPP moves and what is built from them (neighbour
// lanes, the inclusive scan, the reductions), 64-bit readlane, non-temporal 16-byte loads, the one-wave LDS ordering fence.
// The one place that names __builtin_amdgcn_update_dpp, the "wavefront" fence scope and an ext_vector_type typedef
// (tests/test_wave_ops_home.py).  bound_ctrl, the row mask and what a lane without a source receives are part of each name's
// contract - read them here, not at the call site.  (wave_scan.h holds the __shfl_up scan of the sort / filter / join kernels.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bowgpu {

// n / d for 32-bit n by the magic number (m, sh1, sh2) of d (the host computes it: agg_host.h)
__device__ __forceinline__ uint32_t mdiv32(uint32_t n, uint32_t m, uint32_t sh1, uint32_t sh2) {
    const uint32_t t = __umulhi(m, n);
    return (t + ((n - t) >> sh1)) >> sh2;
}

// ---- one DPP move of a 32-bit / 64-bit lane value (kCtrl: 0x111 .. 0x118 row_shr:1 .. 8 inside a row of 16 lanes, 0x142 / 0x143
// row_bcast:15 / 31, 0x138 / 0x130 wave_shr:1 / wave_shl:1).  dpp_*: lanes without a source receive 0
template <int kCtrl, int kRowMask, bool kBound>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kCtrl, kRowMask, 0xf, kBound);
}
template <int kCtrl, int kRowMask, bool kBound>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, kRowMask, 0xf, kBound);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, kRowMask, 0xf, kBound);
    return __hiloint2double(hi, lo);
}
// dpp_keep_*: a lane without a source (or of a masked row) keeps its own value: the identity of min / max
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_keep_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, kCtrl, kRowMask, 0xf, false);
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ double dpp_keep_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(x), __double2loint(x), kCtrl, kRowMask, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(x), __double2hiint(x), kCtrl, kRowMask, 0xf, false);
    return __hiloint2double(hi, lo);
}

// ---- the value of lane - 1 (wave_shr:1); lane 0 receives `lane0`
__device__ __forceinline__ uint32_t left_u32(uint32_t x, uint32_t lane0) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint64_t left_u64(uint64_t x, uint64_t lane0) {
    const uint32_t lo = left_u32((uint32_t)x, (uint32_t)lane0);
    const uint32_t hi = left_u32((uint32_t)(x >> 32), (uint32_t)(lane0 >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double left_f64(double x, double lane0) {
    return __longlong_as_double((long long)left_u64((uint64_t)__double_as_longlong(x), (uint64_t)__double_as_longlong(lane0)));
}
// ---- the value of lane + 1 (wave_shl:1); lane 63 receives `lane63`
__device__ __forceinline__ uint32_t right_u32(uint32_t x, uint32_t lane63) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane63, (int)x, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ double right_f64(double x, double lane63) {
    return __hiloint2double((int)right_u32((uint32_t)__double2hiint(x), (uint32_t)__double2hiint(lane63)),
                            (int)right_u32((uint32_t)__double2loint(x), (uint32_t)__double2loint(lane63)));
}

// ---- lane l's value, uniform (l is uniform).  The 64-bit forms read the high half first: the order every tile kernel had it in
__device__ __forceinline__ uint32_t readlane_u32(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }
__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, int l) {
    return ((uint64_t)readlane_u32((uint32_t)(x >> 32), l) << 32) | readlane_u32((uint32_t)x, l);
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// ---- 16-byte loads / 8-byte stores with the non-temporal hint (why and where: rolling_simple.hip, at the tile's loads)
typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ ulonglong2 load16_nt(const ulonglong2 *q) {
    const u64x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u64x2_t *>(q));
    return make_ulonglong2(v.x, v.y);
}
__device__ __forceinline__ void store8_nt(uint64_t *p, uint64_t v) { __builtin_nontemporal_store(v, p); }

// One wave only: LDS operations of a wave execute in order, so a write phase followed by reads from
// other lanes needs neither s_barrier nor a wait - only that the compiler keeps the program order.
// (__syncthreads() would also drain vmcnt(0), i.e. the next tile's prefetch.)
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive wave scan (row_shr 1 / 2 / 4 / 8 inside the 16-lane rows, row_bcast 15 / 31 across): six DPP moves + adds, no LDS
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t x) {
    x += dpp_u32<0x111, 0xf, true>(x); x += dpp_u32<0x112, 0xf, true>(x); x += dpp_u32<0x114, 0xf, true>(x);
    x += dpp_u32<0x118, 0xf, true>(x); x += dpp_u32<0x142, 0xa, false>(x); x += dpp_u32<0x143, 0xc, false>(x);
    return x;
}
// reductions over the wavefront by the same ladder: the total arrives in lane 63 (only there)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return wave_scan_u32(v); }
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_f64<0x111, 0xf, true>(v); v += dpp_f64<0x112, 0xf, true>(v); v += dpp_f64<0x114, 0xf, true>(v);
    v += dpp_f64<0x118, 0xf, true>(v); v += dpp_f64<0x142, 0xa, false>(v); v += dpp_f64<0x143, 0xc, false>(v);
    return v;
}
// (fmin / fmax: a NaN operand - a lane without a value - yields the other one)
__device__ __forceinline__ double wave_min_f64(double v) {
    v = fmin(v, dpp_keep_f64<0x111, 0xf>(v)); v = fmin(v, dpp_keep_f64<0x112, 0xf>(v)); v = fmin(v, dpp_keep_f64<0x114, 0xf>(v));
    v = fmin(v, dpp_keep_f64<0x118, 0xf>(v)); v = fmin(v, dpp_keep_f64<0x142, 0xa>(v)); v = fmin(v, dpp_keep_f64<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
    v = fmax(v, dpp_keep_f64<0x111, 0xf>(v)); v = fmax(v, dpp_keep_f64<0x112, 0xf>(v)); v = fmax(v, dpp_keep_f64<0x114, 0xf>(v));
    v = fmax(v, dpp_keep_f64<0x118, 0xf>(v)); v = fmax(v, dpp_keep_f64<0x142, 0xa>(v)); v = fmax(v, dpp_keep_f64<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    auto mn = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    v = mn(v, dpp_keep_u32<0x111, 0xf>(v)); v = mn(v, dpp_keep_u32<0x112, 0xf>(v)); v = mn(v, dpp_keep_u32<0x114, 0xf>(v));
    v = mn(v, dpp_keep_u32<0x118, 0xf>(v)); v = mn(v, dpp_keep_u32<0x142, 0xa>(v)); v = mn(v, dpp_keep_u32<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, dpp_keep_u32<0x111, 0xf>(v)); v = mx(v, dpp_keep_u32<0x112, 0xf>(v)); v = mx(v, dpp_keep_u32<0x114, 0xf>(v));
    v = mx(v, dpp_keep_u32<0x118, 0xf>(v)); v = mx(v, dpp_keep_u32<0x142, 0xa>(v)); v = mx(v, dpp_keep_u32<0x143, 0xc>(v));
    return v;
}

// __shfl_xor butterflies over 64-bit integers: every lane receives the result
__device__ __forceinline__ int64_t wave_sum64(int64_t x) {
    for (int o = 32; o > 0; o >>= 1) x += (int64_t)__shfl_xor((long long)x, o);
    return x;
}
__device__ __forceinline__ int64_t wave_min64(int64_t x) {
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = (int64_t)__shfl_xor((long long)x, o); x = y < x ? y : x; }
    return x;
}
__device__ __forceinline__ int64_t wave_max64(int64_t x) {
    for (int o = 32; o > 0; o >>= 1) { const int64_t y = (int64_t)__shfl_xor((long long)x, o); x = y > x ? y : x; }
    return x;
}

}  // namespace bowgpu
