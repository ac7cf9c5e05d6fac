// window_rows.h — the rows a reducer that reads a window through Window.UnsetInclusive sees (aggregation.Mode, mode.hip; the
// Boolean value reducers, rolling_bool.hip), from the first row of every window (interp_fill.hip window_first_rows_kernel).
#pragma once

#include <stdint.h>

namespace bowgpu {

// what the rule reads: first_idx[W + 1], the interval column and the call's plan
struct WindowRowsArgs {
    const int64_t *ts;
    const int64_t *first_idx;  // [W + 1] first row of every window
    int64_t s0, n, interval;
    int32_t pre_rows, inclusive;
};

__device__ __forceinline__ void window_rows(const WindowRowsArgs &p, int64_t k, int64_t *a, int64_t *b) {
    int64_t lo = p.first_idx[k], hi = p.first_idx[k + 1];
    // rows below s0 ride in window 0, but alone they do not make a window (rolling.go:177-239) - unless the call is inclusive
    // and the next window's first row sits exactly on its start: that row makes window 0 exist, and once it is dropped again
    // (Window.UnsetInclusive, window.go:23-31) the rows below s0 are what the reducer sees
    if (k == 0 && p.pre_rows && !(hi > 0 && p.ts[hi - 1] >= p.s0) && !(p.inclusive && hi < p.n && p.ts[hi] == p.s0 + p.interval)) hi = lo;
    *a = lo;
    *b = hi;
}

}  // namespace bowgpu
