// The host arithmetic of a call over several devices (fan_call.cpp, sharded_call.cpp) as functions of plain data: who the fan-out
// serves, its row ranges, the Interpolate edge exchange, a rank's bitmap placed in the frame's, the merge of the ranks' infos.
// No device, no runtime, no Ctx: tests/fan_host_check.cpp links fan_host.cpp alone and runs it under ASan + UBSan.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/bowgpu.h"

namespace bowgpu {

// ranks a call of n rows is cut into: one per listed device, none with fewer than min_rows rows (< 2: not fanned out)
inline int fan_world(size_t n_ids, int64_t n, int64_t min_rows) { return (int)std::min<int64_t>((int64_t)n_ids, n / std::max<int64_t>(min_rows, 1)); }
// row ranges: multiples of 4096 rows (16-byte aligned value pointers, whole bitmap words) except the last one's end.  Trailing ranks
// may get 0 rows (10000 rows over 4 ranks: 4096 / 4096 / 1808 / 0); ADVICE r06 asks for an even cut - a change of behaviour, not made here
void fan_row_ranges(int64_t n, int world, int64_t *row0, int64_t *nrows);
// the gate: false - not a call for the fan-out, the one-device path serves it (first_ts, s0: the plan's)
bool fan_serves(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs, const bowgpu_interp *interps,
                int32_t ninterps, int64_t first_ts, int64_t s0);
// Interpolate -> Aggregate: what lies beyond rank r's two ends, from every rank's points (the "exchange"): *edge, and the caller's
// interpolators with the nearest valid point on the left as their PrevRow (the reference's own mechanism: linear.go:14-18)
void interp_edges(const bowgpu_interp_points *points, int world, int ncols, const bowgpu_interp *interps, int ninterps, int r,
                  bowgpu_interp_edge *edge, std::vector<bowgpu_interp> *rank_interps);

// ---------------------------------------------------------------- bit placement on the host
// A rank's bitmap (slot k at bit k) goes to bits [d0, d0 + nbits) of the frame's bitmap.  Whole bytes in the middle are stored by the
// rank itself; the first and last byte it touches may be shared with its neighbours and are handed to the calling thread as (index,
// mask, value) - applied after every rank is done (frame_bits_finish), so no two threads ever store to one byte.
struct EdgeByte { int64_t idx; uint8_t mask, val; };
inline uint64_t load_bits64(const uint8_t *src, int64_t bit) {   // 64 bits starting at source bit `bit` (src is padded: 16 readable bytes past the end)
    uint64_t lo, hi;
    memcpy(&lo, src + (bit >> 3), 8);
    memcpy(&hi, src + (bit >> 3) + 8, 8);
    const int r = (int)(bit & 7);
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
}
int64_t place_bits(const uint8_t *src, int64_t nbits, uint8_t *dst, int64_t d0, std::vector<EdgeByte> *edges);   // returns the bits set
// the bytes ranks share (first every bit some rank owns cleared, then set - a byte may hold the bits of several ranks), then the padding
// bits of the last byte cleared (bowbuffer.go:22-40 zero-initialises).  Returns the bytes of the frame's bitmap
int64_t frame_bits_finish(uint8_t *frame_bits, int64_t W, const std::vector<EdgeByte> *const *edges_by_rank, int world);

// the ranks' infos as one call's: long_windows summed, the largest kernel_ms, rank 0's new_interval_col / inclusive, the frame's s0 / W
// (out may be null).  *owned_total: the windows the ranks own; != 0 when that is not W - the caller words the failure
int merge_rank_infos(const bowgpu_agg_info *infos, const int64_t *windows_owned, int world, int64_t s0, int64_t W, bowgpu_agg_info *out,
                     int64_t *owned_total);

}  // namespace bowgpu
