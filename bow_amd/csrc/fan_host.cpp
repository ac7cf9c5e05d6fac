// fan_host.cpp — the pure steps of fan_host.h (no device is touched here)
#include "fan_host.h"

namespace bowgpu {

void fan_row_ranges(int64_t n, int world, int64_t *row0, int64_t *nrows) {
    const int64_t per = ((n / world) + 4095) & ~(int64_t)4095;
    int64_t at = 0;
    for (int r = 0; r < world; r++) {
        const int64_t end = r + 1 == world ? n : std::min<int64_t>(n, at + per);
        row0[r] = at;
        nrows[r] = end - at;
        at = end;
    }
}

bool fan_serves(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs, const bowgpu_interp *interps,
                int32_t ninterps, int64_t first_ts, int64_t s0) {
    if (naggs > BOWGPU_CARRY_MAX_AGGS) return false;
    for (int i = 0; i < naggs; i++) if (aggs[i].kind == BOWGPU_AGG_MODE) return false;
    for (int i = 0; i < naggs; i++) if (cols[aggs[i].col].type == BOWGPU_BOOLEAN) return false;   // (Boolean columns: no record for bit ranges, the caller's device serves the call)
    if (cols[ts_col].validity && cols[ts_col].null_count != 0) return false;   // (nulls in the interval column: the one-device path serves them)
    if (interps) {
        // the sharded Interpolate's own limit (include/bowgpu.h): at most 8 columns (bowgpu_interp_edge).  Rows below the first window start
        // (a negative first timestamp under Go's truncating division) make the interpolated frame start with its synthetic row at s0 and go
        // on BELOW it: what Aggregate then does with that frame is the one-device path's business
        if (ncols > 8 || ninterps != ncols || first_ts < s0) return false;
        for (int i = 0; i < ncols; i++) if (interps[i].col != i) return false;
    }
    return true;
}

void interp_edges(const bowgpu_interp_points *points, int world, int ncols, const bowgpu_interp *interps, int ninterps, int r,
                  bowgpu_interp_edge *edge, std::vector<bowgpu_interp> *rank_interps) {
    memset(edge, 0, sizeof *edge);
    rank_interps->assign(interps, interps + ninterps);
    int left_last = -1;
    for (int q = 0; q < r; q++) if (points[q].nrows > 0) left_last = q;
    if (left_last >= 0) { edge->has_left = 1; edge->left_last_ts = points[left_last].last_ts; }
    for (int i = 0; i < ncols; i++) {
        for (int q = r - 1; q >= 0; q--) {      // nearest valid point on the left
            const bowgpu_interp_points &pq = points[q];
            if (pq.nrows > 0 && pq.last_valid[i]) {
                bowgpu_interp &ip = (*rank_interps)[i];
                ip.has_prev_row = 1; ip.prev_t_valid = 1; ip.prev_v_valid = 1;
                ip.prev_t = pq.last_t[i]; ip.prev_v = pq.last_v[i]; ip.prev_v_i64 = pq.last_v_i64[i];
                break;
            }
        }
        for (int q = r + 1; q < world; q++) {   // nearest valid point on the right
            const bowgpu_interp_points &pq = points[q];
            if (pq.nrows > 0 && pq.first_valid[i]) {
                edge->next_valid[i] = 1; edge->next_t[i] = pq.first_t[i]; edge->next_v[i] = pq.first_v[i];
                break;
            }
        }
    }
}

int64_t place_bits(const uint8_t *src, int64_t nbits, uint8_t *dst, int64_t d0, std::vector<EdgeByte> *edges) {
    if (nbits <= 0) return 0;
    int64_t set = 0;
    const int64_t B0 = d0 >> 3, B1 = (d0 + nbits - 1) >> 3;
    auto byte_at = [&](int64_t B, uint8_t *mask) -> uint8_t {   // dest byte B: its bits that belong to this rank, and their values
        const int64_t lo = std::max<int64_t>(B * 8, d0), hi = std::min<int64_t>(B * 8 + 8, d0 + nbits);   // [lo, hi) global bits
        const uint64_t v = load_bits64(src, lo - d0);
        const int cnt = (int)(hi - lo), sh = (int)(lo - B * 8);
        const uint8_t m = (uint8_t)(((1u << cnt) - 1u) << sh);
        *mask = m;
        return (uint8_t)(((uint32_t)(v & ((1u << cnt) - 1u))) << sh);
    };
    uint8_t m, v = byte_at(B0, &m);
    edges->push_back({B0, m, v});
    set += __builtin_popcount(v);
    if (B1 > B0) {
        v = byte_at(B1, &m);
        edges->push_back({B1, m, v});
        set += __builtin_popcount(v);
    }
    int64_t B = B0 + 1;
    for (; B + 8 <= B1; B += 8) {   // eight whole destination bytes per step
        const uint64_t w = load_bits64(src, B * 8 - d0);
        memcpy(dst + B, &w, 8);
        set += __builtin_popcountll(w);
    }
    for (; B < B1; B++) {
        const uint8_t b = (uint8_t)load_bits64(src, B * 8 - d0);
        dst[B] = b;
        set += __builtin_popcount(b);
    }
    return set;
}

int64_t frame_bits_finish(uint8_t *fb, int64_t W, const std::vector<EdgeByte> *const *edges_by_rank, int world) {
    const int64_t frame_bytes = (W + 7) >> 3;
    for (int r = 0; r < world; r++) for (const EdgeByte &e : *edges_by_rank[r]) fb[e.idx] &= (uint8_t)~e.mask;
    for (int r = 0; r < world; r++) for (const EdgeByte &e : *edges_by_rank[r]) fb[e.idx] |= e.val;
    if (W & 7) fb[frame_bytes - 1] &= (uint8_t)((1u << (W & 7)) - 1u);
    return frame_bytes;
}

int merge_rank_infos(const bowgpu_agg_info *infos, const int64_t *windows_owned, int world, int64_t s0, int64_t W, bowgpu_agg_info *out,
                     int64_t *owned_total) {
    *owned_total = 0;
    for (int r = 0; r < world; r++) *owned_total += std::max<int64_t>(windows_owned[r], 0);
    if (*owned_total != W) return 1;
    if (!out) return 0;
    out->s0 = s0; out->num_windows = W; out->new_interval_col = infos[0].new_interval_col; out->inclusive = infos[0].inclusive;
    out->long_windows = 0; out->kernel_ms = 0;
    for (int r = 0; r < world; r++) {
        out->long_windows += infos[r].long_windows;
        out->kernel_ms = std::max(out->kernel_ms, infos[r].kernel_ms);
    }
    return 0;
}

}  // namespace bowgpu
