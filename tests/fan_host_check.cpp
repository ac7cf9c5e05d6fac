// fan_host_check — the pure host steps of a call over several devices (bow_amd/csrc/fan_host.h) against naive models written here, bit by
// bit and rank by rank.  Links fan_host.cpp alone; tests/test_fan_host_cpu.py builds it with ASan + UBSan, so the buffers below have
// EXACTLY the sizes the product gives them: a read or store past them ends the program.  Fixed seed; prints the first mismatch; exit 1.
#include <stdio.h>
#include <stdlib.h>

#include "../bow_amd/csrc/fan_host.h"

using namespace bowgpu;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static int rnd_below(int n) { return (int)(rnd() % (uint64_t)n); }

#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) { printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
    } while (0)

// ---------------------------------------------------------------- bit placement
static const int64_t kLens[] = {0, 1, 2, 3, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000};
static const int kNumLens = (int)(sizeof kLens / sizeof kLens[0]);

static void check_layout(const std::vector<int64_t> &owned) {
    const int world = (int)owned.size();
    int64_t W = 0;
    for (int64_t o : owned) W += o;
    const size_t frame_bytes = (size_t)((W + 7) >> 3);
    uint8_t *frame = (uint8_t *)malloc(frame_bytes);   // exactly the frame's bitmap
    if (frame_bytes) memset(frame, 0xFF, frame_bytes);      // (so that "clear, then set" is what makes a 0 bit)
    std::vector<uint8_t> model((size_t)W);                  // one byte per bit
    std::vector<std::vector<EdgeByte>> edges(world);
    int64_t d0 = 0, returned = 0, model_set = 0;
    for (int r = 0; r < world; r++) {
        const size_t src_bytes = (size_t)((owned[r] + 7) >> 3) + 24;   // the padding rank_finish_impl gives
        uint8_t *src = (uint8_t *)malloc(src_bytes);
        for (size_t k = 0; k < src_bytes; k++) src[k] = (uint8_t)rnd();   // (bits past `owned` too: they must not reach the frame)
        for (int64_t k = 0; k < owned[r]; k++) {
            model[(size_t)(d0 + k)] = (uint8_t)((src[k >> 3] >> (k & 7)) & 1);
            model_set += model[(size_t)(d0 + k)];
        }
        returned += place_bits(src, owned[r], frame, d0, &edges[r]);
        free(src);
        d0 += owned[r];
    }
    std::vector<const std::vector<EdgeByte> *> by_rank(world);
    for (int r = 0; r < world; r++) by_rank[r] = &edges[r];
    const int64_t got_bytes = frame_bits_finish(frame, W, by_rank.data(), world);
    CHECK(got_bytes == (int64_t)frame_bytes, "frame_bits_finish says %lld bytes for %lld windows", (long long)got_bytes, (long long)W);
    int64_t popcount = 0;
    for (int64_t b = 0; b < (int64_t)frame_bytes * 8; b++) {
        const int bit = (frame[b >> 3] >> (b & 7)) & 1;
        const int want = b < W ? model[(size_t)b] : 0;   // (padding bits of the last byte: clear)
        popcount += bit;
        if (bit != want) {
            printf("MISMATCH bit %lld of %lld is %d, model %d; owned:", (long long)b, (long long)W, bit, want);
            for (int64_t o : owned) printf(" %lld", (long long)o);
            printf("\n");
            exit(1);
        }
    }
    CHECK(returned == popcount && popcount == model_set, "counts: place_bits %lld, frame %lld, model %lld", (long long)returned,
          (long long)popcount, (long long)model_set);
    free(frame);
}

static void check_bit_placement() {
    for (int a = 0; a < kNumLens; a++)
        for (int b = 0; b < kNumLens; b++) check_layout({kLens[a], kLens[b]});
    for (int it = 0; it < 2500; it++) {
        std::vector<int64_t> owned((size_t)(1 + rnd_below(6)));
        for (int64_t &o : owned) o = kLens[rnd_below(kNumLens)];
        check_layout(owned);
    }
}

// ---------------------------------------------------------------- row ranges, ranks of a call
static void check_row_ranges() {
    const int64_t ns[] = {1, 4095, 4096, 4097, 10000, 65536, 1 << 20, (1 << 20) + 1, 40000003};
    const int64_t min_rows[] = {1, 100, 1000, 1 << 20};
    for (int64_t n : ns)
        for (int world = 2; world <= 8; world++) {
            int64_t row0[8], nrows[8];
            fan_row_ranges(n, world, row0, nrows);
            const int64_t per = ((n / world) + 4095) / 4096 * 4096;   // the parent's rule, written out
            int64_t at = 0;
            for (int r = 0; r < world; r++) {
                int64_t end = at + per < n ? at + per : n;
                if (r == world - 1) end = n;
                CHECK(row0[r] == at && nrows[r] == end - at, "n %lld world %d rank %d: rows [%lld, +%lld), the rule says [%lld, +%lld)",
                      (long long)n, world, r, (long long)row0[r], (long long)nrows[r], (long long)at, (long long)(end - at));
                CHECK(row0[r] % 4096 == 0 || nrows[r] == 0, "n %lld world %d rank %d starts at row %lld", (long long)n, world, r, (long long)row0[r]);
                CHECK(nrows[r] >= 0, "n %lld world %d rank %d has %lld rows", (long long)n, world, r, (long long)nrows[r]);
                at = end;
            }
            CHECK(row0[0] == 0 && at == n, "n %lld world %d: the ranges end at %lld", (long long)n, world, (long long)at);
            for (int64_t m : min_rows) {
                const int64_t cut = n / m, want = cut < world ? cut : world;
                CHECK(fan_world((size_t)world, n, m) == (int)want, "fan_world(%d, %lld, %lld) = %d, not %lld", world, (long long)n, (long long)m,
                      fan_world((size_t)world, n, m), (long long)want);
            }
        }
    int64_t row0[4], nrows[4];
    fan_row_ranges(10000, 4, row0, nrows);
    CHECK(nrows[0] == 4096 && nrows[1] == 4096 && nrows[2] == 1808 && nrows[3] == 0, "10000 rows over 4 ranks: %lld / %lld / %lld / %lld",
          (long long)nrows[0], (long long)nrows[1], (long long)nrows[2], (long long)nrows[3]);
    CHECK(fan_world(4, 10, 0) == 4 && fan_world(4, 10, -5) == 4, "a row threshold below 1 counts as 1");
}

// ---------------------------------------------------------------- the gate
struct GateCall {
    bowgpu_col cols[9];
    bowgpu_agg aggs[17];
    bowgpu_interp interps[9];
    int32_t ncols = 3, naggs = 3, ninterps = 3;
    bool interpolate = false;
    int64_t first_ts = 100, s0 = 100;
    uint8_t some_bits[8] = {};
    GateCall() {
        memset(cols, 0, sizeof cols); memset(aggs, 0, sizeof aggs); memset(interps, 0, sizeof interps);
        for (int i = 0; i < 9; i++) { cols[i].type = i == 0 ? BOWGPU_INT64 : BOWGPU_FLOAT64; cols[i].length = 64; interps[i].col = i; }
        for (int i = 0; i < 17; i++) { aggs[i].kind = i == 0 ? BOWGPU_AGG_WINDOW_START : BOWGPU_AGG_SUM; aggs[i].col = i == 0 ? 0 : 1 + i % 2; }
    }
    bool served() const { return fan_serves(cols, ncols, 0, aggs, naggs, interpolate ? interps : nullptr, ninterps, first_ts, s0); }
};

static void check_gate() {
    { GateCall g; CHECK(g.served(), "a plain call is served"); }
    { GateCall g; g.naggs = 16; CHECK(g.served(), "16 aggregators are served"); }
    { GateCall g; g.cols[0].validity = g.some_bits; g.cols[0].null_count = 0; CHECK(g.served(), "an interval column with a bitmap and no nulls is served"); }
    { GateCall g; g.interpolate = true; CHECK(g.served(), "a plain Interpolate call is served"); }
    { GateCall g; g.interpolate = true; g.ncols = g.ninterps = 8; CHECK(g.served(), "Interpolate over 8 columns is served"); }
    { GateCall g; g.first_ts = 50; CHECK(g.served(), "rows below s0 matter to Interpolate only"); }
    { GateCall g; g.aggs[2].kind = BOWGPU_AGG_MODE; CHECK(!g.served(), "a Mode reducer"); }
    { GateCall g; g.cols[2].type = BOWGPU_BOOLEAN; CHECK(!g.served(), "a Boolean value column"); }
    { GateCall g; g.naggs = 17; CHECK(!g.served(), "17 aggregators"); }
    { GateCall g; g.cols[0].validity = g.some_bits; g.cols[0].null_count = 2; CHECK(!g.served(), "nulls in the interval column"); }
    { GateCall g; g.cols[0].validity = g.some_bits; g.cols[0].null_count = -1; CHECK(!g.served(), "an interval column whose nulls are not counted"); }
    { GateCall g; g.interpolate = true; g.ncols = g.ninterps = 9; CHECK(!g.served(), "nine columns with interpolators"); }
    { GateCall g; g.interpolate = true; g.ninterps = 2; CHECK(!g.served(), "fewer interpolators than columns"); }
    { GateCall g; g.interpolate = true; g.interps[1].col = 2; CHECK(!g.served(), "interps[1].col = 2"); }
    { GateCall g; g.interpolate = true; g.interps[2].col = 1; CHECK(!g.served(), "interps[2].col = 1"); }
    { GateCall g; g.interpolate = true; g.first_ts = 99; CHECK(!g.served(), "Interpolate with first_ts < s0"); }
}

// ---------------------------------------------------------------- Interpolate edges
static void check_interp_edges() {
    for (int it = 0; it < 3000; it++) {
        const int world = 1 + rnd_below(5), ncols = 1 + rnd_below(8);
        std::vector<bowgpu_interp_points> pts((size_t)world);
        const int dead_col = rnd_below(ncols + 1);   // a column without a valid point anywhere (ncols: none)
        for (bowgpu_interp_points &p : pts) {
            memset(&p, 0, sizeof p);
            p.nrows = rnd_below(3) == 0 ? 0 : 1 + rnd_below(1000);
            p.first_ts = (int64_t)rnd_below(1 << 20); p.last_ts = p.first_ts + rnd_below(1 << 20);
            for (int i = 0; i < 8; i++) {
                p.first_valid[i] = p.last_valid[i] = i != dead_col && rnd_below(3) != 0;   // (set on ranks of 0 rows too: nrows decides)
                p.first_t[i] = rnd_below(1 << 20); p.first_v[i] = rnd_below(1 << 20) / 8.0; p.last_t[i] = rnd_below(1 << 20);
                p.last_v[i] = rnd_below(1 << 20) / 8.0; p.last_v_i64[i] = (int64_t)rnd();
            }
        }
        std::vector<bowgpu_interp> given((size_t)ncols);
        for (int i = 0; i < ncols; i++) {
            memset(&given[i], 0, sizeof given[i]);
            given[i].kind = rnd_below(4); given[i].col = i; given[i].const_value = rnd_below(100);
            given[i].has_prev_row = rnd_below(2); given[i].prev_t_valid = rnd_below(2); given[i].prev_v_valid = rnd_below(2);
            given[i].prev_t = rnd_below(1000); given[i].prev_v = rnd_below(1000); given[i].prev_v_i64 = rnd_below(1000);
        }
        // the model: "last rank with rows" and per column "last valid point seen" carried left to right, "next valid" right to left
        std::vector<int> left_rows((size_t)world), prev((size_t)world * 8), next((size_t)world * 8);
        int carry = -1;
        for (int r = 0; r < world; r++) { left_rows[r] = carry; if (pts[r].nrows > 0) carry = r; }
        for (int i = 0; i < ncols; i++) {
            carry = -1;
            for (int r = 0; r < world; r++) { prev[r * 8 + i] = carry; if (pts[r].nrows > 0 && pts[r].last_valid[i]) carry = r; }
            carry = -1;
            for (int r = world - 1; r >= 0; r--) { next[r * 8 + i] = carry; if (pts[r].nrows > 0 && pts[r].first_valid[i]) carry = r; }
        }
        for (int r = 0; r < world; r++) {
            bowgpu_interp_edge want_edge, edge;
            memset(&want_edge, 0, sizeof want_edge);
            memset(&edge, 0xAB, sizeof edge);   // (whatever the rank's edge held before)
            std::vector<bowgpu_interp> want = given, got(3);
            if (left_rows[r] >= 0) { want_edge.has_left = 1; want_edge.left_last_ts = pts[left_rows[r]].last_ts; }
            for (int i = 0; i < ncols; i++) {
                if (const int q = prev[r * 8 + i]; q >= 0) {
                    want[i].has_prev_row = want[i].prev_t_valid = want[i].prev_v_valid = 1;
                    want[i].prev_t = pts[q].last_t[i]; want[i].prev_v = pts[q].last_v[i]; want[i].prev_v_i64 = pts[q].last_v_i64[i];
                }
                if (const int q = next[r * 8 + i]; q >= 0) {
                    want_edge.next_valid[i] = 1; want_edge.next_t[i] = pts[q].first_t[i]; want_edge.next_v[i] = pts[q].first_v[i];
                }
            }
            interp_edges(pts.data(), world, ncols, given.data(), ncols, r, &edge, &got);
            CHECK(memcmp(&edge, &want_edge, sizeof edge) == 0, "layout %d: the edge of rank %d of %d (%d columns) is not the model's", it, r, world, ncols);
            CHECK(got.size() == want.size() && memcmp(got.data(), want.data(), want.size() * sizeof want[0]) == 0,
                  "layout %d: the interpolators of rank %d of %d (%d columns) are not the model's", it, r, world, ncols);
        }
    }
}

// ---------------------------------------------------------------- info merge
static void check_info_merge() {
    for (int it = 0; it < 200; it++) {
        const int world = 1 + rnd_below(8);
        std::vector<bowgpu_agg_info> infos((size_t)world);
        std::vector<int64_t> owned((size_t)world);
        int64_t sum_long = 0, total = 0;
        double max_ms = 0;
        for (int r = 0; r < world; r++) {
            infos[r].s0 = rnd_below(100); infos[r].num_windows = rnd_below(100);   // (a rank's own: the frame's are the arguments)
            infos[r].new_interval_col = rnd_below(16); infos[r].inclusive = rnd_below(2);
            infos[r].long_windows = rnd_below(1000); infos[r].kernel_ms = rnd_below(1000) / 16.0;
            owned[r] = rnd_below(50) - 5;   // (a rank that owns nothing may say a negative count)
            sum_long += infos[r].long_windows;
            if (infos[r].kernel_ms > max_ms) max_ms = infos[r].kernel_ms;
            if (owned[r] > 0) total += owned[r];
        }
        bowgpu_agg_info out;
        int64_t got_total = -1;
        CHECK(merge_rank_infos(infos.data(), owned.data(), world, 1234, total, &out, &got_total) == 0 && got_total == total,
              "merge %d: %lld owned windows of %lld", it, (long long)got_total, (long long)total);
        CHECK(out.s0 == 1234 && out.num_windows == total && out.new_interval_col == infos[0].new_interval_col && out.inclusive == infos[0].inclusive &&
                  out.long_windows == sum_long && out.kernel_ms == max_ms, "merge %d: the merged info is not the model's", it);
        CHECK(merge_rank_infos(infos.data(), owned.data(), world, 1234, total, nullptr, &got_total) == 0 && got_total == total, "merge %d without an info", it);
        CHECK(merge_rank_infos(infos.data(), owned.data(), world, 1234, total + 1, &out, &got_total) != 0 && got_total == total,
              "merge %d: ranks that own %lld of %lld windows pass", it, (long long)total, (long long)total + 1);
    }
}

int main() {
    check_bit_placement();
    check_row_ranges();
    check_gate();
    check_interp_edges();
    check_info_merge();
    printf("fan_host_check: ok\n");
    return 0;
}
