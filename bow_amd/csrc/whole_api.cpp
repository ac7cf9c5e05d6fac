// whole_api.cpp - the whole-frame aggregation.Aggregate (reference rolling/aggregation/whole.go): one window over every row.
// Host code validates, prepares residency and runs the whole_* kernels of interp_fill.hip and mode.hip.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"

using namespace bowgpu;

extern "C" {

int bowgpu_aggregate_whole(const bowgpu_col *cols, int32_t ncols, int32_t ts_col, const bowgpu_agg *aggs, int32_t naggs, bowgpu_out *outs) {
    // reference rolling/aggregation/whole.go:12-93
    if (!cols || ncols <= 0) return fail(BOWGPU_ERR_ARG, "nil bow");
    if (naggs <= 0) return fail(BOWGPU_ERR_NO_AGG, "at least one column aggregation is required");
    if (ts_col < 0 || ts_col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "no interval column with index %d", ts_col);
    if (!outs) return fail(BOWGPU_ERR_ARG, "no output columns");
    for (int i = 0; i < naggs; i++) {
        if (aggs[i].col < 0 || aggs[i].col >= ncols) return fail(BOWGPU_ERR_BAD_COL, "column aggregation %d: no column with index %d", i, aggs[i].col);
        if (aggs[i].kind < 0 || aggs[i].kind >= BOWGPU_AGG__COUNT) return fail(BOWGPU_ERR_ARG, "column aggregation %d: unknown kind", i);
        const int t = cols[aggs[i].col].type;
        if (t != BOWGPU_INT64 && t != BOWGPU_FLOAT64) return fail(BOWGPU_ERR_UNSUPPORTED, "column aggregation %d: column type outside the device path", i);
    }
    const int64_t n = cols[ts_col].length;
    auto out_type_of = [&](int i) {
        int t = kind_type(aggs[i].kind);
        // both InputDependent and IteratorDependent resolve to the INPUT column's type here (whole.go:44-46)
        if (t == BOWGPU_INPUT_DEPENDENT || t == BOWGPU_ITERATOR_DEPENDENT) t = cols[aggs[i].col].type;
        return t;
    };
    if (n == 0) {  // whole.go:49-50
        outs_empty(outs, naggs, out_type_of);
        return 0;
    }
    if (cols[ts_col].type != BOWGPU_INT64 && cols[ts_col].type != BOWGPU_FLOAT64) return fail(BOWGPU_ERR_UNSUPPORTED, "interval column type outside the device path");
    Ctx *c;
    BG_TRY(ctx_get(&c));
    BG_TRY(ts_contract(c, &cols[ts_col]));  // (the reference tolerates null ts here; the device path declines them)
    if (cols[ts_col].type != BOWGPU_INT64) return fail(BOWGPU_ERR_UNSUPPORTED, "whole-frame aggregation on the device path needs an Int64 interval column");
    DevCol dts;
    BG_TRY(ts_device(c, &cols[ts_col], &dts));
    // FirstValue / LastValue: int64(float64(first / last valid ts)) (whole.go:54-71).  The product path reads them in its finish
    // launch; the second implementation (BOWGPU_ROUTE_FORCE_GENERAL: whole_partial_kernel and the launches of rounds 1 - 5) on the host
    const bool general = (route_mask() & BOWGPU_ROUTE_FORCE_GENERAL) != 0;
    bool any_mode = false;
    for (int i = 0; i < naggs; i++) any_mode |= aggs[i].kind == BOWGPU_AGG_MODE;
    int64_t tfirst = 0, tlast = 0;
    if (general) {
        int64_t *hp;   // (one small kernel that stores both into the registered block: aggregate_api.cpp plan_make does the same)
        BG_TRY(registered_at(c, kRegTwoTs, &hp));
        BG_TRY(launch_fetch_two(c, reinterpret_cast<const int64_t *>(dts.values), 0, n - 1, hp));
        BG_HIP(hipStreamSynchronize(c->stream));
        tfirst = hp[0]; tlast = hp[1];
    }
    auto go_i64 = [](double x) -> int64_t { return (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) ? INT64_MIN : (int64_t)x; };
    const int64_t first_value = go_i64((double)tfirst), last_value = go_i64((double)tlast);
    // where the finish launches store what the host reads back: the context's registered block (values, then validity bytes)
    uint64_t *host_values;
    uint8_t *host_valid;
    BG_TRY(registered_at(c, kRegWholeValues, &host_values));
    BG_TRY(registered_at(c, kRegWholeValid, &host_valid));
    if (naggs > kWholeMaxAggs) return fail(BOWGPU_ERR_UNSUPPORTED, "whole-frame aggregation: at most %d aggregators per call", kWholeMaxAggs);

    int64_t nblocks = (n + 65535) / 65536;
    if (nblocks > 2048) nblocks = 2048;
    // (a multiple of the kernels' 512-row step: every workgroup's rows then start on a 16-byte boundary of the columns and on a byte of
    // the bitmap's rows; the workgroups this leaves without rows write the identity state)
    const int64_t chunk = ((n + nblocks - 1) / nblocks + 511) & ~(int64_t)511;
    // (one block of the context pool - no hipMalloc / hipFree per call: the partial states + the merged state of the column
    // (whole_run), one value and one validity byte per reducer)
    struct Part { void *p; } partials, onev, oneb;
    {
        const size_t pb = ((size_t)(nblocks + 1) * stats_size() + 255) & ~(size_t)255, vb = (8 * (size_t)naggs + 255) & ~(size_t)255;
        void *blk;
        BG_TRY(ctx_pool(c, kPoolWhole, pb + vb + 64 + (size_t)naggs, &blk));
        partials.p = blk; onev.p = reinterpret_cast<char *>(blk) + pb; oneb.p = reinterpret_cast<char *>(blk) + pb + vb;
    }
    std::vector<DevCol> dcols(ncols);
    std::vector<char> done(naggs, 0);
    // column `col` on the device, staged by the first reducer that reads it (the interval column: the copy the call already holds)
    auto device_col = [&](int col) -> int {
        DevCol &dc = dcols[col];
        if (dc.values != nullptr) return 0;
        if (col == ts_col) { dc.values = dts.values; dc.length = n; dc.type = BOWGPU_INT64; }
        else BG_TRY(devcol_prepare(c, &cols[col], &dc, true, true));
        return 0;
    };
    // reducer j of column `col` as the finish kernels read it (the callers add where its result goes)
    auto final_of = [&](int j, int col, WholeFinalH *F) {
        F->kind = aggs[j].kind; F->out_type = out_type_of(j); F->col_is_int = cols[col].type == BOWGPU_INT64;
        F->n_factors = aggs[j].n_factors;
        for (int k = 0; k < F->n_factors && k < BOWGPU_MAX_FACTORS; k++) F->factors[k] = aggs[j].factors[k];
    };
    // Mode (mode.go:8-32) over the one window [0, n): mode.hip, not the streaming partial states
    for (int i = 0; i < naggs; i++) {
        if (aggs[i].kind != BOWGPU_AGG_MODE) continue;
        done[i] = 1;
        const int col = aggs[i].col;
        BG_TRY(device_col(col));
        const DevCol &dc = dcols[col];
        DevBuf fi;
        BG_TRY(fi.alloc(64));
        const int64_t bounds[2] = {0, n};
        BG_HIP(hipMemcpyAsync(fi.p, bounds, 16, hipMemcpyHostToDevice, c->stream));
        BG_HIP(hipMemsetAsync(reinterpret_cast<char *>(fi.p) + 16, 0, 8, c->stream));
        uint32_t *word = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(fi.p) + 16);
        int64_t n_mid = 0, n_long = 0;
        BG_TRY(launch_mode(c, reinterpret_cast<const int64_t *>(dts.values), reinterpret_cast<const int64_t *>(fi.p), n, 0, 1, 1, 0, 0, dc.values, dc.vbits,
                           dc.vbit0, cols[col].type == BOWGPU_INT64, &aggs[i], reinterpret_cast<uint64_t *>(onev.p) + i, word, &n_mid, &n_long));
        BG_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t *>(oneb.p) + i, word, 1, hipMemcpyDeviceToDevice, c->stream));
        BG_HIP(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < naggs; i++) {
        if (done[i]) continue;
        // one pass per distinct input column: the partial state holds what every reducer needs
        const int col = aggs[i].col;
        BG_TRY(device_col(col));
        const DevCol &dc = dcols[col];
        WholeParamsH P;
        memset(&P, 0, sizeof P);
        P.ts = reinterpret_cast<const int64_t *>(dts.values);
        P.values = reinterpret_cast<const uint64_t *>(dc.values);
        P.vbits = dc.vbits; P.vbit0 = dc.vbit0; P.n = n; P.type = cols[col].type;
        P.need_ts = 0;
        for (int j = i; j < naggs; j++)
            if (aggs[j].col == col && aggs[j].kind >= BOWGPU_AGG_INTEGRAL_STEP && aggs[j].kind <= BOWGPU_AGG_WAVG_LINEAR) P.need_ts = 1;
        P.partials = partials.p; P.chunk = chunk;
        if (!general) {
            // the value kernel + ONE launch that merges its partials, evaluates every reducer of the column and stores the results where
            // the host reads them (kMaxAggs reducers per launch)
            BG_TRY(whole_value_run(c, &P, nblocks));
            std::vector<int> mine;
            for (int j = i; j < naggs; j++) if (aggs[j].col == col && !done[j]) { mine.push_back(j); done[j] = 1; }
            for (size_t at = 0; at < mine.size(); at += kMaxAggs) {
                WholeFinishH fin;
                memset(&fin, 0, sizeof fin);
                fin.ts = reinterpret_cast<const int64_t *>(dts.values); fin.nrows = n;
                fin.n = (int32_t)std::min<size_t>(kMaxAggs, mine.size() - at);
                fin.host_values = host_values; fin.host_valid = host_valid;
                for (int q = 0; q < fin.n; q++) {
                    const int j = mine[at + q];
                    final_of(j, col, &fin.f[q]);
                    fin.slot[q] = j;
                }
                BG_TRY(whole_finish_run(c, partials.p, nblocks, fin));
            }
            continue;
        }
        BG_TRY(whole_run(c, &P, nblocks));
        for (int j = i; j < naggs; j++) {
            if (aggs[j].col != col || done[j]) continue;
            done[j] = 1;
            WholeFinalH F;
            memset(&F, 0, sizeof F);
            final_of(j, col, &F);
            F.out_value = reinterpret_cast<uint64_t *>(onev.p) + j;
            F.out_valid_byte = reinterpret_cast<uint8_t *>(oneb.p) + j;
            BG_TRY(whole_final_run(c, reinterpret_cast<const char *>(partials.p) + (size_t)nblocks * stats_size(), 1, n, first_value, last_value, &F));
        }
    }
    std::vector<uint64_t> hv(naggs);
    std::vector<uint8_t> hb(naggs);
    if (general || any_mode) {   // (Mode's outputs, and everything of the second implementation, leave through the device block)
        BG_HIP(hipMemcpyAsync(hv.data(), onev.p, 8 * (size_t)naggs, hipMemcpyDeviceToHost, c->stream));
        BG_HIP(hipMemcpyAsync(hb.data(), oneb.p, (size_t)naggs, hipMemcpyDeviceToHost, c->stream));
    }
    BG_HIP(hipStreamSynchronize(c->stream));   // THE synchronisation of the call
    if (!general)
        for (int i = 0; i < naggs; i++)
            if (aggs[i].kind != BOWGPU_AGG_MODE) { hv[i] = host_values[i]; hb[i] = host_valid[i]; }
    bool any_device = false;
    std::vector<uint8_t> vbs(naggs);
    for (int i = 0; i < naggs; i++) {
        if (outs[i].length < 1 || !outs[i].values || !outs[i].validity) return fail(BOWGPU_ERR_ARG, "output column %d needs one slot", i);
        vbs[i] = hb[i] ? 1 : 0;
        if (outs[i].residency == BOWGPU_DEVICE) {   // (one synchronisation behind all of them; host-resident slots are plain stores)
            BG_HIP(hipMemcpyAsync(outs[i].values, &hv[i], 8, hipMemcpyHostToDevice, c->stream));
            BG_HIP(hipMemcpyAsync(outs[i].validity, &vbs[i], 1, hipMemcpyHostToDevice, c->stream));
            any_device = true;
        } else {
            memcpy(outs[i].values, &hv[i], 8);
            *outs[i].validity = vbs[i];
        }
        outs[i].length = 1;
        outs[i].null_count = vbs[i] ? 0 : 1;
        outs[i].type = out_type_of(i);
    }
    if (any_device) BG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
