// equal_api.cpp — C-ABI entry points of the per-row half of Bow.Equal (reference bow.go:227-275), of the search behind GetPrevRowIndex /
// GetNextRowIndex / GetPrevValue(s) / GetNextValue(s) (bowgetters.go:65-151) and of IsColEmpty (bowassertion.go:84-86): bowgpu_equal,
// bowgpu_valid_row, bowgpu_is_col_empty.  Host code validates, answers what needs no data, prepares residency and launches the kernels
// of equal.hip; no value is compared and no validity bit is looked at on the CPU.
#include <string.h>

#include <vector>

#include "common.h"

using namespace bowgpu;

namespace {

constexpr int64_t kEqualMaxRows = (int64_t)1 << 31;   // rows inside the kernels are 32 bits wide

int too_many_rows(int64_t n) {
    return fail(BOWGPU_ERR_UNSUPPORTED, "the column has %lld rows: the device path serves fewer than 2^31 = 2147483648 rows", (long long)n);
}

// what can be said about one frame of bowgpu_equal without reading a column
int equal_frame_checks(const bowgpu_col *cols, int32_t ncols) {
    for (int i = 0; i < ncols; i++) {
        if (cols[i].length < 0 || cols[i].offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (cols[i].length != cols[0].length) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        if (cols[i].type == BOWGPU_STRING) return fail(BOWGPU_ERR_UNSUPPORTED, "column %d is of unsupported type (utf8): Int64 / Float64 / Boolean only", i);
        if (!movable_type(cols[i].type) && cols[i].type != BOWGPU_BOOLEAN)
            return fail(BOWGPU_ERR_UNSUPPORTED, "column %d is of unsupported type (Int64 / Float64 / Boolean only)", i);
        if (!residency_ok(cols[i].residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", cols[i].residency);
    }
    if (ncols > 0 && cols[0].length >= kEqualMaxRows) return too_many_rows(cols[0].length);
    return 0;
}

BitsAt bits_at(const DevBits &b) { return BitsAt{b.words, b.bit0, b.nwords}; }

// the staged copies of one launch group: they go back behind the group's synchronise
struct EqualStaged {
    DevCol cols[2 * kMoveCols];
    DevBoolCol bools[2 * kMoveCols];
};

// one side of one column into its EqualCol
int equal_side(Ctx *c, const bowgpu_col &col, int side, EqualStaged *st, int slot, EqualCol *e) {
    if (col.type == BOWGPU_BOOLEAN) {
        DevBoolCol &b = st->bools[slot];
        BG_TRY(devboolcol_prepare(c, &col, &b));
        e->truth[side] = bits_at(b.t);
        e->valid[side] = bits_at(b.v);
        return 0;
    }
    DevCol &dc = st->cols[slot];
    const bowgpu_col k = uncounted(col);
    BG_TRY(devcol_prepare(c, &k, &dc, true, true));
    e->values[side] = reinterpret_cast<const uint64_t *>(dc.values);
    e->valid[side] = BitsAt{dc.vbits, dc.vbit0, dc.vwords};
    return 0;
}

int equal_group(Ctx *c, const bowgpu_col *left, const bowgpu_col *right, int32_t g0, int32_t gc, int32_t mode, int64_t n, unsigned long long *result,
                EqualStaged *st) {
    EqualArgs a;
    memset(&a, 0, sizeof a);
    a.ncols = gc;
    a.n = n;
    a.result = result;
    for (int i = 0; i < gc; i++) {
        EqualCol &e = a.col[i];
        const int32_t t = left[g0 + i].type;
        e.kind = t == BOWGPU_BOOLEAN ? kEqualBool : (t == BOWGPU_FLOAT64 && mode == BOWGPU_EQUAL_GO) ? kEqualIeee : kEqualBits;
        e.col = g0 + i;
        BG_TRY(equal_side(c, left[g0 + i], 0, st, 2 * i, &e));
        BG_TRY(equal_side(c, right[g0 + i], 1, st, 2 * i + 1, &e));
    }
    return launch_equal(c, a);
}

// a column's bitmap where the call has to read it
int stage_validity(Ctx *c, const bowgpu_col &col, DevBits *b) {
    return stage_bits(c, col.validity, col.offset, col.length, col.residency, "validity", b);
}

}  // namespace

extern "C" {

int bowgpu_equal(const bowgpu_col *left, const bowgpu_col *right, int32_t ncols, int32_t mode, bowgpu_equal_info *info) {
    if (!info) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ncols < 0) return fail(BOWGPU_ERR_ARG, "negative column count");
    if (mode != BOWGPU_EQUAL_GO && mode != BOWGPU_EQUAL_BITS) return fail(BOWGPU_ERR_ARG, "unknown mode %d", mode);
    if (ncols > 0 && (!left || !right)) return fail(BOWGPU_ERR_ARG, "null argument");
    BG_TRY(equal_frame_checks(left, ncols));
    BG_TRY(equal_frame_checks(right, ncols));
    info->equal = 1;
    info->first_col = -1;
    info->first_row = -1;
    if (ncols == 0) return 0;
    for (int i = 0; i < ncols; i++)
        if (left[i].type != right[i].type) {   // Schema().Equal: bow.go:243-245
            info->equal = 0;
            info->first_col = i;
            return 0;
        }
    const int64_t n = left[0].length;
    if (n != right[0].length) {
        info->equal = 0;
        return 0;
    }
    if (n == 0) return 0;
    Ctx *c;
    BG_TRY(ctx_get(&c));
    unsigned long long *d_word, *h_word;
    BG_TRY(scratch_at(c, kScrEqualWord, &d_word));
    BG_TRY(registered_at(c, kRegEqualWord, &h_word));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(launch_equal_preset(c, d_word));
    for (int g0 = 0; g0 < ncols; g0 += kMoveCols) {
        const int gc = ncols - g0 < kMoveCols ? ncols - g0 : kMoveCols;
        EqualStaged staged;
        BG_TRY(synced(c, equal_group(c, left, right, g0, gc, mode, n, d_word, &staged)));
        bool copies = false;
        for (int i = 0; i < 2 * gc; i++)
            copies |= staged.cols[i].own_values.p || staged.cols[i].own_validity.p || staged.bools[i].t.own.p || staged.bools[i].v.own.p;
        if (copies) BG_HIP(hipStreamSynchronize(c->stream));   // (columns read where they lie: the groups follow each other without one)
    }
    BG_TRY(synced(c, launch_equal_result(c, d_word, h_word)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    const unsigned long long word = *const_cast<const volatile unsigned long long *>(h_word);
    if (word != kEqualNone) {
        info->equal = 0;
        info->first_row = (int64_t)(word >> 32);
        info->first_col = (int32_t)(word & 0xFFFFFFFFull);
    }
    kernel_done(c, "equal_kernel");
    return 0;
}

int bowgpu_valid_row(const bowgpu_col *cols, int32_t ncols, int64_t row_start, int32_t direction, int64_t *row) {
    if (!cols || !row) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ncols < 1) return fail(BOWGPU_ERR_ARG, "no column to look at (%d)", ncols);
    if (ncols > BOWGPU_VALID_ROW_MAX_COLS)
        return fail(BOWGPU_ERR_ARG, "%d columns: a valid-row search takes at most BOWGPU_VALID_ROW_MAX_COLS = %d", ncols, BOWGPU_VALID_ROW_MAX_COLS);
    if (direction != 1 && direction != -1) return fail(BOWGPU_ERR_ARG, "direction %d: +1 or -1", direction);
    const int64_t n = cols[0].length;
    for (int i = 0; i < ncols; i++) {
        if (cols[i].length < 0 || cols[i].offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (cols[i].length != n) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        if (!residency_ok(cols[i].residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", cols[i].residency);
    }
    if (n >= kEqualMaxRows) return too_many_rows(n);
    *row = -1;
    if (row_start < 0 || row_start >= n) return 0;   // the loops' guard: bowgetters.go:68, :129
    ValidRowArgs a;
    memset(&a, 0, sizeof a);
    const bowgpu_col *look[BOWGPU_VALID_ROW_MAX_COLS];
    for (int i = 0; i < ncols; i++)
        if (has_bitmap(cols[i])) look[a.ncols++] = &cols[i];
    if (a.ncols == 0) {
        *row = row_start;
        return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevBits bits[BOWGPU_VALID_ROW_MAX_COLS];   // (bitmaps alone: eight of them are the bytes of one column of values)
    for (int i = 0; i < a.ncols; i++) {
        BG_TRY(synced(c, stage_validity(c, *look[i], &bits[i])));
        a.valid[i] = bits_at(bits[i]);
    }
    a.direction = direction;
    a.n = n;
    a.row_start = row_start;
    BG_TRY(synced(c, scratch_at(c, kScrFlags, &a.result)));
    BG_TRY(synced(c, registered_at(c, kRegFindRow, &a.host_result)));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, launch_valid_row(c, a)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    const uint32_t found = *const_cast<const volatile uint32_t *>(a.host_result);
    if (found != kFindNone) *row = (int64_t)found;
    kernel_done(c, "valid_row_kernel");
    return 0;
}

int bowgpu_is_col_empty(const bowgpu_col *col, int32_t *empty) {
    if (!col || !empty) return fail(BOWGPU_ERR_ARG, "null argument");
    if (col->length < 0 || col->offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
    if (!residency_ok(col->residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col->residency);
    const int64_t n = col->length;
    if (n == 0 || !has_bitmap(*col) || col->null_count > 0) {   // NullN() == Len() from what the column states
        *empty = n == 0 || (has_bitmap(*col) && col->null_count == n);
        return 0;
    }
    Ctx *c;
    BG_TRY(ctx_get(&c));
    DevBits b;
    BG_TRY(synced(c, stage_validity(c, *col, &b)));
    uint64_t *d_count;
    BG_TRY(synced(c, scratch_at(c, kScrNullCount, &d_count)));
    BG_HIP(hipEventRecord(c->ev0, c->stream));
    BG_TRY(synced(c, launch_popcount(c, b.words, b.bit0, n, d_count)));
    BG_HIP(hipEventRecord(c->ev1, c->stream));
    uint64_t set = 0;
    BG_HIP(hipMemcpyAsync(&set, d_count, 8, hipMemcpyDeviceToHost, c->stream));
    BG_HIP(hipStreamSynchronize(c->stream));
    *empty = set == 0;
    kernel_done(c, "popcount_kernel");
    return 0;
}

}  // extern "C"
