// parquet_decode.hip — device side of the Parquet column-chunk loader (reference bowparquet.go:44-153 reads
// the file with parquet-go into []interface{} rows and SetOrDrop's every value, bowparquet.go:101-105).  Here the compressed
// pages of one column travel to HBM as they lie in the file and are decoded there, one wavefront per page:
//
//   snappy_pages_kernel   raw Snappy block -> the page's uncompressed bytes.  All 64 lanes parse the same element header (uniform
//                         control flow), then copy cooperatively: a literal is a plain strided copy; a back-reference of
//                         `len` bytes at distance `off` is periodic with period `off` when it overlaps itself, so
//                         dst[i] = base[off >= len ? i : i % off] is parallel in every case.
//   dict_indices_kernel   dictionary-encoded data pages: bit width byte + RLE / bit-packed hybrid of indices -> dense uint32 array
//   delta_pages_kernel    DELTA_BINARY_PACKED data pages (INT64): header + blocks of bit-packed miniblocks -> dense int64 array, one
//                         slot per non-null value.  All lanes parse the same block headers; per 64 values of a miniblock each lane
//                         extracts one delta, a wrapping inclusive wave scan + the carry of the values before give the values.
//   bss_pages_kernel      BYTE_STREAM_SPLIT data pages (INT64 / DOUBLE): the eight byte streams of a page -> the same dense array
//                         (lane i assembles value i: every stream is read and the array written in consecutive addresses).
//   page_scatter_kernel   data page (v1 / v2) of a flat OPTIONAL / REQUIRED INT64 / DOUBLE column: definition levels
//                         (RLE / bit-packed hybrid, bit width 1) -> Arrow validity bits; dense PLAIN / expanded values -> row slots
//                         (null slots = 0, as bow.NewBuffer leaves them: bowbuffer.go:22-40).  Lane l owns rows 32k + l ... of the
//                         page in words of 32: level word, popcount, wave scan = index of its first value.
//   bool_pages_kernel     data page (v1 / v2) of a flat OPTIONAL / REQUIRED BOOLEAN column: the same level words -> validity bits; the
//                         page's dense value bits (PLAIN: one bit each; RLE: 4-byte length + RLE / bit-packed hybrid, bit width 1)
//                         -> Arrow value bits, deposited onto the set positions of the lane's validity word (null rows = 0).  No
//                         expansion pass and no per-row workspace: a lane takes its bits [vi, vi + popcount) straight from the page.
#include "agg_device.h"
#include "wave_scan.h"

namespace bowgpu {

struct PqPage {
    int64_t src_off;        // payload offset inside the uploaded column chunk bytes
    int64_t raw_off;        // offset of the page's uncompressed bytes inside the scratch buffer (or the chunk, if stored raw)
    int64_t row0;           // first output row of the page
    int32_t comp_size, raw_size;
    int32_t num_values;     // rows of the page (levels); non-null values = what the levels say
    int32_t compressed;     // 1: Snappy
    int32_t kind;           // 0: data page, PLAIN values; 1: data page, dictionary indices; 2: the chunk's dictionary page (PLAIN values);
                            // 3: data page, DELTA_BINARY_PACKED; 4: data page, BYTE_STREAM_SPLIT;
                            // 5: data page of a BOOLEAN column, PLAIN bits; 6: data page of a BOOLEAN column, RLE (bool_pages_kernel)
    int32_t dict_count;     // kind 1: entries of the chunk's dictionary
    int64_t dict_off;       // kind 1: offset of the dictionary's values (same buffer as raw_off)
    int64_t idx_off;        // kind 1: first slot of this page in the expanded index array; kind 3 / 4: in the expanded value array
    int64_t lv_off;         // data page v2: offset of the definition-level bytes inside the chunk bytes (never compressed there)
    int32_t lv_len;         // data page v2: their length (v1 pages carry a 4-byte length in front of the levels instead)
    int32_t v2;             // data page v2: src / raw describe the VALUES section only
    int32_t dict_in_raw;    // kind 1: the dictionary was decompressed (it lives in the scratch buffer, else in the chunk bytes)
    int32_t _pad;
};

namespace {

__device__ __forceinline__ uint32_t rd_varint(const uint8_t *p, int64_t *pos, int64_t end) {
    uint32_t r = 0;
    int sh = 0;
    while (*pos < end) {
        const uint8_t c = p[(*pos)++];
        r |= (uint32_t)(c & 0x7f) << sh;
        if (!(c & 0x80)) break;
        sh += 7;
        if (sh > 28) break;
    }
    return r;
}

// ULEB128 of up to 10 bytes (DELTA_BINARY_PACKED: first_value and min_delta are zigzag 64-bit).  false: the bytes ran out or the
// number did not end within 10 bytes; *pos never passes end.
__device__ __forceinline__ bool rd_varint64(const uint8_t *p, int64_t *pos, int64_t end, uint64_t *out) {
    uint64_t r = 0;
    for (int sh = 0; sh < 70; sh += 7) {
        if (*pos >= end) return false;
        const uint8_t c = p[(*pos)++];
        r |= (uint64_t)(c & 0x7f) << sh;   // (the 10th byte's high bits fall off: wrapping, like the writers' decoders)
        if (!(c & 0x80)) { *out = r; return true; }
    }
    return false;
}

__device__ __forceinline__ uint64_t unzigzag64(uint64_t v) { return (v >> 1) ^ (0ull - (v & 1ull)); }

// Offset of a data page's values section inside its bytes: v1 pages of an OPTIONAL column carry a 4-byte length and the definition
// levels in front of it.  -1: the length runs past the page.
__device__ __forceinline__ int64_t values_offset(const uint8_t *src, const PqPage &P, int optional) {
    if (!optional || P.v2) return 0;
    if (P.raw_size < 4) return -1;
    const uint32_t lbytes = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
    if ((int64_t)lbytes + 4 > P.raw_size) return -1;
    return 4 + (int64_t)lbytes;
}

// status bits of the scatter kernels (page_scatter_kernel, bool_pages_kernel).  1 (a broken Snappy block), 8 (an index outside the
// dictionary) and 16 (a broken index stream) stay literals of the one kernel each that raises them
constexpr uint32_t kStLevelLength = 2u;   // a v1 page's level length prefix runs past the page
constexpr uint32_t kStValuesEnd = 4u;     // a PLAIN values section ends before the values the levels count
// status bits of the expanded encodings
constexpr uint32_t kStPastPage = 32u;     // a position past the page's raw_size
constexpr uint32_t kStWidth = 64u;        // DELTA_BINARY_PACKED: a miniblock's bit width above 64
constexpr uint32_t kStBlockSize = 128u;   // DELTA_BINARY_PACKED: illegal block / miniblock size
constexpr uint32_t kStCount = 256u;       // the values section holds more values than the page has rows
constexpr uint32_t kStLevels = 512u;      // the definition levels ask for more values than the section holds
constexpr uint32_t kStBssLength = 1024u;  // BYTE_STREAM_SPLIT: a section length that is no multiple of 8
constexpr uint32_t kStLevelsEnd = 2048u;  // the definition levels end before the page's rows do

// Header of a DELTA_BINARY_PACKED values section at src[*pos .. end).  0, or the status bit of what is wrong with it.
__device__ __forceinline__ uint32_t delta_header(const uint8_t *src, int64_t *pos, int64_t end, int64_t *vals_per_mini, int64_t *minis,
                                                 int64_t *total, uint64_t *first) {
    uint64_t bs, mpb, tot, fv;
    if (!rd_varint64(src, pos, end, &bs) || !rd_varint64(src, pos, end, &mpb) || !rd_varint64(src, pos, end, &tot) ||
        !rd_varint64(src, pos, end, &fv))
        return kStPastPage;
    // legal: block_size a positive multiple of 128, miniblocks_per_block > 0 dividing it, values per miniblock a multiple of 32.
    // (a page holds fewer than 2^31 values: a larger block is declined with the same bit, and the byte counts below cannot wrap)
    if (bs == 0 || (bs & 127) || bs > (1ull << 30) || mpb == 0 || bs % mpb || ((bs / mpb) & 31)) return kStBlockSize;
    *vals_per_mini = (int64_t)(bs / mpb);
    *minis = (int64_t)mpb;
    *total = tot > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)tot;
    *first = unzigzag64(fv);
    return 0;
}

// A page's definition levels (RLE / bit-packed hybrid, bit width 1) arrive as runs; rows are handled 2048 at a time (64 lanes x one
// 32-row word).  The walk's state between two trips of a wavefront:
struct LevelWalk {
    int64_t lpos = 0;        // read position in the level bytes
    int run_left = 0;        // levels left in the current run
    int run_kind = 0;        // 0: RLE, 1: bit-packed
    int run_val = 0;         // RLE value
    int64_t run_bits = 0;    // bit-packed: BIT position (from lv) of the run's next unread level
};

// The lane's validity word of one trip: rows [row + 32 * lane, + 32) of a page of nv rows, bit k = row k is not null.  A REQUIRED
// column gets all ones up to the page's rows.  Every lane walks the same runs (uniform), keeping the bits of its own word.
__device__ __forceinline__ uint32_t level_trip_word(int optional, const uint8_t *lv, int64_t lv_end, LevelWalk &W, int row, int nv, int lane,
                                                    uint32_t *status) {
    uint32_t word = 0;
    const int my0 = row + 32 * lane;
    if (!optional) {
        const int cnt = nv - my0;
        return cnt >= 32 ? 0xFFFFFFFFu : (cnt > 0 ? ((1u << cnt) - 1u) : 0u);
    }
    int pos = row;               // level index the walk has reached
    const int stop = row + 2048 < nv ? row + 2048 : nv;
    while (pos < stop) {
        if (W.run_left == 0) {
            if (W.lpos >= lv_end) { if (lane == 0) atomicOr(&status[0], kStLevelsEnd); break; }  // rows are left, levels are not
            const uint32_t h = rd_varint(lv, &W.lpos, lv_end);
            if (h & 1) { W.run_kind = 1; W.run_left = (int)(h >> 1) * 8; W.run_bits = W.lpos * 8; W.lpos += (h >> 1); }  // bit width 1: one byte per group of 8
            else { W.run_kind = 0; W.run_left = (int)(h >> 1); W.run_val = W.lpos < lv_end ? (lv[W.lpos] & 1) : 0; W.lpos += 1; }
            if (W.lpos > lv_end && lane == 0) atomicOr(&status[0], kStLevelsEnd);  // the run's own bytes lie past the levels
            if (W.run_left == 0) continue;
        }
        const int take = W.run_left < stop - pos ? W.run_left : stop - pos;
        // levels [pos, pos + take) come from this run; intersect with my word [my0, my0 + 32)
        const int a = pos > my0 ? pos : my0, b = (pos + take) < (my0 + 32) ? (pos + take) : (my0 + 32);
        if (a < b) {
            if (W.run_kind == 0) {
                if (W.run_val) word |= (b - a >= 32 ? 0xFFFFFFFFu : ((1u << (b - a)) - 1u)) << (a - my0);
            } else {
                for (int r = a; r < b; r++) {  // (at most 32 single-bit reads; LSB first, like Arrow validity)
                    const int64_t bit = W.run_bits + (r - pos);
                    const uint8_t byte = (bit >> 3) < lv_end ? lv[bit >> 3] : 0;
                    word |= (uint32_t)((byte >> (bit & 7)) & 1u) << (r - my0);
                }
            }
        }
        pos += take;
        W.run_left -= take;
        if (W.run_kind == 1) W.run_bits += take;
    }
    if (my0 < nv) { const int cnt = nv - my0; if (cnt < 32) word &= (1u << cnt) - 1u; }
    else word = 0;
    return word;
}

// Up to 32 bits at BIT position `bit` from p (any byte alignment), LSB first, by aligned 8-byte loads and a funnel shift.  The
// caller keeps byte bit / 8 inside the page; the loads reach at most 11 bytes past it (the buffers are padded by 16, as for PLAIN)
// and, the address being aligned DOWN to 8, up to 7 bytes in front of it.  The latter is safe because a page lies inside the
// uploaded chunk bytes or the Snappy scratch, both pool blocks of their own whose base is at least 8-byte aligned (an address is
// never aligned down past the block's base); a caller that hands in a sub-allocated buffer must keep its base 8-byte aligned too.
__device__ __forceinline__ uint32_t bits32_at(const uint8_t *p, int64_t bit) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p + (bit >> 3));
    const uint64_t *al = reinterpret_cast<const uint64_t *>(addr & ~(uintptr_t)7);
    const int shb = (int)(addr & 7) * 8 + (int)(bit & 7);
    uint64_t v = al[0] >> shb;
    if (shb > 32) v |= al[1] << (64 - shb);
    return (uint32_t)v;
}

__device__ __forceinline__ uint32_t low_mask32(int k) { return k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u); }

// `bits`, dense from bit 0, onto the set positions of `mask`, ascending; zeros elsewhere (a 32-bit pdep)
__device__ __forceinline__ uint32_t deposit32(uint32_t bits, uint32_t mask) {
    if (mask == 0xFFFFFFFFu) return bits;
    uint32_t r = 0;
    for (uint32_t m = mask; m; m &= m - 1u) {
        if (bits & 1u) r |= m & (0u - m);
        bits >>= 1;
    }
    return r;
}

}  // namespace

// status[0] |= 1: malformed Snappy stream / size mismatch
__global__ __launch_bounds__(256) void snappy_pages_kernel(const uint8_t *__restrict__ chunk, const PqPage *__restrict__ pages, int64_t npages,
                                                           uint8_t *raw, uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t pg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (!P.compressed) return;
    const uint8_t *src = chunk + P.src_off;
    uint8_t *dst = raw + P.raw_off;
    int64_t ip = 0;
    const int64_t iend = P.comp_size;
    const uint32_t ulen = rd_varint(src, &ip, iend);
    bool bad = ulen != (uint32_t)P.raw_size;
    int64_t op = 0;
    while (ip < iend && !bad) {
        const uint32_t tag = src[ip++];
        uint32_t len, off = 0;
        if ((tag & 3) == 0) {  // literal
            len = (tag >> 2) + 1;
            if (len > 60) {
                const int nb = (int)len - 60;
                if (ip + nb > iend) { bad = true; break; }
                uint32_t v = 0;
                for (int k = 0; k < nb; k++) v |= (uint32_t)src[ip + k] << (8 * k);
                ip += nb;
                len = v + 1;
            }
            if (ip + len > iend || op + len > P.raw_size) { bad = true; break; }
            for (uint32_t i = lane; i < len; i += 64) dst[op + i] = src[ip + i];
            ip += len;
        } else {
            if ((tag & 3) == 1) {
                if (ip + 1 > iend) { bad = true; break; }
                len = 4 + ((tag >> 2) & 7);
                off = ((tag >> 5) << 8) | src[ip];
                ip += 1;
            } else if ((tag & 3) == 2) {
                if (ip + 2 > iend) { bad = true; break; }
                len = (tag >> 2) + 1;
                off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8);
                ip += 2;
            } else {
                if (ip + 4 > iend) { bad = true; break; }
                len = (tag >> 2) + 1;
                off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8) | ((uint32_t)src[ip + 2] << 16) | ((uint32_t)src[ip + 3] << 24);
                ip += 4;
            }
            if (off == 0 || off > op || op + len > P.raw_size) { bad = true; break; }
            // earlier stores of this wavefront must be visible to the loads below.  Workgroup scope is enough (the lanes share
            // one vector L1, which its own write-through stores keep current); an agent-scope release would write the XCD's
            // L2 back on every element (measured: 400 ms per 160 MB column).
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const uint8_t *base = dst + op - off;
            for (uint32_t i = lane; i < len; i += 64) {
                const uint32_t j = off >= len ? i : i % off;
                dst[op + i] = base[j];
            }
        }
        op += len;
    }
    if (!bad && op != P.raw_size) bad = true;
    if (bad && lane == 0) atomicOr(&status[0], 1u);
}

// Dictionary-encoded data pages (PLAIN_DICTIONARY / RLE_DICTIONARY): after the definition levels comes one byte = bit width, then
// the RLE / bit-packed hybrid of dictionary indices, one per non-null value.  One wavefront per page expands it into a dense
// uint32 array (the lanes share every run: an RLE run is a fill, a bit-packed run one bit-field extraction per value).
// idx_counts[pg] = how many indices the page's stream gave (at most num_values): page_scatter_kernel looks up no index past it, so a
// stream that ends early is reported there (kStLevels) and never read from what an earlier call left in the index workspace.
__global__ __launch_bounds__(256) void dict_indices_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ chunk,
                                                           const PqPage *__restrict__ pages, int64_t npages,
                                                           int optional, uint32_t *indices, uint32_t *idx_counts, uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t pg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (P.kind != 1) return;
    const uint8_t *src = (P.compressed ? raw : chunk) + P.raw_off;  // a page's values: decompressed into the scratch buffer, or stored
    int64_t pos = 0;
    if (optional && !P.v2) {
        const uint32_t lbytes = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
        pos = 4 + (int64_t)lbytes;
    }
    if (pos >= P.raw_size) { if (lane == 0) idx_counts[pg] = 0; return; }  // a page of nulls only carries no index stream
    const int bw = src[pos++];
    if (bw > 32) { if (lane == 0) { idx_counts[pg] = 0; atomicOr(&status[0], 16u); } return; }
    const int vbytes = (bw + 7) >> 3;
    uint32_t *dst = indices + P.idx_off;
    int64_t outp = 0;
    const int64_t cap = P.num_values;  // at most one index per row
    while (pos < P.raw_size && outp < cap) {
        const uint32_t h = rd_varint(src, &pos, P.raw_size);
        if (h & 1) {  // bit-packed: (h >> 1) groups of 8 values, bw bits each, LSB first
            const int64_t count = (int64_t)(h >> 1) * 8;
            const int64_t nbytes = (int64_t)(h >> 1) * bw;
            if (pos + nbytes > P.raw_size + 8) { if (lane == 0) atomicOr(&status[0], 16u); break; }
            int64_t take = count < cap - outp ? count : cap - outp;
            // a last group may lack its padding bytes (some writers cut it); an index whose own bits lie past the page is not given
            if (bw) { const int64_t whole = (P.raw_size - pos) * 8 / bw; if (whole < take) take = whole; }
            for (int64_t j = lane; j < take; j += 64) {
                const int64_t bit = j * bw;
                const uint8_t *q = src + pos + (bit >> 3);
                uint64_t w = 0;
                for (int b = 0; b < 5; b++) w |= (pos + (bit >> 3) + b < P.raw_size ? (uint64_t)q[b] : 0ull) << (8 * b);
                dst[outp + j] = bw == 32 ? (uint32_t)(w >> (bit & 7)) : (uint32_t)((w >> (bit & 7)) & ((1ull << bw) - 1ull));
            }
            pos += nbytes;
            outp += take;
        } else {  // RLE: (h >> 1) copies of one value stored in ceil(bw / 8) bytes
            const int64_t count = h >> 1;
            if (count == 0 || pos + vbytes > P.raw_size) break;  // malformed: no progress / the run's value lies past the page
            uint32_t val = 0;
            for (int b = 0; b < vbytes; b++) val |= (uint32_t)src[pos + b] << (8 * b);
            pos += vbytes;
            const int64_t take = count < cap - outp ? count : cap - outp;
            for (int64_t j = lane; j < take; j += 64) dst[outp + j] = val;
            outp += take;
        }
    }
    if (lane == 0) idx_counts[pg] = (uint32_t)outp;
}

// DELTA_BINARY_PACKED data pages (INT64): <block size> <miniblocks per block> <total value count> <first value (zigzag)>, then per
// block <min delta (zigzag)> <one bit-width byte per miniblock> <miniblock bodies, LSB-first bit-packed>.  The last miniblock that
// holds values is padded to its full length; the ones after it keep their width byte and have no body.  value[i] = value[i - 1] +
// min_delta + delta[i] in wrapping 64-bit arithmetic.  One wavefront per page, every lane parses the same headers; a damaged page
// raises a status bit and the wavefront leaves it (every read lies below raw_size, every write inside the page's num_values slots).
__global__ __launch_bounds__(256) void delta_pages_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ chunk,
                                                          const PqPage *__restrict__ pages, int64_t npages, int optional,
                                                          uint64_t *expanded, uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t pg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (P.kind != 3) return;
    const uint8_t *src = (P.compressed ? raw : chunk) + P.raw_off;
    const int64_t end = P.raw_size;
    int64_t pos = values_offset(src, P, optional);
    if (pos < 0) { if (lane == 0) atomicOr(&status[0], kStLevelLength); return; }
    if (pos >= end) return;  // a page of nulls only may carry no values section
    int64_t V, mpb, total;
    uint64_t carry;
    uint32_t bad = delta_header(src, &pos, end, &V, &mpb, &total, &carry);
    if (!bad && total > (int64_t)P.num_values) bad = kStCount;
    if (bad) { if (lane == 0) atomicOr(&status[0], bad); return; }
    if (total == 0) return;
    uint64_t *dst = expanded + P.idx_off;
    if (lane == 0) dst[0] = carry;
    int64_t outp = 1;
    while (outp < total) {  // one block per trip: its first miniblock always takes at least one value
        uint64_t md;
        if (!rd_varint64(src, &pos, end, &md) || pos + mpb > end) { bad = kStPastPage; break; }
        const uint64_t min_delta = unzigzag64(md);
        const int64_t wpos = pos;
        pos += mpb;
        for (int64_t m = 0; m < mpb && outp < total; m++) {
            const int w = src[wpos + m];
            if (w > 64) { bad = kStWidth; break; }
            const int64_t nbytes = V * w >> 3;   // (V is a multiple of 32: whole bytes)
            if (pos + nbytes > end) { bad = kStPastPage; break; }
            const int64_t take = V < total - outp ? V : total - outp;
            for (int64_t j0 = 0; j0 < take; j0 += 64) {
                const int64_t j = j0 + lane;
                uint64_t d = 0;
                if (j < take) {
                    uint64_t v = 0;
                    if (w) {
                        // w bits at bit j * w of the body: they span up to 9 bytes, all below pos + nbytes <= raw_size.  Two aligned
                        // 8-byte loads cover 9 bytes from any byte offset (the buffers are padded by 16 bytes, like for PLAIN).
                        const int64_t bit = j * w;
                        const uintptr_t addr = reinterpret_cast<uintptr_t>(src + pos + (bit >> 3));
                        const uint64_t *al = reinterpret_cast<const uint64_t *>(addr & ~(uintptr_t)7);
                        const int shb = (int)(addr & 7) * 8 + (int)(bit & 7);
                        v = shb ? ((al[0] >> shb) | (al[1] << (64 - shb))) : al[0];
                        if (w < 64) v &= (1ull << w) - 1ull;
                    }
                    d = v + min_delta;
                }
                for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up((unsigned long long)d, o); if (lane >= o) d += y; }
                if (j < take) dst[outp + j] = carry + d;
                carry += (uint64_t)__shfl((unsigned long long)d, 63);   // (lanes past `take` added 0)
            }
            pos += nbytes;
            outp += take;
        }
        if (bad) break;
    }
    if (bad && lane == 0) atomicOr(&status[0], bad);
}

// BYTE_STREAM_SPLIT data pages (INT64 / DOUBLE): with N values in the page, byte k of value i lies at values[k * N + i].  Lane i
// assembles value i, so each of the eight streams is read in consecutive bytes across the wavefront and the dense array is written
// in consecutive 8-byte words (read from page_scatter_kernel instead, where a lane owns 32 consecutive rows, neighbouring lanes
// would sit ~32 bytes apart in every stream).
__global__ __launch_bounds__(256) void bss_pages_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ chunk,
                                                        const PqPage *__restrict__ pages, int64_t npages, int optional,
                                                        uint64_t *expanded, uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t pg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (P.kind != 4) return;
    const uint8_t *src = (P.compressed ? raw : chunk) + P.raw_off;
    const int64_t vpos = values_offset(src, P, optional);
    if (vpos < 0) { if (lane == 0) atomicOr(&status[0], kStLevelLength); return; }
    const int64_t len = P.raw_size - vpos;
    if (len <= 0) return;
    const int64_t N = len >> 3;
    if ((len & 7) || N > (int64_t)P.num_values) { if (lane == 0) atomicOr(&status[0], (len & 7) ? kStBssLength : kStCount); return; }
    const uint8_t *vals = src + vpos;
    uint64_t *dst = expanded + P.idx_off;
    for (int64_t i = lane; i < N; i += 64) {
        uint64_t v = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) v |= (uint64_t)vals[k * N + i] << (8 * k);
        dst[i] = v;
    }
}

// optional: column has definition levels (max level 1); out_valid must be zeroed; valid_count += non-null rows;
// expanded: the dense values of DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages (delta_pages_kernel / bss_pages_kernel)
__global__ __launch_bounds__(256) void page_scatter_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ chunk,
                                                           const PqPage *__restrict__ pages, int64_t npages,
                                                           int optional, const uint32_t *__restrict__ indices,
                                                           const uint32_t *__restrict__ idx_counts, const uint64_t *__restrict__ expanded,
                                                           uint64_t *out_values, uint32_t *out_valid,
                                                           unsigned long long *valid_count, uint32_t *status) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t pg = (int64_t)blockIdx.x * 4 + wv;
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (P.kind == 2) return;  // the dictionary page itself holds no rows
    const uint8_t *src = (P.compressed ? raw : chunk) + P.raw_off;
    const int nv = P.num_values;
    int64_t vpos = 0;  // offset of the PLAIN values inside the page
    const uint8_t *lv = nullptr;
    int64_t lv_end = 0;
    if (optional && P.v2) {  // levels sit uncompressed in the chunk, without a length prefix
        lv = chunk + P.lv_off;
        lv_end = P.lv_len;
    } else if (optional) {
        const uint32_t lbytes = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
        if ((int64_t)lbytes + 4 > P.raw_size) { if (lane == 0) atomicOr(&status[0], kStLevelLength); return; }
        lv = src + 4;
        lv_end = lbytes;
        vpos = 4 + (int64_t)lbytes;
    }
    const uint8_t *vals = src + vpos;
    const int64_t val_bytes = P.raw_size - vpos;
    unsigned long long page_valid = 0;
    // kind 3 / 4: how many values the page's section holds (what delta_pages_kernel / bss_pages_kernel expanded, never more than nv)
    int64_t xcount = 0;
    if (P.kind == 4) {
        xcount = val_bytes > 0 ? val_bytes >> 3 : 0;
    } else if (P.kind == 3 && vpos < P.raw_size) {
        int64_t hp = vpos, V, mpb;
        uint64_t first;
        if (delta_header(src, &hp, P.raw_size, &V, &mpb, &xcount, &first)) xcount = 0;  // (the status bit is delta_pages_kernel's)
    }
    if (xcount > nv) xcount = nv;
    const int64_t icount = P.kind == 1 ? (int64_t)idx_counts[pg] : 0;  // kind 1: how many indices dict_indices_kernel gave

    LevelWalk walk;          // the levels arrive as runs; rows are handled 2048 at a time (64 lanes x one 32-row word)
    int64_t vidx_base = 0;   // values consumed so far
    for (int row = 0; row < nv; row += 2048) {
        const int my0 = row + 32 * lane;
        const uint32_t word = level_trip_word(optional, lv, lv_end, walk, row, nv, lane, status);
        // value index of my word's first value: scan of the popcounts
        const int pc = __popc(word);
        int inc = pc;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o); if (lane >= o) inc += y; }
        const int total = __shfl(inc, 63);
        int64_t vi = vidx_base + inc - pc;
        if (my0 < nv) {
            const int64_t orow = P.row0 + my0;
            const int cnt = nv - my0 < 32 ? nv - my0 : 32;
            for (int k = 0; k < cnt; k++) {
                uint64_t v = 0;
                if ((word >> k) & 1u) {
                    if (P.kind == 1) {  // the vi-th index of the page (expanded by dict_indices_kernel) -> the chunk's dictionary
                        const uint32_t ix = vi < icount ? indices[P.idx_off + vi] : 0u;
                        if (vi >= icount) {
                            atomicOr(&status[0], kStLevels);
                        } else if (ix < (uint32_t)P.dict_count) {
                            const uintptr_t addr = reinterpret_cast<uintptr_t>((P.dict_in_raw ? raw : chunk) + P.dict_off + (int64_t)ix * 8);  // (a stored dictionary sits at any byte offset)
                            const uint64_t *al = reinterpret_cast<const uint64_t *>(addr & ~(uintptr_t)7);
                            const int shb = (int)(addr & 7) * 8;
                            v = shb ? ((al[0] >> shb) | (al[1] << (64 - shb))) : al[0];
                        } else {
                            atomicOr(&status[0], 8u);
                        }
                    } else if (P.kind >= 3) {  // the vi-th value of the page, expanded; vi < nv always, so the slot is the page's own
                        if (vi < xcount) v = expanded[P.idx_off + vi];
                        else atomicOr(&status[0], kStLevels);
                    } else if ((vi + 1) * 8 <= val_bytes) {
                        // PLAIN: 8 little-endian bytes at any byte offset inside the page: two aligned loads + funnel shift
                        // (the buffers are padded by 16 bytes, so the second load never leaves them)
                        const uintptr_t addr = reinterpret_cast<uintptr_t>(vals + vi * 8);
                        const uint64_t *al = reinterpret_cast<const uint64_t *>(addr & ~(uintptr_t)7);
                        const int shb = (int)(addr & 7) * 8;
                        v = shb ? ((al[0] >> shb) | (al[1] << (64 - shb))) : al[0];
                    } else {
                        atomicOr(&status[0], kStValuesEnd);
                    }
                    vi++;
                }
                out_values[orow + k] = v;
            }
            // validity bits of rows [orow, orow + cnt): the page's first row is anywhere inside a word
            const int sh = (int)(orow & 31);
            const int64_t w = orow >> 5;
            if (word) {
                atomicOr(&out_valid[w], word << sh);
                if (sh && (word >> (32 - sh))) atomicOr(&out_valid[w + 1], word >> (32 - sh));
            }
        }
        vidx_base += total;
        page_valid += total;
    }
    if (lane == 0 && page_valid) atomicAdd(valid_count, page_valid);
}

// Data pages of a BOOLEAN column (kind 5: PLAIN, kind 6: RLE) -> Arrow value bits and validity bits; both bitmaps must be zeroed.
// A trip covers 2048 rows, a lane one 32-row word of them: validity word from the levels, popcount + exclusive wave scan = index vi of
// the lane's first value, the dense bits [vi, vi + popcount) of the values section, deposited onto the word's set positions.
//   PLAIN  a bit-field at bit vi of the section.
//   RLE    <4-byte length> <hybrid, bit width 1>: every lane walks the same value runs over the trip's value range (uniform, the run
//          state carries across trips like the level walk's) and keeps the intersection with its own range: an RLE run is a mask
//          fill, a bit-packed run a bit-field.  A bit-packed run is whole groups of 8: what its last group holds past the page's
//          values is never reached, because a trip asks for exactly the values its levels count.
// A page's first row lies anywhere inside an output word and pages of other wavefronts meet it there: a word the lane does not own
// alone is combined with atomicOr, one it owns (row0 a multiple of 32, 32 rows) is stored whole.  A damaged page raises a status bit
// and the wavefront leaves it; every read lies below raw_size (+ the padding bits32_at names), every write inside the page's rows.
__global__ __launch_bounds__(256) void bool_pages_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ chunk,
                                                         const PqPage *__restrict__ pages, int64_t npages, int optional,
                                                         uint32_t *out_bits, uint32_t *out_valid, unsigned long long *valid_count,
                                                         uint32_t *status) {
    const int lane = threadIdx.x & 63;
    const int64_t pg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pg >= npages) return;
    const PqPage P = pages[pg];
    if (P.kind != 5 && P.kind != 6) return;
    const uint8_t *src = (P.compressed ? raw : chunk) + P.raw_off;
    const int nv = P.num_values;
    const int64_t vpos = values_offset(src, P, optional);
    if (vpos < 0) { if (lane == 0) atomicOr(&status[0], kStLevelLength); return; }
    const uint8_t *lv = nullptr;
    int64_t lv_end = 0;
    if (optional && P.v2) { lv = chunk + P.lv_off; lv_end = P.lv_len; }   // (uncompressed in the chunk, without a length prefix)
    else if (optional) { lv = src + 4; lv_end = vpos - 4; }
    // the value bits: PLAIN [vpos, raw_size); RLE [vpos + 4, vpos + 4 + length).  A section too short for its length prefix is one
    // without values (a page of nulls only may carry none)
    int64_t vbeg = vpos, vend = P.raw_size;
    if (P.kind == 6) {
        if (vend - vpos >= 4) {
            const uint32_t rl = (uint32_t)src[vpos] | ((uint32_t)src[vpos + 1] << 8) | ((uint32_t)src[vpos + 2] << 16) | ((uint32_t)src[vpos + 3] << 24);
            if ((int64_t)rl + 4 > vend - vpos) { if (lane == 0) atomicOr(&status[0], kStPastPage); return; }
            vbeg = vpos + 4;
            vend = vbeg + (int64_t)rl;
        } else {
            vend = vbeg;
        }
    }
    int64_t rpos = vbeg;     // RLE: read position in the page's bytes
    int64_t vrun_left = 0;   //      values left in the current run
    int vrun_kind = 0;       //      0: RLE, 1: bit-packed
    int vrun_val = 0;        //      RLE value
    int64_t vrun_bits = 0;   //      bit-packed: BIT position (from src) of the run's next unread value
    LevelWalk walk;
    int64_t vidx_base = 0;   // values consumed so far
    unsigned long long page_valid = 0;
    for (int row = 0; row < nv; row += 2048) {
        const int my0 = row + 32 * lane;
        const uint32_t word = level_trip_word(optional, lv, lv_end, walk, row, nv, lane, status);
        const int pc = __popc(word);
        const int inc = (int)wave_inclusive_scan((uint32_t)pc, lane);
        const int total = __shfl(inc, 63);
        const int64_t vi = vidx_base + inc - pc;
        uint32_t dense = 0;
        if (P.kind == 5) {
            if (((vidx_base + total + 7) >> 3) > vend - vbeg) { if (lane == 0) atomicOr(&status[0], kStValuesEnd); return; }  // the section ends before the values do
            if (pc) dense = bits32_at(src + vbeg, vi) & low_mask32(pc);
        } else {
            int64_t vp = vidx_base;
            const int64_t vstop = vidx_base + total;
            while (vp < vstop) {
                if (vrun_left == 0) {
                    if (rpos >= vend) { if (lane == 0) atomicOr(&status[0], kStLevels); return; }  // values are left, runs are not
                    const uint32_t h = rd_varint(src, &rpos, vend);
                    if (h & 1) { vrun_kind = 1; vrun_left = (int64_t)(h >> 1) * 8; vrun_bits = rpos * 8; rpos += (h >> 1); }
                    else { vrun_kind = 0; vrun_left = (int64_t)(h >> 1); vrun_val = rpos < vend ? (src[rpos] & 1) : 0; rpos += 1; }
                    if (rpos > vend) { if (lane == 0) atomicOr(&status[0], kStPastPage); return; }  // the run's own bytes lie past the section
                    if (vrun_left == 0) continue;   // (a zero-length run: its header is consumed, so the walk moves on)
                }
                const int64_t take = vrun_left < vstop - vp ? vrun_left : vstop - vp;
                // values [vp, vp + take) come from this run; intersect with mine [vi, vi + pc)
                const int64_t a = vp > vi ? vp : vi, b = (vp + take) < (vi + pc) ? (vp + take) : (vi + pc);
                if (a < b) {
                    const uint32_t m = low_mask32((int)(b - a));
                    if (vrun_kind == 0) { if (vrun_val) dense |= m << (a - vi); }
                    else dense |= (bits32_at(src, vrun_bits + (a - vp)) & m) << (a - vi);   // (its bytes lie below rpos <= vend)
                }
                vp += take;
                vrun_left -= take;
                if (vrun_kind == 1) vrun_bits += take;
            }
        }
        if (my0 < nv && word) {
            const uint32_t bits = deposit32(dense, word);
            const int64_t orow = P.row0 + my0;
            const int sh = (int)(orow & 31);
            const int64_t w = orow >> 5;
            if (sh == 0 && nv - my0 >= 32) {
                out_valid[w] = word;
                out_bits[w] = bits;
            } else {
                atomicOr(&out_valid[w], word << sh);
                if (bits << sh) atomicOr(&out_bits[w], bits << sh);
                if (sh && (word >> (32 - sh))) atomicOr(&out_valid[w + 1], word >> (32 - sh));
                if (sh && (bits >> (32 - sh))) atomicOr(&out_bits[w + 1], bits >> (32 - sh));
            }
        }
        vidx_base += total;
        page_valid += total;
    }
    if (lane == 0 && page_valid) atomicAdd(valid_count, page_valid);
}

// the pages of a BOOLEAN column (behind the same Snappy pass): out_bits and out_valid are zeroed by the caller
int launch_parquet_bool_decode(Ctx *c, const uint8_t *chunk, const PqPage *pages, int64_t npages, bool any_compressed, uint8_t *raw,
                               int optional, uint32_t *out_bits, uint32_t *out_valid, unsigned long long *valid_count, uint32_t *status) {
    if (npages <= 0) return 0;
    const unsigned grid = (unsigned)((npages + 3) / 4);
    if (any_compressed) hipLaunchKernelGGL(snappy_pages_kernel, dim3(grid), dim3(256), 0, c->stream, chunk, pages, npages, raw, status);
    hipLaunchKernelGGL(bool_pages_kernel, dim3(grid), dim3(256), 0, c->stream, raw, chunk, pages, npages, optional, out_bits, out_valid,
                       valid_count, status);
    BG_HIP(hipGetLastError());
    return 0;
}

int launch_parquet_decode(Ctx *c, const uint8_t *chunk, const PqPage *pages, int64_t npages, bool any_compressed, uint8_t *raw,
                          int optional, uint32_t kinds, uint32_t *indices, uint32_t *idx_counts, uint64_t *expanded, uint64_t *out_values,
                          uint32_t *out_valid, unsigned long long *valid_count, uint32_t *status) {  // kinds: bit k set = some page has PqPage.kind k
    if (npages <= 0) return 0;
    const unsigned grid = (unsigned)((npages + 3) / 4);
    if (any_compressed) hipLaunchKernelGGL(snappy_pages_kernel, dim3(grid), dim3(256), 0, c->stream, chunk, pages, npages, raw, status);
    if (kinds & 2u) hipLaunchKernelGGL(dict_indices_kernel, dim3(grid), dim3(256), 0, c->stream, raw, chunk, pages, npages, optional, indices, idx_counts, status);
    if (kinds & 8u) hipLaunchKernelGGL(delta_pages_kernel, dim3(grid), dim3(256), 0, c->stream, raw, chunk, pages, npages, optional, expanded, status);
    if (kinds & 16u) hipLaunchKernelGGL(bss_pages_kernel, dim3(grid), dim3(256), 0, c->stream, raw, chunk, pages, npages, optional, expanded, status);
    hipLaunchKernelGGL(page_scatter_kernel, dim3(grid), dim3(256), 0, c->stream, raw, chunk, pages, npages, optional, indices, idx_counts,
                       expanded, out_values, out_valid, valid_count, status);
    BG_HIP(hipGetLastError());
    return 0;
}

}  // namespace bowgpu
