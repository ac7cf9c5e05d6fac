// parquet_write.cpp — host side of the device -> Parquet writer (the reference's Bow.WriteParquet, bowparquet.go:157-253, minus
// its codec): a Thrift compact WRITER for the page headers and the footer (restated from the Parquet format specification), the
// assembly of the file from the page tables and the level / value images that pq_finish_chunk (parquet_encode.hip; declared, like
// the two chunk drivers called here, in parquet_encode.h) leaves in host memory, and the entry points bowgpu_parquet_write / _codec / _bool.  The assembly
// (PqWriter) is plain C++ over host buffers and touches no device and nothing else of the library; with
// BOWGPU_PARQUET_ASSEMBLE_ONLY defined this file is that alone (tests/cpp/test_parquet_assemble.cpp).
//
// The file: format version 1, root `Schema`, every column OPTIONAL (bowparquet.go:190), INT64 / DOUBLE / BOOLEAN, UNCOMPRESSED,
// data page v1, definition levels as RLE / bit-packed hybrid of bit width 1, PLAIN, DELTA_BINARY_PACKED or RLE_DICTIONARY values (the last
// behind the chunk's dictionary page, whose entries parquet_dict.hip finds and the host orders).  With codec SNAPPY
// (bowgpu_parquet_write_codec; the reference's codec, bowparquet.go:326-338) a page's section is one raw Snappy stream of
// [4-byte levels length | levels | values]: the preamble and the levels literal are written here, the values' elements come from
// snappy_encode.hip as they lie.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <exception>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "parquet_write.h"

namespace bowgpu {

namespace {

// ---------------------------------------------------------------- Thrift compact protocol (write side)
struct TWriter {
    std::vector<uint8_t> b;
    std::vector<int16_t> stack;   // field id last written in each enclosing struct
    int16_t last = 0;
    void byte(uint8_t v) { b.push_back(v); }
    void varint(uint64_t v) {
        while (v >= 0x80) { byte((uint8_t)(v | 0x80)); v >>= 7; }
        byte((uint8_t)v);
    }
    void zigzag(int64_t v) { varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
    void field(int16_t fid, int type) {
        const int d = fid - last;
        if (d > 0 && d < 16) byte((uint8_t)((d << 4) | type));
        else { byte((uint8_t)type); zigzag(fid); }
        last = fid;
    }
    void i32(int16_t fid, int32_t v) { field(fid, 5); zigzag(v); }
    void i64(int16_t fid, int64_t v) { field(fid, 6); zigzag(v); }
    void binary(int16_t fid, const void *p, size_t n) {
        field(fid, 8);
        varint(n);
        b.insert(b.end(), reinterpret_cast<const uint8_t *>(p), reinterpret_cast<const uint8_t *>(p) + n);
    }
    void string(int16_t fid, const std::string &s) { binary(fid, s.data(), s.size()); }
    void list(int16_t fid, int etype, size_t n) {
        field(fid, 9);
        if (n < 15) byte((uint8_t)((n << 4) | etype));
        else { byte((uint8_t)(0xF0 | etype)); varint(n); }
    }
    void open_struct() { stack.push_back(last); last = 0; }                 // a list element, or the top level
    void open_struct(int16_t fid) { field(fid, 12); open_struct(); }        // a field
    void close_struct() { byte(0); last = stack.back(); stack.pop_back(); }
};

// definition levels of one v1 page, max level 1: one RLE run where every row says the same, else one bit-packed run over the
// page's validity bits
void put_levels(std::vector<uint8_t> *out, const PqwPage &pg) {
    TWriter w;
    if (pg.valid == pg.rows || pg.valid == 0) {
        w.varint((uint64_t)pg.rows << 1);
        w.byte(pg.valid ? 1 : 0);
    } else {
        const uint64_t groups = ((uint64_t)pg.rows + 7) >> 3;
        w.varint((groups << 1) | 1);
        w.b.insert(w.b.end(), pg.level_bits, pg.level_bits + groups);
    }
    const uint32_t len = (uint32_t)w.b.size();
    for (int k = 0; k < 4; k++) out->push_back((uint8_t)(len >> (8 * k)));
    out->insert(out->end(), w.b.begin(), w.b.end());
}

// the tag of a Snappy literal element of n bytes, 1 <= n <= 2^24: the length in the tag itself, or in the 1 to 3 bytes behind it
void put_literal_tag(TWriter *s, size_t n) {
    if (n <= 60) { s->byte((uint8_t)((n - 1) << 2)); return; }
    const int k = n <= 256 ? 1 : n <= 65536 ? 2 : 3;
    s->byte((uint8_t)((59 + k) << 2));
    for (int j = 0; j < k; j++) s->byte((uint8_t)((n - 1) >> (8 * j)));
}

// a page's Thrift header; type 2: the DICTIONARY_PAGE of num_values entries, type 0: the v1 DATA_PAGE of num_values rows
std::vector<uint8_t> page_header(int32_t type, int64_t raw, int64_t comp, int32_t num_values, int32_t encoding) {
    TWriter w;
    w.open_struct();
    w.i32(1, type);
    w.i32(2, (int32_t)raw);       // uncompressed_page_size
    w.i32(3, (int32_t)comp);      // compressed_page_size
    w.open_struct(type == 2 ? 7 : 5);   // DictionaryPageHeader / DataPageHeader
    w.i32(1, num_values);         //   of a data page: rows, nulls included
    w.i32(2, encoding);
    if (type == 0) { w.i32(3, 3); w.i32(4, 3); }   //   definition levels: RLE; repetition levels: RLE (there are none)
    w.close_struct();
    w.close_struct();
    return w.b;
}

constexpr size_t kBufBytes = 1u << 20;   // what put() gathers before it writes; longer pieces go out as they lie

}  // namespace

PqWriter::~PqWriter() { drop(); }

void PqWriter::drop() {
    if (fd_ >= 0) {
        close(fd_);
        fd_ = -1;
        unlink(tmp_.c_str());
    }
}

int PqWriter::sys_fail(const char *what) {
    err_ = std::string("parquet: cannot ") + what + " '" + tmp_ + "': " + strerror(errno);
    drop();
    return -1;
}

int PqWriter::flush() {
    size_t done = 0;
    while (done < buf_.size()) {
        const ssize_t k = write(fd_, buf_.data() + done, buf_.size() - done);
        if (k < 0) { if (errno == EINTR) continue; return sys_fail("write"); }
        done += (size_t)k;
    }
    buf_.clear();
    return 0;
}

int PqWriter::put(const void *p, size_t n) {
    if (fd_ < 0) { if (err_.empty()) err_ = "parquet: the writer is not open"; return -1; }
    pos_ += (int64_t)n;
    if (n < kBufBytes / 4) {
        if (buf_.size() + n > kBufBytes && flush() != 0) return -1;
        buf_.insert(buf_.end(), reinterpret_cast<const uint8_t *>(p), reinterpret_cast<const uint8_t *>(p) + n);
        return 0;
    }
    if (flush() != 0) return -1;
    const uint8_t *s = reinterpret_cast<const uint8_t *>(p);
    while (n > 0) {
        const ssize_t k = write(fd_, s, n);
        if (k < 0) { if (errno == EINTR) continue; return sys_fail("write"); }
        s += k;
        n -= (size_t)k;
    }
    return 0;
}

int PqWriter::open(const char *path, const char *const *names, const int32_t *types, int32_t ncols, bool statistics, const char *const *meta_keys,
                   const char *const *meta_values, int32_t n_meta) {
    path_ = path;
    tmp_ = path_ + ".tmp";
    stats_ = statistics;
    for (int i = 0; i < ncols; i++) { names_.push_back(names[i]); types_.push_back(types[i]); }
    for (int i = 0; i < n_meta; i++) { meta_k_.push_back(meta_keys[i]); meta_v_.push_back(meta_values[i] ? meta_values[i] : ""); }
    fd_ = ::open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd_ < 0) {
        err_ = "parquet: cannot create '" + tmp_ + "': " + strerror(errno);
        return -1;
    }
    buf_.reserve(kBufBytes);
    return put("PAR1", 4);
}

int PqWriter::begin_row_group(int64_t rows) {
    groups_.push_back(Group{rows, 0, {}});
    return 0;
}

int PqWriter::add_chunk(int32_t encoding, const PqwPage *pages, int64_t npages, const PqwStats &stats, int32_t codec, const uint64_t *dict, int64_t ndict) {
    if (codec != kPqUncompressed && codec != kPqSnappy) { err_ = "parquet: the writer has no codec " + std::to_string(codec); drop(); return -1; }
    if ((encoding == kPqEncRleDict) != (dict != nullptr && ndict > 0) || ndict > ((int64_t)1 << 27)) {
        err_ = "parquet: a dictionary of " + std::to_string(ndict) + " entries with value encoding " + std::to_string(encoding);
        drop();
        return -1;
    }
    Group &g = groups_.back();
    Chunk ch{encoding, codec, pos_, pos_, 0, 0, 0, stats};
    std::vector<uint8_t> head;
    if (encoding == kPqEncRleDict) {   // the dictionary page: PLAIN entries; kPqSnappy: the preamble and literal elements of at most 64 KiB
        const uint8_t *body = reinterpret_cast<const uint8_t *>(dict);
        const int64_t raw = 8 * ndict;
        TWriter s;
        if (codec == kPqSnappy) {
            s.varint((uint64_t)raw);
            for (int64_t at = 0; at < raw; at += 65536) {
                const size_t n = (size_t)(raw - at < 65536 ? raw - at : 65536);   // a multiple of 8
                put_literal_tag(&s, n);
                s.b.insert(s.b.end(), body + at, body + at + n);
            }
        }
        const int64_t comp = codec == kPqSnappy ? (int64_t)s.b.size() : raw;
        head = page_header(2, raw, comp, (int32_t)ndict, kPqEncPlain);
        if (put(head.data(), head.size()) != 0) return -1;
        if (codec == kPqSnappy ? put(s.b.data(), s.b.size()) != 0 : put(body, (size_t)raw) != 0) return -1;
        ch.raw += (int64_t)head.size() + raw;
        ch.data_offset = pos_;
        tot_.value_bytes += raw;
    }
    for (int64_t p = 0; p < npages; p++) {
        const PqwPage &pg = pages[p];
        std::vector<uint8_t> lv;
        put_levels(&lv, pg);
        const int64_t body = (int64_t)lv.size() + pg.value_bytes;
        const uint8_t *values = pg.values;
        int64_t value_bytes = pg.value_bytes;
        if (codec == kPqSnappy) {   // the preamble and the levels section as a literal in front of it; the values' stream follows
            TWriter s;
            s.varint((uint64_t)body);
            const size_t n = lv.size();   // 4 + a run header + at most 128 KiB of bits: the 3-byte length form at the most
            if (n - 1 >= (1u << 24)) { err_ = "parquet: a page's levels section of " + std::to_string(n) + " bytes does not fit a literal"; drop(); return -1; }
            put_literal_tag(&s, n);
            s.b.insert(s.b.end(), lv.begin(), lv.end());
            lv.swap(s.b);
            values = pg.comp;
            value_bytes = pg.comp_bytes;
        }
        head = page_header(0, body, (int64_t)lv.size() + value_bytes, pg.rows, encoding);
        ch.raw += (int64_t)head.size() + body;
        head.insert(head.end(), lv.begin(), lv.end());
        if (put(head.data(), head.size()) != 0) return -1;
        if (value_bytes > 0 && put(values, (size_t)value_bytes) != 0) return -1;
        ch.values += pg.rows;
        tot_.level_bytes += body - pg.value_bytes;
        tot_.value_bytes += pg.value_bytes;
    }
    tot_.data_pages += npages;
    ch.bytes = pos_ - ch.offset;
    g.bytes += ch.raw;
    g.chunks.push_back(ch);
    return 0;
}

int PqWriter::end_row_group() {
    const Group &g = groups_.back();
    if (g.chunks.size() != names_.size()) { err_ = "parquet: a row group lacks column chunks"; drop(); return -1; }
    tot_.rows += g.rows;
    tot_.row_groups++;
    return 0;
}

int PqWriter::finish(PqwTotals *totals) {
    TWriter w;
    w.open_struct();
    w.i32(1, 1);   // version
    w.list(2, 12, names_.size() + 1);
    w.open_struct();
    w.string(4, "Schema");
    w.i32(5, (int32_t)names_.size());
    w.close_struct();
    for (size_t i = 0; i < names_.size(); i++) {
        w.open_struct();
        w.i32(1, types_[i]);
        w.i32(3, 1);   // OPTIONAL
        w.string(4, names_[i]);
        w.close_struct();
    }
    w.i64(3, tot_.rows);
    w.list(4, 12, groups_.size());
    for (const Group &g : groups_) {
        w.open_struct();
        w.list(1, 12, g.chunks.size());
        for (size_t i = 0; i < g.chunks.size(); i++) {
            const Chunk &ch = g.chunks[i];
            w.open_struct();              // ColumnChunk
            w.i64(2, ch.offset);          //   file_offset
            w.open_struct(3);             //   ColumnMetaData
            w.i32(1, types_[i]);
            const bool dict = ch.encoding == kPqEncRleDict;
            w.list(2, 5, dict ? 3 : 2);   //   encodings: the values' (and PLAIN for a dictionary page), and RLE for the levels
            w.zigzag(ch.encoding);
            if (dict) w.zigzag(kPqEncPlain);
            w.zigzag(3);
            w.list(3, 8, 1);              //   path_in_schema
            w.varint(names_[i].size());
            w.b.insert(w.b.end(), names_[i].begin(), names_[i].end());
            w.i32(4, ch.codec);           //   UNCOMPRESSED / SNAPPY
            w.i64(5, ch.values);
            w.i64(6, ch.raw);             //   total_uncompressed_size, total_compressed_size: the page headers count in both
            w.i64(7, ch.bytes);
            w.i64(9, ch.data_offset);     //   data_page_offset
            if (dict) w.i64(11, ch.offset);   // dictionary_page_offset
            w.open_struct(12);            //   Statistics
            w.i64(3, ch.stats.null_count);
            if (stats_ && ch.stats.has_minmax) {
                const size_t sb = types_[i] == kPqBoolean ? 1 : 8;   // (the low byte of the payload comes first)
                w.binary(5, &ch.stats.max, sb);   // max_value / min_value: PLAIN little-endian, TYPE_DEFINED_ORDER
                w.binary(6, &ch.stats.min, sb);
            }
            w.close_struct();
            w.close_struct();
            w.close_struct();
        }
        w.i64(2, g.bytes);
        w.i64(3, g.rows);
        w.close_struct();
    }
    if (!meta_k_.empty()) {
        w.list(5, 12, meta_k_.size());
        for (size_t i = 0; i < meta_k_.size(); i++) {
            w.open_struct();
            w.string(1, meta_k_[i]);
            w.string(2, meta_v_[i]);
            w.close_struct();
        }
    }
    w.string(6, "bowgpu (libbowgpu.so, bowgpu_parquet_write)");
    if (stats_) {
        w.list(7, 12, names_.size());
        for (size_t i = 0; i < names_.size(); i++) {
            w.open_struct();      // ColumnOrder (a union)
            w.open_struct(1);     //   TYPE_ORDER: TypeDefinedOrder, an empty struct
            w.close_struct();
            w.close_struct();
        }
    }
    w.close_struct();
    const uint32_t flen = (uint32_t)w.b.size();
    uint8_t tail[8] = {(uint8_t)flen, (uint8_t)(flen >> 8), (uint8_t)(flen >> 16), (uint8_t)(flen >> 24), 'P', 'A', 'R', '1'};
    if (put(w.b.data(), w.b.size()) != 0 || put(tail, 8) != 0 || flush() != 0) return -1;
    if (close(fd_) != 0) { fd_ = -1; unlink(tmp_.c_str()); err_ = "parquet: cannot close '" + tmp_ + "': " + strerror(errno); return -1; }
    fd_ = -1;
    if (rename(tmp_.c_str(), path_.c_str()) != 0) {
        err_ = "parquet: cannot rename '" + tmp_ + "' to '" + path_ + "': " + strerror(errno);
        unlink(tmp_.c_str());
        return -1;
    }
    tot_.file_bytes = pos_;
    if (totals) *totals = tot_;
    return 0;
}

}  // namespace bowgpu

#ifndef BOWGPU_PARQUET_ASSEMBLE_ONLY
// ---------------------------------------------------------------- bowgpu_parquet_write
#include "parquet_encode.h"

using namespace bowgpu;

namespace {

constexpr int64_t kWriteMaxRows = ((int64_t)1 << 31) - 1;

struct WritePlan { int64_t n, rg_rows; int32_t page_rows; bool statistics; std::vector<int32_t> enc, types; };

// everything that can be said about the call without a device or the file system; booleans: Boolean columns are admitted
// (bowgpu_parquet_write_bool) - the older entry points decline them with the text they always had
int write_checks(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols, const bowgpu_parquet_write_options *o, bool booleans,
                 WritePlan *p) {
    if (!path || !path[0] || !cols || !names) return fail(BOWGPU_ERR_ARG, "null argument");
    if (ncols < 1) return fail(BOWGPU_ERR_ARG, "parquet: a file needs at least one column (ncols = %d)", ncols);
    if (o && o->reserved != 0) return fail(BOWGPU_ERR_ARG, "parquet: bowgpu_parquet_write_options.reserved must be 0");
    p->page_rows = o && o->page_rows ? o->page_rows : 65536;
    p->rg_rows = o && o->row_group_rows ? o->row_group_rows : (int64_t)1 << 24;
    p->statistics = o ? o->statistics != 0 : true;
    if (p->page_rows < 64 || p->page_rows % 64 != 0 || p->page_rows > (1 << 20))
        return fail(BOWGPU_ERR_ARG, "parquet: page_rows %d is not a multiple of 64 in [64, 1048576]", p->page_rows);
    if (p->rg_rows < p->page_rows || p->rg_rows % p->page_rows != 0 || p->rg_rows > ((int64_t)1 << 27))
        return fail(BOWGPU_ERR_ARG, "parquet: row_group_rows %lld is not a multiple of page_rows %d of at most 134217728", (long long)p->rg_rows, p->page_rows);
    if (o && (o->n_meta < 0 || (o->n_meta > 0 && (!o->meta_keys || !o->meta_values)))) return fail(BOWGPU_ERR_ARG, "parquet: key / value metadata without its arrays");
    if (o) for (int i = 0; i < o->n_meta; i++) if (!o->meta_keys[i]) return fail(BOWGPU_ERR_ARG, "parquet: metadata key %d is NULL", i);
    p->n = cols[0].length;
    std::set<std::string> seen;
    for (int i = 0; i < ncols; i++) {
        const bowgpu_col &col = cols[i];
        const bool is_bool = booleans && col.type == BOWGPU_BOOLEAN;
        if (!movable_type(col.type) && !is_bool)
            return fail(BOWGPU_ERR_UNSUPPORTED, booleans ? "parquet: column %d is of unsupported type (Int64 / Float64 / Boolean are written)"
                                                         : "parquet: column %d is of unsupported type (Int64 / Float64 are written)", i);
        if (col.length < 0 || col.offset < 0) return fail(BOWGPU_ERR_ARG, "negative column length/offset");
        if (col.length != p->n) return fail(BOWGPU_ERR_ARG, "columns differ in length");
        if (!residency_ok(col.residency)) return fail(BOWGPU_ERR_ARG, "unknown residency %d", col.residency);
        if (col.length > 0 && !col.values) return fail(BOWGPU_ERR_ARG, "column has no values buffer");
        if (!names[i] || !names[i][0]) return fail(BOWGPU_ERR_ARG, "parquet: column %d has no name", i);
        if (!seen.insert(names[i]).second) return fail(BOWGPU_ERR_ARG, "parquet: two columns are named '%s'", names[i]);
        const int32_t e = o && o->encodings ? o->encodings[i] : kPqEncPlain;
        if (is_bool && e != kPqEncPlain)
            return fail(BOWGPU_ERR_UNSUPPORTED, "parquet: value encoding %d for the Boolean column '%s' (PLAIN = 0 is written; RLE value runs are not)", e, names[i]);
        if (e != kPqEncPlain && e != kPqEncDelta && e != kPqEncRleDict)
            return fail(BOWGPU_ERR_UNSUPPORTED, "parquet: value encoding %d for column '%s' (PLAIN = 0, DELTA_BINARY_PACKED = 5 and RLE_DICTIONARY = 8 are written)", e, names[i]);
        if (e == kPqEncDelta && col.type != BOWGPU_INT64) return fail(BOWGPU_ERR_UNSUPPORTED, "parquet: DELTA_BINARY_PACKED on the Float64 column '%s' (it is written for Int64 columns)", names[i]);
        p->enc.push_back(e);
        p->types.push_back(is_bool ? kPqBoolean : col.type == BOWGPU_INT64 ? kPqInt64 : kPqDouble);
    }
    if (p->n > kWriteMaxRows) return fail(BOWGPU_ERR_UNSUPPORTED, "the frame has %lld rows: the writer serves up to 2^31 - 1 = 2147483647 rows", (long long)p->n);
    return 0;
}

int writer_fail(const PqWriter &w) { return fail(BOWGPU_ERR_ARG, "%s", w.error().c_str()); }

int write_impl(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols, const bowgpu_parquet_write_options *o, int32_t codec,
               bool booleans, bowgpu_parquet_write_info *info) {
    WritePlan plan;
    BG_TRY(write_checks(path, cols, names, ncols, o, booleans, &plan));
    if (codec != kPqUncompressed && codec != kPqSnappy)
        return fail(BOWGPU_ERR_UNSUPPORTED, "parquet: compression codec %d (UNCOMPRESSED = 0 and SNAPPY = 1 are written)", codec);
    Ctx *c;
    BG_TRY(ctx_get(&c));
    PqWriter w;
    if (w.open(path, names, plan.types.data(), ncols, plan.statistics, o ? o->meta_keys : nullptr, o ? o->meta_values : nullptr, o ? o->n_meta : 0) != 0)
        return writer_fail(w);
    PqEncChunk ch;   // (one chunk's images at a time, in host buffers that are taken once)
    for (int64_t a = 0; a < plan.n; a += plan.rg_rows) {
        const int64_t b = a + plan.rg_rows < plan.n ? a + plan.rg_rows : plan.n;
        if (w.begin_row_group(b - a) != 0) return writer_fail(w);
        for (int i = 0; i < ncols; i++) {
            if (plan.types[(size_t)i] == kPqBoolean) BG_TRY(synced(c, pq_encode_bool_chunk(c, cols[i], a, b, plan.page_rows, codec, plan.statistics, &ch)));
            else BG_TRY(synced(c, pq_encode_chunk(c, cols[i], a, b, plan.page_rows, plan.enc[(size_t)i], codec, plan.statistics, &ch)));
            // (ch.encoding: PLAIN where a dictionary was asked for and the chunk fell back)
            if (w.add_chunk(ch.encoding, ch.pages.data(), (int64_t)ch.pages.size(), ch.stats, codec, ch.dict.empty() ? nullptr : ch.dict.data(), (int64_t)ch.dict.size()) != 0)
                return writer_fail(w);
        }
        if (w.end_row_group() != 0) return writer_fail(w);
    }
    PqwTotals t;
    if (w.finish(&t) != 0) return writer_fail(w);
    if (info) {
        info->file_bytes = t.file_bytes;
        info->rows = t.rows;
        info->row_groups = t.row_groups;
        info->data_pages = t.data_pages;
        info->level_bytes = t.level_bytes;
        info->value_bytes = t.value_bytes;
    }
    return 0;
}

// no C++ exception may cross the C ABI; the writer's destructor has removed the temporary by the time one is caught
int write_guarded(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols, const bowgpu_parquet_write_options *o, int32_t codec,
                  bool booleans, bowgpu_parquet_write_info *info) {
    try { return write_impl(path, cols, names, ncols, o, codec, booleans, info); }
    catch (const std::bad_alloc &) { return fail(BOWGPU_ERR_OOM, "parquet: out of host memory while writing '%s'", path); }
    catch (const std::exception &e) { return fail(BOWGPU_ERR_ARG, "parquet: writing '%s' failed (%s)", path, e.what()); }
}

}  // namespace

extern "C" int bowgpu_parquet_write(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                                    const bowgpu_parquet_write_options *opts, bowgpu_parquet_write_info *info) {
    return write_guarded(path, cols, names, ncols, opts, kPqUncompressed, false, info);
}

extern "C" int bowgpu_parquet_write_codec(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                                          const bowgpu_parquet_write_options *opts, int32_t codec, bowgpu_parquet_write_info *info) {
    return write_guarded(path, cols, names, ncols, opts, codec, false, info);
}

extern "C" int bowgpu_parquet_write_bool(const char *path, const bowgpu_col *cols, const char *const *names, int32_t ncols,
                                         const bowgpu_parquet_write_options *opts, int32_t codec, bowgpu_parquet_write_info *info) {
    return write_guarded(path, cols, names, ncols, opts, codec, true, info);
}
#endif  // BOWGPU_PARQUET_ASSEMBLE_ONLY
