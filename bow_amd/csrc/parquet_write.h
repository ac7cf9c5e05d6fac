// What parquet_write.cpp (the file assembly: plain C++ over host buffers, no device, no other translation unit of the library)
// and parquet_encode.hip / parquet_bool_encode.hip (the encoding of one column chunk on the device; what those files share among
// themselves is parquet_encode.h) hand each other.  Included by
// the stand-alone assembly tests as well (tests/cpp/test_parquet_assemble.cpp, test_parquet_bool_assemble.cpp), so nothing here
// needs HIP.
#pragma once

#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

namespace bowgpu {

constexpr int32_t kPqEncPlain = 0, kPqEncDelta = 5, kPqEncRleDict = 8;   // Parquet Encoding values the writer produces
constexpr int32_t kPqBoolean = 0, kPqInt64 = 2, kPqDouble = 5;   // Parquet physical types
constexpr int32_t kPqUncompressed = 0, kPqSnappy = 1; // Parquet CompressionCodec values the writer produces

// One data page as the assembly takes it: its level BIT bytes (ceil(rows / 8), bit k = row k of the page is valid; read only when
// 0 < valid < rows) and its encoded values section, both in host memory.  Under kPqSnappy the section itself stays away: value_bytes
// is still its size, and comp / comp_bytes is the raw Snappy stream (a sequence of elements, no preamble) that decodes to it.
struct PqwPage {
    int32_t rows = 0, valid = 0;
    const uint8_t *level_bits = nullptr;
    const uint8_t *values = nullptr;
    int64_t value_bytes = 0;
    const uint8_t *comp = nullptr;
    int64_t comp_bytes = 0;
};
// Statistics of one column chunk: min / max are the raw 8-byte payloads of the column's type (kPqBoolean: 0 / 1, written as one byte)
struct PqwStats {
    bool has_minmax = false;
    uint64_t min = 0, max = 0;
    int64_t null_count = 0;
};
// A host buffer that only grows and is never cleared: the images of one column chunk after the other land in the same pages
struct PqHostBytes {
    std::unique_ptr<uint8_t[]> p;
    size_t cap = 0;
    uint8_t *take(size_t n) {
        if (cap < n) { p.reset(); p.reset(new uint8_t[n]); cap = n; }
        return p.get();
    }
};
// One column chunk as parquet_encode.hip hands it over: the page table, and the host images its pages point into.  encoding: what the
// chunk came out as - kPqEncPlain where kPqEncRleDict was asked for and the chunk has no value or too many distinct ones; dict: the
// entries of a kPqEncRleDict chunk in the order of the contract, empty otherwise
struct PqEncChunk {
    std::vector<PqwPage> pages;
    PqHostBytes levels, values, comp;
    PqwStats stats;
    int32_t encoding = kPqEncPlain;
    std::vector<uint64_t> dict;
};
struct PqwTotals { int64_t file_bytes = 0, rows = 0, row_groups = 0, data_pages = 0, level_bytes = 0, value_bytes = 0; };

// The file, written front to back under `<path>.tmp` and renamed by finish().  Every method returns 0 or -1 with error() set (an
// errno text where a system call failed); after a failure, or when the writer goes away before finish(), the temporary is removed.
// Call order: open, then per row group begin_row_group, add_chunk once per column in column order, end_row_group; finish.
class PqWriter {
public:
    PqWriter() = default;
    PqWriter(const PqWriter &) = delete;
    PqWriter &operator=(const PqWriter &) = delete;
    ~PqWriter();
    // types: kPqInt64 / kPqDouble / kPqBoolean per column; statistics: min / max in the chunk metadata and column_orders in the footer
    int open(const char *path, const char *const *names, const int32_t *types, int32_t ncols, bool statistics, const char *const *meta_keys,
             const char *const *meta_values, int32_t n_meta);
    int begin_row_group(int64_t rows);
    // codec kPqSnappy: a page's compressed section is the preamble (the varint of its uncompressed size), its levels section as
    // one literal element, and the page's comp stream as it lies.  encoding kPqEncRleDict: dict / ndict (> 0) are the chunk's dictionary
    // entries, 8 bytes each, written as its dictionary page in front of the data pages (kPqSnappy: as literal elements, here); a page's
    // values section is then the bit width and its indices as parquet_dict.hip leaves them
    int add_chunk(int32_t encoding, const PqwPage *pages, int64_t npages, const PqwStats &stats, int32_t codec = kPqUncompressed,
                  const uint64_t *dict = nullptr, int64_t ndict = 0);
    int end_row_group();
    int finish(PqwTotals *totals);
    const std::string &error() const { return err_; }

private:
    struct Chunk { int32_t encoding, codec; int64_t offset, data_offset, bytes, raw, values; PqwStats stats; };   // offset: of the chunk (its dictionary page, if any); bytes: as written; raw: uncompressed
    struct Group { int64_t rows, bytes; std::vector<Chunk> chunks; };                                // bytes: uncompressed
    int put(const void *p, size_t n);
    int flush();
    int sys_fail(const char *what);
    void drop();

    std::string path_, tmp_, err_;
    int fd_ = -1;
    bool stats_ = false;
    std::vector<std::string> names_, meta_k_, meta_v_;
    std::vector<int32_t> types_;
    std::vector<Group> groups_;
    std::vector<uint8_t> buf_;
    int64_t pos_ = 0;   // bytes handed to put() so far: the file offset of the next one
    PqwTotals tot_;
};

}  // namespace bowgpu
