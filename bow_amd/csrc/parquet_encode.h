// parquet_encode.h — what the device side of the Parquet writer shares: the page grid and the values sections of one column chunk,
// and the one declaration of each function that parquet_encode.hip, parquet_bool_encode.hip, parquet_dict.hip, snappy_encode.hip
// and parquet_write.cpp call across files.  (parquet_write.h stays free of HIP: the stand-alone assembly programs include it.)
#pragma once

#include "common.h"
#include "parquet_write.h"

namespace bowgpu {

// The pages of a chunk of n rows: npages of page_rows rows (a multiple of 64), the last one with the rows that are left
struct PqGrid {
    int64_t n, npages;
    int32_t page_rows;
    PqGrid(int64_t rows, int32_t per_page) : n(rows), npages((rows + per_page - 1) / per_page), page_rows(per_page) {}
    int64_t rows(int64_t p) const { return p + 1 < npages ? page_rows : n - p * page_rows; }
    size_t level_bytes() const { return (size_t)page_rows >> 3; }   // of one page's bits in a levels image: page p's lie at p * level_bytes()
};

// The values sections of a chunk: page p's is image[off[p], off[p] + len[p]), image in device memory.  Every off is a multiple of 8
// and the image is readable up to the next multiple of 8 behind each section.  used: the end of the last section that holds a byte.
// own: the image's memory where its producer allocated it (PLAIN sections lie in the dense values themselves).
struct PqSections {
    const uint8_t *image = nullptr;
    std::vector<int64_t> off, len;
    size_t used = 0;
    DevBuf own;
};

// parquet_encode.hip: rows [a, b) of one Int64 / Float64 column as the pages of one column chunk, encoded on the device and brought
// back once (codec kPqSnappy: the values sections stay on the device and their Snappy streams come back instead)
int pq_encode_chunk(Ctx *c, const bowgpu_col &col, int64_t a, int64_t b, int32_t page_rows, int32_t encoding, int32_t codec, bool minmax, PqEncChunk *out);
// parquet_bool_encode.hip: the same for a Boolean column, whose pages hold the value bits of their valid rows (PLAIN)
int pq_encode_bool_chunk(Ctx *c, const bowgpu_col &col, int64_t a, int64_t b, int32_t page_rows, int32_t codec, bool minmax, PqEncChunk *out);
// parquet_encode.hip, the hand-over of both: page p has valid[p] valid rows, its level bits lie in d_levels (read only when some
// page is mixed), its values in s.  The levels image comes back if a page is mixed; s.used bytes of the values image come back in
// one copy, or (kPqSnappy) their streams do; out->pages is filled.  The stream has drained when this returns.
int pq_finish_chunk(Ctx *c, const PqGrid &g, const std::vector<uint32_t> &valid, const void *d_levels, const PqSections &s, int32_t codec, PqEncChunk *out);
// parquet_dict.hip: the dictionary of the chunk's dense values (m > 0 of them, page p holds counts[p]) and its values sections.
// *fallback: more than BOWGPU_PARQUET_DICT_MAX distinct patterns, nothing else is set.  Else dict holds the entries in the
// contract's order, s the sections, and the stream has drained.
int pq_dict_chunk(Ctx *c, const uint64_t *dense, int64_t m, const std::vector<uint32_t> &counts, std::vector<uint64_t> *dict, PqSections *s, bool *fallback);
// snappy_encode.hip: the sections of s as one raw Snappy stream per page: the streams end to end in out (host), page p's at coff[p]
// with clen[p] bytes (0 for a section without bytes).  The stream has drained when this returns.
int pq_snappy_chunk(Ctx *c, const PqSections &s, PqHostBytes *out, std::vector<int64_t> *coff, std::vector<int64_t> *clen);

}  // namespace bowgpu
