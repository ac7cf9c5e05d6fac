// The file assembly of bowgpu_parquet_write_codec under SNAPPY (bow_amd/csrc/parquet_write.cpp, PqWriter::add_chunk with codec 1)
// driven from host-made page tables, without a device and without the rest of the library: built with
// -DBOWGPU_PARQUET_ASSEMBLE_ONLY -fsanitize=address,undefined and run by tests/test_parquet_snappy_cpu.py, which reads the file back
// with pyarrow and compares it with the same formulas.
//
//   usage: test_parquet_snappy_assemble OUT.parquet
//
// Two columns, "t" (INT64, value 1000 r - 5 at row r) and "v" (DOUBLE, 2.5 everywhere), PLAIN, statistics on.  Row group 0: pages
// of 64, 64 and 40 rows, row group 1: one page of 24 rows.
//   "t" valid rows: page 0 all, page 1 none, page 2 where r % 3 != 0; row group 1 where r % 2 == 0
//   "v" valid rows: page 0 where r % 5 != 1, page 1 all, page 2 none; row group 1 all
// so the three levels forms, pages with an empty values stream, a stream of one literal ("t", row group 1: 96 bytes) and streams
// of several fragments occur.  The values' streams come from fragment_stream() below: the section cut into fragments of 128 bytes,
// a fragment of equal 8-byte words as an 8-byte literal and overlapping copies at distance 8, any other as one literal.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../bow_amd/csrc/parquet_write.h"

using namespace bowgpu;

static bool valid_at(int col, int group, int page, int64_t r) {
    if (group == 1) return col == 0 ? r % 2 == 0 : true;
    if (col == 0) return page == 0 ? true : page == 1 ? false : r % 3 != 0;
    return page == 0 ? r % 5 != 1 : page == 1;
}

static uint64_t value_at(int col, int64_t r) {
    uint64_t u;
    if (col == 0) { const int64_t x = 1000 * r - 5; memcpy(&u, &x, 8); }
    else { const double x = 2.5; memcpy(&u, &x, 8); }
    return u;
}

static bool less(int col, uint64_t a, uint64_t b) {
    if (col == 0) return (int64_t)a < (int64_t)b;
    double x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x < y;
}

static void put_literal(std::vector<uint8_t> *out, const uint8_t *p, size_t n) {
    if (n <= 60) out->push_back((uint8_t)((n - 1) << 2));
    else { out->push_back(60 << 2); out->push_back((uint8_t)(n - 1)); }   // (a fragment holds at most 128 bytes)
    out->insert(out->end(), p, p + n);
}

static constexpr size_t kFrag = 128;
static std::vector<uint8_t> fragment_stream(const uint8_t *p, size_t n) {
    std::vector<uint8_t> out;
    for (size_t a = 0; a < n; a += kFrag) {
        const size_t len = n - a < kFrag ? n - a : kFrag;
        bool same = len >= 16;
        for (size_t k = 8; k < len && same; k++) same = p[a + k] == p[a + k - 8];
        if (!same) { put_literal(&out, p + a, len); continue; }
        put_literal(&out, p + a, 8);
        size_t left = len - 8;   // a multiple of 8, at least 8: copies of 64, the last one of what is left
        while (left > 0) {
            const size_t c = left > 64 ? 64 : left;
            out.push_back((uint8_t)(2 | ((c - 1) << 2)));
            out.push_back(8);
            out.push_back(0);
            left -= c;
        }
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s OUT.parquet\n", argv[0]); return 2; }
    const char *names[2] = {"t", "v"};
    const int32_t types[2] = {kPqInt64, kPqDouble};
    PqWriter w;
    if (w.open(argv[1], names, types, 2, true, nullptr, nullptr, 0) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
    const std::vector<std::vector<int>> group_pages = {{64, 64, 40}, {24}};
    int64_t row0 = 0, comp_bytes = 0;
    for (int g = 0; g < 2; g++) {
        int64_t rows = 0;
        for (int n : group_pages[g]) rows += n;
        if (w.begin_row_group(rows) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        for (int col = 0; col < 2; col++) {
            std::vector<std::vector<uint8_t>> bits(group_pages[g].size()), comp(group_pages[g].size());
            std::vector<PqwPage> pages(group_pages[g].size());
            PqwStats st;
            int64_t r = row0;
            for (size_t p = 0; p < group_pages[g].size(); p++) {
                const int n = group_pages[g][p];
                std::vector<uint64_t> body;
                bits[p].assign((size_t)(n + 7) / 8, 0);
                for (int k = 0; k < n; k++, r++) {
                    if (!valid_at(col, g, (int)p, r)) { st.null_count++; continue; }
                    bits[p][(size_t)k / 8] |= (uint8_t)(1u << (k % 8));
                    const uint64_t x = value_at(col, r);
                    body.push_back(x);
                    if (!st.has_minmax || less(col, x, st.min)) st.min = x;
                    if (!st.has_minmax || less(col, st.max, x)) st.max = x;
                    st.has_minmax = true;
                }
                comp[p] = fragment_stream(reinterpret_cast<const uint8_t *>(body.data()), body.size() * 8);
                comp_bytes += (int64_t)comp[p].size();
                pages[p].rows = n;
                pages[p].valid = (int32_t)body.size();
                pages[p].level_bits = bits[p].data();
                pages[p].values = nullptr;   // (the uncompressed section is not looked at under the codec)
                pages[p].value_bytes = (int64_t)body.size() * 8;
                pages[p].comp = comp[p].empty() ? nullptr : comp[p].data();
                pages[p].comp_bytes = (int64_t)comp[p].size();
            }
            if (w.add_chunk(kPqEncPlain, pages.data(), (int64_t)pages.size(), st, kPqSnappy) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        }
        if (w.end_row_group() != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        row0 += rows;
    }
    PqwTotals t;
    if (w.finish(&t) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
    printf("file_bytes %lld rows %lld row_groups %lld data_pages %lld level_bytes %lld value_bytes %lld comp_bytes %lld\n", (long long)t.file_bytes,
           (long long)t.rows, (long long)t.row_groups, (long long)t.data_pages, (long long)t.level_bytes, (long long)t.value_bytes, (long long)comp_bytes);

    // a codec the writer does not have: an error, and the temporary is gone (the test looks at the directory)
    {
        PqWriter bad;
        const std::string p = std::string(argv[1]) + ".gzip";
        PqwPage pg;
        pg.rows = 1;
        if (bad.open(p.c_str(), names, types, 2, true, nullptr, nullptr, 0) != 0 || bad.begin_row_group(1) != 0) { fprintf(stderr, "%s\n", bad.error().c_str()); return 1; }
        if (bad.add_chunk(kPqEncPlain, &pg, 1, PqwStats(), 2) == 0) { fprintf(stderr, "codec 2 was taken\n"); return 1; }
    }
    return 0;
}
