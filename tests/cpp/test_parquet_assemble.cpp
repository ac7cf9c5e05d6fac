// The file assembly of bowgpu_parquet_write (bow_amd/csrc/parquet_write.cpp, PqWriter) driven from host-made page bodies, without
// a device and without the rest of the library: built with -DBOWGPU_PARQUET_ASSEMBLE_ONLY -fsanitize=address,undefined and run by
// tests/test_parquet_write_cpu.py, which reads the file back with pyarrow and compares it with the same formulas.
//
//   usage: test_parquet_assemble OUT.parquet
//
// Two columns, "t" (INT64, value 1000 r - 5 at row r) and "v" (DOUBLE, 0.5 r - 10), PLAIN, statistics on, metadata
// {"origin": "assemble", "empty": ""}.  Row group 0: pages of 64, 64 and 40 rows, row group 1: one page of 24 rows.
//   "t" valid rows: page 0 all, page 1 none, page 2 where r % 3 != 0; row group 1 where r % 2 == 0
//   "v" valid rows: page 0 where r % 5 != 1, page 1 all, page 2 none; row group 1 all
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
    else { const double x = 0.5 * (double)r - 10.0; memcpy(&u, &x, 8); }
    return u;
}

static bool less(int col, uint64_t a, uint64_t b) {
    if (col == 0) return (int64_t)a < (int64_t)b;
    double x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x < y;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s OUT.parquet\n", argv[0]); return 2; }
    const char *names[2] = {"t", "v"};
    const int32_t types[2] = {kPqInt64, kPqDouble};
    const char *keys[2] = {"origin", "empty"}, *vals[2] = {"assemble", ""};
    PqWriter w;
    if (w.open(argv[1], names, types, 2, true, keys, vals, 2) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
    const std::vector<std::vector<int>> group_pages = {{64, 64, 40}, {24}};
    int64_t row0 = 0;
    for (int g = 0; g < 2; g++) {
        int64_t rows = 0;
        for (int n : group_pages[g]) rows += n;
        if (w.begin_row_group(rows) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        for (int col = 0; col < 2; col++) {
            std::vector<std::vector<uint8_t>> bits(group_pages[g].size());
            std::vector<std::vector<uint64_t>> body(group_pages[g].size());
            std::vector<PqwPage> pages(group_pages[g].size());
            PqwStats st;
            int64_t r = row0;
            for (size_t p = 0; p < group_pages[g].size(); p++) {
                const int n = group_pages[g][p];
                bits[p].assign((size_t)(n + 7) / 8, 0);
                for (int k = 0; k < n; k++, r++) {
                    if (!valid_at(col, g, (int)p, r)) { st.null_count++; continue; }
                    bits[p][(size_t)k / 8] |= (uint8_t)(1u << (k % 8));
                    const uint64_t x = value_at(col, r);
                    body[p].push_back(x);
                    if (!st.has_minmax || less(col, x, st.min)) st.min = x;
                    if (!st.has_minmax || less(col, st.max, x)) st.max = x;
                    st.has_minmax = true;
                }
                pages[p].rows = n;
                pages[p].valid = (int32_t)body[p].size();
                pages[p].level_bits = bits[p].data();
                pages[p].values = reinterpret_cast<const uint8_t *>(body[p].data());
                pages[p].value_bytes = (int64_t)body[p].size() * 8;
            }
            if (w.add_chunk(kPqEncPlain, pages.data(), (int64_t)pages.size(), st) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        }
        if (w.end_row_group() != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
        row0 += rows;
    }
    PqwTotals t;
    if (w.finish(&t) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
    printf("file_bytes %lld rows %lld row_groups %lld data_pages %lld level_bytes %lld value_bytes %lld\n", (long long)t.file_bytes, (long long)t.rows,
           (long long)t.row_groups, (long long)t.data_pages, (long long)t.level_bytes, (long long)t.value_bytes);

    // a path that cannot be created: an error with the errno text, and no temporary
    PqWriter bad;
    if (bad.open("/nonexistent-directory/x.parquet", names, types, 2, true, nullptr, nullptr, 0) == 0) { fprintf(stderr, "open of a bad path succeeded\n"); return 1; }
    if (bad.error().find("No such file") == std::string::npos) { fprintf(stderr, "unexpected error text: %s\n", bad.error().c_str()); return 1; }
    // a writer given up half way removes its temporary (the test looks at the directory)
    {
        PqWriter half;
        const std::string p = std::string(argv[1]) + ".abandoned";
        if (half.open(p.c_str(), names, types, 2, true, nullptr, nullptr, 0) != 0 || half.begin_row_group(1) != 0) { fprintf(stderr, "%s\n", half.error().c_str()); return 1; }
    }
    return 0;
}
