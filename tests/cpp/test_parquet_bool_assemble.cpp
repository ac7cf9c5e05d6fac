// The file assembly of bowgpu_parquet_write_bool (bow_amd/csrc/parquet_write.cpp, PqWriter) with a BOOLEAN column, driven from
// host-made page bodies without a device and without the rest of the library: built with -DBOWGPU_PARQUET_ASSEMBLE_ONLY
// -fsanitize=address,undefined and run by tests/test_parquet_bool_write_cpu.py, which reads the files back with pyarrow and
// compares them with the same formulas.
//
//   usage: test_parquet_bool_assemble OUT_DIR      writes OUT_DIR/stored.parquet and OUT_DIR/snappy.parquet
//
// Two columns, "t" (INT64, value 1000 r - 5 at row r, no nulls) and "flag" (BOOLEAN, true where (7 r) % 5 < 2), PLAIN, statistics
// on.  Row group 0: pages of 64, 64 and 40 rows, row group 1: one page of 24 rows.
//   "flag" valid rows: page 0 all (k = 64), page 1 none (k = 0), page 2 where r % 3 != 0 (k = 27); row group 1 where r % 2 == 0 (k = 12)
// Under SNAPPY a page's values stream is its section as one literal element (what any Snappy reader takes).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bow_amd/csrc/parquet_write.h"

using namespace bowgpu;

static bool flag_valid(int group, int page, int64_t r) {
    if (group == 1) return r % 2 == 0;
    return page == 0 ? true : page == 1 ? false : r % 3 != 0;
}
static bool flag_at(int64_t r) { return (7 * r) % 5 < 2; }

// the raw Snappy stream of one literal element over `body` (empty for an empty body)
static std::vector<uint8_t> literal(const std::vector<uint8_t> &body) {
    std::vector<uint8_t> s;
    const size_t n = body.size();
    if (n == 0) return s;
    if (n <= 60) s.push_back((uint8_t)((n - 1) << 2));
    else {
        const int k = n <= 256 ? 1 : 2;
        s.push_back((uint8_t)((59 + k) << 2));
        for (int j = 0; j < k; j++) s.push_back((uint8_t)((n - 1) >> (8 * j)));
    }
    s.insert(s.end(), body.begin(), body.end());
    return s;
}

static int fail(const PqWriter &w) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; }

static const std::vector<std::vector<int>> kGroupPages = {{64, 64, 40}, {24}};

// one column chunk of group g from row row0 on; col 0: "t", col 1: "flag"
static int add_column(PqWriter &w, int col, int g, int64_t row0, int32_t codec) {
    const size_t np = kGroupPages[g].size();
    std::vector<std::vector<uint8_t>> bits(np), body(np), comp(np);
    std::vector<PqwPage> pages(np);
    PqwStats st;
    int64_t r = row0;
    for (size_t p = 0; p < np; p++) {
        const int n = kGroupPages[g][p];
        bits[p].assign((size_t)(n + 7) / 8, 0);
        int k = 0;
        for (int i = 0; i < n; i++, r++) {
            if (col == 1 && !flag_valid(g, (int)p, r)) { st.null_count++; continue; }
            bits[p][(size_t)i / 8] |= (uint8_t)(1u << (i % 8));
            uint64_t x;
            if (col == 0) {
                const int64_t v = 1000 * r - 5;
                memcpy(&x, &v, 8);
                for (int j = 0; j < 8; j++) body[p].push_back((uint8_t)(x >> (8 * j)));
                if (!st.has_minmax || v < (int64_t)st.min) st.min = x;
                if (!st.has_minmax || v > (int64_t)st.max) st.max = x;
            } else {
                x = flag_at(r) ? 1 : 0;
                if (k % 8 == 0) body[p].push_back(0);
                body[p].back() |= (uint8_t)(x << (k % 8));
                if (!st.has_minmax || x < st.min) st.min = x;
                if (!st.has_minmax || x > st.max) st.max = x;
            }
            st.has_minmax = true;
            k++;
        }
        comp[p] = literal(body[p]);
        pages[p].rows = n;
        pages[p].valid = k;
        pages[p].level_bits = bits[p].data();
        pages[p].value_bytes = (int64_t)body[p].size();
        if (codec == kPqSnappy) { pages[p].comp = comp[p].data(); pages[p].comp_bytes = (int64_t)comp[p].size(); }
        else pages[p].values = body[p].data();
    }
    return w.add_chunk(kPqEncPlain, pages.data(), (int64_t)pages.size(), st, codec);
}

static const char *kNames[2] = {"t", "flag"};
static const int32_t kTypes[2] = {kPqInt64, kPqBoolean};

static int assemble(const std::string &path, int32_t codec) {
    PqWriter w;
    if (w.open(path.c_str(), kNames, kTypes, 2, true, nullptr, nullptr, 0) != 0) return fail(w);
    int64_t row0 = 0;
    for (int g = 0; g < 2; g++) {
        int64_t rows = 0;
        for (int n : kGroupPages[g]) rows += n;
        if (w.begin_row_group(rows) != 0) return fail(w);
        for (int col = 0; col < 2; col++)
            if (add_column(w, col, g, row0, codec) != 0) return fail(w);
        if (w.end_row_group() != 0) return fail(w);
        row0 += rows;
    }
    PqwTotals t;
    if (w.finish(&t) != 0) return fail(w);
    printf("file_bytes %lld rows %lld row_groups %lld data_pages %lld level_bytes %lld value_bytes %lld\n", (long long)t.file_bytes, (long long)t.rows,
           (long long)t.row_groups, (long long)t.data_pages, (long long)t.level_bytes, (long long)t.value_bytes);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s OUT_DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    if (assemble(dir + "/stored.parquet", kPqUncompressed) != 0) return 1;
    if (assemble(dir + "/snappy.parquet", kPqSnappy) != 0) return 1;
    // a writer given up behind its first column chunks removes its temporary (the test looks at the directory)
    {
        PqWriter half;
        const std::string p = dir + "/abandoned.parquet";
        if (half.open(p.c_str(), kNames, kTypes, 2, true, nullptr, nullptr, 0) != 0 || half.begin_row_group(168) != 0) return fail(half);
        if (add_column(half, 0, 0, 0, kPqSnappy) != 0 || add_column(half, 1, 0, 0, kPqSnappy) != 0) return fail(half);
    }
    return 0;
}
