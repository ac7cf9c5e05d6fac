// The file assembly of RLE_DICTIONARY column chunks (bow_amd/csrc/parquet_write.cpp, PqWriter::add_chunk with a dictionary) driven
// from host-made dictionaries and index sections, without a device and without the rest of the library: built with
// -DBOWGPU_PARQUET_ASSEMBLE_ONLY -fsanitize=address,undefined and run by tests/test_parquet_dict_cpu.py, which reads the file back
// with pyarrow and compares it with the same formulas.
//
//   usage: test_parquet_dict_assemble OUT.parquet CODEC        (0: UNCOMPRESSED, 1: SNAPPY)
//
// Two columns, "s" (INT64) and "v" (DOUBLE), statistics on.  Row group 0: pages of 64, 64 and 40 rows, row group 1: one page of 24.
//   "s" at row r: row group 0  ((7 r) % 5) * 1000 - 2000   (5 entries, two of them negative: they sort last; width 3)
//                 row group 1  r % 3 - 1                    (3 entries; width 2)
//   "v" at row r: row group 0  0.25 * (r % 9)               (9 entries; width 4)
//                 row group 1  0.5 * r                      written PLAIN: the chunk a writer falls back on
//   valid rows as in tests/cpp/test_parquet_snappy_assemble.cpp: the three levels forms, and a page without a valid row (the width
//   byte alone) in either column.
// Under SNAPPY a page's values stream is its section as one literal.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../bow_amd/csrc/parquet_write.h"

using namespace bowgpu;

static bool valid_at(int col, int group, int page, int64_t r) {
    if (group == 1) return col == 0 ? r % 2 == 0 : true;
    if (col == 0) return page == 0 ? true : page == 1 ? false : r % 3 != 0;
    return page == 0 ? r % 5 != 1 : page == 1;
}

static uint64_t value_at(int col, int group, int64_t r) {
    uint64_t u;
    if (col == 0) { const int64_t x = group == 0 ? ((7 * r) % 5) * 1000 - 2000 : r % 3 - 1; memcpy(&u, &x, 8); }
    else { const double x = group == 0 ? 0.25 * (double)(r % 9) : 0.5 * (double)r; memcpy(&u, &x, 8); }
    return u;
}

static bool less(int col, uint64_t a, uint64_t b) {
    if (col == 0) return (int64_t)a < (int64_t)b;
    double x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x < y;
}

// the width byte, and one bit-packed run of the indices where there is one
static std::vector<uint8_t> index_section(const std::vector<uint64_t> &vals, const std::vector<uint64_t> &dict) {
    int w = 1;
    while ((1u << w) < dict.size()) w++;
    std::vector<uint8_t> out{(uint8_t)w};
    if (vals.empty()) return out;
    const size_t groups = (vals.size() + 7) / 8;
    for (uint64_t h = (groups << 1) | 1;; h >>= 7) {
        out.push_back((uint8_t)((h & 0x7F) | (h >= 0x80 ? 0x80 : 0)));
        if (h < 0x80) break;
    }
    const size_t at = out.size();
    out.resize(at + groups * (size_t)w, 0);
    for (size_t i = 0; i < vals.size(); i++) {
        const uint64_t idx = (uint64_t)(std::lower_bound(dict.begin(), dict.end(), vals[i]) - dict.begin());
        for (int b = 0; b < w; b++)
            if ((idx >> b) & 1) out[at + (i * (size_t)w + (size_t)b) / 8] |= (uint8_t)(1u << ((i * (size_t)w + (size_t)b) % 8));
    }
    return out;
}

static std::vector<uint8_t> literal(const std::vector<uint8_t> &s) {   // (a section here holds at most 256 bytes)
    std::vector<uint8_t> out;
    if (s.size() <= 60) out.push_back((uint8_t)((s.size() - 1) << 2));
    else { out.push_back(60 << 2); out.push_back((uint8_t)(s.size() - 1)); }
    out.insert(out.end(), s.begin(), s.end());
    return out;
}

#define CHECK(call) do { if ((call) != 0) { fprintf(stderr, "%s\n", w.error().c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s OUT.parquet CODEC\n", argv[0]); return 2; }
    const int32_t codec = atoi(argv[2]);
    const char *names[2] = {"s", "v"};
    const int32_t types[2] = {kPqInt64, kPqDouble};
    PqWriter w;
    CHECK(w.open(argv[1], names, types, 2, true, nullptr, nullptr, 0));
    const std::vector<std::vector<int>> group_pages = {{64, 64, 40}, {24}};
    int64_t row0 = 0, dict_bytes = 0;
    for (int g = 0; g < 2; g++) {
        int64_t rows = 0;
        for (int n : group_pages[g]) rows += n;
        CHECK(w.begin_row_group(rows));
        for (int col = 0; col < 2; col++) {
            const bool plain = g == 1 && col == 1;
            const size_t np = group_pages[g].size();
            std::vector<std::vector<uint8_t>> bits(np), section(np), comp(np);
            std::vector<std::vector<uint64_t>> vals(np);
            std::vector<uint64_t> dict;
            std::vector<PqwPage> pages(np);
            PqwStats st;
            int64_t r = row0;
            for (size_t p = 0; p < np; p++) {
                const int n = group_pages[g][p];
                bits[p].assign((size_t)(n + 7) / 8, 0);
                for (int k = 0; k < n; k++, r++) {
                    if (!valid_at(col, g, (int)p, r)) { st.null_count++; continue; }
                    bits[p][(size_t)k / 8] |= (uint8_t)(1u << (k % 8));
                    const uint64_t x = value_at(col, g, r);
                    vals[p].push_back(x);
                    dict.push_back(x);
                    if (!st.has_minmax || less(col, x, st.min)) st.min = x;
                    if (!st.has_minmax || less(col, st.max, x)) st.max = x;
                    st.has_minmax = true;
                }
            }
            std::sort(dict.begin(), dict.end());   // (as unsigned 64-bit integers)
            dict.erase(std::unique(dict.begin(), dict.end()), dict.end());
            for (size_t p = 0; p < np; p++) {
                if (plain) section[p].assign(reinterpret_cast<const uint8_t *>(vals[p].data()), reinterpret_cast<const uint8_t *>(vals[p].data()) + 8 * vals[p].size());
                else section[p] = index_section(vals[p], dict);
                if (codec == kPqSnappy && !section[p].empty()) comp[p] = literal(section[p]);
                pages[p].rows = group_pages[g][p];
                pages[p].valid = (int32_t)vals[p].size();
                pages[p].level_bits = bits[p].data();
                pages[p].values = codec == kPqSnappy || section[p].empty() ? nullptr : section[p].data();
                pages[p].value_bytes = (int64_t)section[p].size();
                pages[p].comp = comp[p].empty() ? nullptr : comp[p].data();
                pages[p].comp_bytes = (int64_t)comp[p].size();
            }
            if (plain) CHECK(w.add_chunk(kPqEncPlain, pages.data(), (int64_t)np, st, codec));
            else {
                CHECK(w.add_chunk(kPqEncRleDict, pages.data(), (int64_t)np, st, codec, dict.data(), (int64_t)dict.size()));
                dict_bytes += 8 * (int64_t)dict.size();
            }
        }
        CHECK(w.end_row_group());
        row0 += rows;
    }
    PqwTotals t;
    CHECK(w.finish(&t));
    printf("file_bytes %lld rows %lld row_groups %lld data_pages %lld level_bytes %lld value_bytes %lld dict_bytes %lld\n", (long long)t.file_bytes,
           (long long)t.rows, (long long)t.row_groups, (long long)t.data_pages, (long long)t.level_bytes, (long long)t.value_bytes, (long long)dict_bytes);

    // a dictionary chunk without its dictionary, and a dictionary beside another encoding: errors, and the temporaries are gone
    for (int k = 0; k < 2; k++) {
        PqWriter bad;
        const std::string p = std::string(argv[1]) + (k ? ".stray" : ".nodict");
        PqwPage pg;
        pg.rows = 1;
        const uint64_t entry = 5;
        if (bad.open(p.c_str(), names, types, 2, true, nullptr, nullptr, 0) != 0 || bad.begin_row_group(1) != 0) { fprintf(stderr, "%s\n", bad.error().c_str()); return 1; }
        const int rc = k ? bad.add_chunk(kPqEncPlain, &pg, 1, PqwStats(), codec, &entry, 1) : bad.add_chunk(kPqEncRleDict, &pg, 1, PqwStats(), codec);
        if (rc == 0) { fprintf(stderr, "a mismatched dictionary was taken (%d)\n", k); return 1; }
    }
    return 0;
}
