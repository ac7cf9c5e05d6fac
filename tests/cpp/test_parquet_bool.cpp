// test_parquet_bool.cpp — NewBowFromParquet (reference bowparquet.go:44-153) through the C++ mirror of the reference's interface
// (bow_amd/host/bow_rolling.hpp) on a file that holds Int64, Float64 and BOOLEAN columns: under ParquetBooleans::Read the flag
// column arrives as a Boolean series (decoded on the device by bowgpu_parquet_read_bool_column), beside the columns bowgpu_parquet_read_column gives.
// argv[1]: the file tests/test_gpu_parquet_bool_mirror.py wrote with pyarrow; argv[2]: its row count.  Row r holds
//   time  = 10 r                       (Int64, no nulls)
//   value = r / 2                      (Float64, null where r % 5 == 3)
//   flag  = r % 3 == 0                 (Boolean, null where r % 7 == 2)
// Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../bow_amd/host/bow_rolling.hpp"

using namespace bow;
namespace rl = bow::rolling;
namespace ag = bow::rolling::aggregation;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        g_checks++;                                                                 \
        if (!(cond)) { g_fail++; printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: test_parquet_bool FILE ROWS\n"); return 2; }
    const int rows = atoi(argv[2]);
    auto [b, e] = NewBowFromParquet(argv[1], ParquetBooleans::Read);
    CHECK(!e);
    if (e) { printf("   %s\n%d checks, %d failures\n", e.msg.c_str(), g_checks, g_fail); return 1; }
    CHECK(b->NumRows() == rows);
    CHECK(b->NumCols() == 3);
    CHECK(b->ColumnName(0) == "time" && b->ColumnName(1) == "value" && b->ColumnName(2) == "flag");
    CHECK(b->ColumnType(0) == Int64 && b->ColumnType(1) == Float64 && b->ColumnType(2) == Boolean);
    int bad = 0;
    for (int r = 0; r < rows && b->NumCols() == 3; r++) {
        const Value t = I(10 * (int64_t)r);
        const Value v = r % 5 == 3 ? N : F(r / 2.0);
        const Value f = r % 7 == 2 ? N : Scalar(r % 3 == 0);
        if (!(b->GetValue(0, r) == t) || !(b->GetValue(1, r) == v) || !(b->GetValue(2, r) == f)) {
            if (bad++ < 10) printf("FAIL row %d\n", r);
        }
    }
    CHECK(bad == 0);
    {   // the default keeps skipping the flag column, as the mirror always did
        auto [skipped, e0] = NewBowFromParquet(argv[1]);
        CHECK(!e0);
        CHECK(skipped && skipped->NumCols() == 2 && skipped->ColumnName(1) == "value");
    }
    // the Boolean series is one the device reducers take: a window's Count and Mode over the flag
    auto [r, e2] = rl::IntervalRolling(b, "time", 100, {});
    CHECK(!e2);
    if (!e2) {
        auto [a, e3] = r->Aggregate({ag::WindowStart("time"), ag::Count("flag"), ag::Mode("flag")})->Bow();
        CHECK(!e3);
        if (e3) printf("   %s\n", e3.msg.c_str());
        if (!e3) {
            CHECK(a->NumRows() == (rows + 9) / 10);
            CHECK(a->ColumnType(2) == Boolean);
            // window 0 holds rows 0 .. 9: row 2 and row 9 are null; true at rows 0, 3, 6 -> 3 of 8: Mode false
            CHECK(a->GetValue(1, 0) == I(8));
            CHECK(a->GetValue(2, 0) == Scalar(false));
        }
    }
    if (argc > 3) {   // argv[3]: tests/golden/bow1-100-rows.parquet, the reference's own benchmark input (written by parquet-go)
        auto [g, e4] = NewBowFromParquet(argv[3], ParquetBooleans::Read);
        CHECK(!e4);
        if (e4) printf("   %s\n", e4.msg.c_str());
        CHECK(g && g->NumRows() == 100 && g->NumCols() == 5);
        CHECK(g && g->NumCols() == 5 && g->ColumnName(3) == "Float64_bow1" && g->ColumnName(4) == "Boolean_bow1" && g->ColumnType(4) == Boolean);
    }
    printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
