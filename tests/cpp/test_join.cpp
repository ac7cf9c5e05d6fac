// test_join.cpp — the reference's tests of Bow.OuterJoin and Bow.InnerJoin (bowjoin_test.go:11-669), read from
// tests/golden/join_vectors.json and replayed through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp), i.e. through the
// C ABI and the HIP kernels.  Needs a GPU (run by tests/test_gpu_join.py).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "fixture_json.hpp"

using namespace bow;
using fixture::J;

static int g_fail = 0, g_checks = 0;
static std::string g_test;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        g_checks++;                                                                     \
        if (!(cond)) { g_fail++; printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_test.c_str(), #cond); } \
    } while (0)

static void expect_equal(const BowPtr &have, const BowPtr &want) {
    g_checks++;
    if (!have || !have->Equal(*want)) {
        g_fail++;
        printf("FAIL [%s]\n expect:\n%s have:\n%s", g_test.c_str(), want->String().c_str(), have ? have->String().c_str() : "<nil>\n");
    }
}

static void null_slots_hold_zero(const BowPtr &b) {
    for (const Series &s : b->cols)
        for (int64_t row = 0; row < s.length; row++)
            if (!s.IsValid(row)) CHECK(s.data[(size_t)row] == 0);
}

static uint64_t bits(const BowPtr &b, int col, int row) { return b->cols[(size_t)col].data[(size_t)row]; }

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const J doc = fixture::load(dir + "/join_vectors.json");
    int ran = 0, expected = 0, declined = 0, errors = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = c["name"].str + " (" + c["source"].str + ")";
        ran++;
        const BowPtr left = fixture::frame(c["left"]), right = fixture::frame(c["right"]);
        CHECK(left != nullptr && right != nullptr);
        if (!left || !right) continue;
        const bool outer = c["kind"].str == "outer";
        std::pair<BowPtr, Error> r = outer ? left->OuterJoin(right) : left->InnerJoin(right);
        if (c.has("declined")) {   // two common columns: one key per side, so an Error and no frame
            declined++;
            CHECK((bool)r.second && r.first == nullptr && r.second.msg.find("common columns") != std::string::npos);
            continue;
        }
        if (c.has("error")) {   // the reference's panic text, with the column's name
            errors++;
            const std::string name = left->ColumnName((int)c["left_key"].inum);
            CHECK((bool)r.second && r.first == nullptr && r.second.msg == c["error"].str + ": " + name);
            continue;
        }
        expected++;
        CHECK(!r.second);
        if (r.second) { printf("   error: %s\n", r.second.msg.c_str()); continue; }
        expect_equal(r.first, fixture::frame(c["expected"]));
        null_slots_hold_zero(r.first);
    }
    CHECK(ran == 19 && expected == 12 && declined == 5 && errors == 2);
    {   // two series on one clock put into one frame, as before a Rolling.Aggregate
        g_test = "OuterJoin / InnerJoin";
        const BowPtr a = NewBowFromColBasedInterfaces({"time", "a"}, {Float64, Int64},
                                                      {{F(30.), F(-0.0), N, F(10.), F(10.)}, {I(1), I(2), I(3), N, I(5)}}).first;
        const BowPtr b = NewBowFromColBasedInterfaces({"b", "time"}, {Float64, Float64},
                                                      {{F(.5), N, F(2.5), F(3.5), F(4.5)}, {F(10.), F(0.0), N, F(20.), F(10.)}}).first;
        auto [o, e1] = a->OuterJoin(b);
        CHECK(!e1);
        if (!e1) {   // left rows in their own order, ties in ascending right row, nil == nil, the right-only row behind with ITS key
            expect_equal(o, NewBowFromColBasedInterfaces({"time", "a", "b"}, {Float64, Int64, Float64},
                                                         {{F(30.), F(-0.0), N, F(10.), F(10.), F(10.), F(10.), F(20.)},
                                                          {I(1), I(2), I(3), N, N, I(5), I(5), N},
                                                          {N, N, F(2.5), F(.5), F(4.5), F(.5), F(4.5), F(3.5)}}).first);
            CHECK(bits(o, 0, 1) == 0x8000000000000000ull);   // -0.0 == +0.0, and the key keeps the LEFT row's bits
            null_slots_hold_zero(o);
        }
        auto [i, e2] = a->InnerJoin(b);
        CHECK(!e2);
        if (!e2)
            expect_equal(i, NewBowFromColBasedInterfaces({"time", "a", "b"}, {Float64, Int64, Float64},
                                                         {{F(-0.0), N, F(10.), F(10.), F(10.), F(10.)},
                                                          {I(2), I(3), N, N, I(5), I(5)},
                                                          {N, F(2.5), F(.5), F(4.5), F(.5), F(4.5)}}).first);
        auto [sw, e3] = b->OuterJoin(a);   // the other way round: b's columns first, its key where b has it
        CHECK(!e3 && sw && sw->NumCols() == 3 && sw->ColumnName(0) == "b" && sw->ColumnName(1) == "time" && sw->ColumnName(2) == "a" &&
              sw->NumRows() == 8);
        // a NaN among the valid keys: the device declines it, and the Error says so
        const BowPtr nan = NewBowFromColBasedInterfaces({"time"}, {Float64}, {{F(1.), F(std::nan(""))}}).first;
        auto [bad1, e4] = a->OuterJoin(nan);
        CHECK((bool)e4 && bad1 == nullptr && e4.msg.find("NaN") != std::string::npos);
        // where the reference panics: no bow, a name twice in the right bow
        auto [bad2, e5] = a->InnerJoin(nullptr);
        CHECK((bool)e5 && bad2 == nullptr);
        const BowPtr twice = NewBowFromColBasedInterfaces({"time", "time"}, {Float64, Float64}, {{F(1.)}, {F(1.)}}).first;
        auto [bad3, e6] = a->OuterJoin(twice);
        CHECK((bool)e6 && bad3 == nullptr && e6.msg.rfind("too many columns have the same name", 0) == 0);
        // InnerJoin with a bow without columns: the empty slice of the one that has some (bowjoin.go:19-29)
        const BowPtr none = std::make_shared<Bow>();
        auto [s1, e7] = a->InnerJoin(none);
        auto [s2, e8] = none->InnerJoin(a);
        CHECK(!e7 && !e8 && s1 && s2 && s1->NumRows() == 0 && s2->NumRows() == 0 && s1->NumCols() == 2 && s2->NumCols() == 2);
    }
    printf("%d checks, %d failures, %d cases of bowjoin_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
