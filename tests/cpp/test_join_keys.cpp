// test_join_keys.cpp — the reference's tests of Bow.OuterJoin and Bow.InnerJoin on bows that share TWO column names (the five cases of
// bowjoin_test.go that tests/golden/join_vectors.json marks "declined"), read from tests/golden/join_keys_vectors.json and replayed
// through Bow::InnerJoinAll / OuterJoinAll of the C++ mirror (bow_amd/host/bow_rolling.hpp), i.e. through bowgpu_join_keys and the HIP
// kernels.  Needs a GPU (run by tests/test_gpu_join_keys.py).
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
    const J doc = fixture::load(dir + "/join_keys_vectors.json");
    int ran = 0, swapped = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = c["name"].str + " (" + c["source"].str + ")";
        ran++;
        const BowPtr left = fixture::frame(c["left"]), right = fixture::frame(c["right"]);
        CHECK(left != nullptr && right != nullptr);
        if (!left || !right) continue;
        const bool outer = c["kind"].str == "outer";
        // InnerJoin / OuterJoin keep declining two common columns
        std::pair<BowPtr, Error> one = outer ? left->OuterJoin(right) : left->InnerJoin(right);
        CHECK((bool)one.second && one.first == nullptr && one.second.msg.find("common columns") != std::string::npos);
        std::pair<BowPtr, Error> r = outer ? left->OuterJoinAll(right) : left->InnerJoinAll(right);
        CHECK(!r.second);
        if (r.second) { printf("   error: %s\n", r.second.msg.c_str()); continue; }
        expect_equal(r.first, fixture::frame(c["expected"]));
        null_slots_hold_zero(r.first);
        if (c.has("expected_swapped")) {   // the reference's second assertion: right.OuterJoin(left)
            swapped++;
            std::pair<BowPtr, Error> s = outer ? right->OuterJoinAll(left) : right->InnerJoinAll(left);
            CHECK(!s.second);
            if (!s.second) expect_equal(s.first, fixture::frame(c["expected_swapped"]));
        }
    }
    CHECK(ran == 5 && swapped == 1);
    {   // several series on one clock: frames that share (time, series)
        g_test = "OuterJoinAll / InnerJoinAll";
        const BowPtr a = NewBowFromColBasedInterfaces({"time", "series", "a"}, {Float64, Int64, Int64},
                                                      {{F(10.), F(10.), F(-0.0), N, F(20.)}, {I(1), I(2), I(1), N, I(1)}, {I(1), I(2), I(3), N, I(5)}}).first;
        const BowPtr b = NewBowFromColBasedInterfaces({"b", "series", "time"}, {Float64, Int64, Float64},
                                                      {{F(.5), F(1.5), F(2.5), F(3.5), F(4.5)}, {I(2), I(1), N, I(1), I(2)},
                                                       {F(10.), F(0.0), N, F(30.), F(10.)}}).first;
        auto [o, e1] = a->OuterJoinAll(b);
        CHECK(!e1);
        if (!e1) {   // (10, 2) twice in ascending right row, -0.0 == +0.0, (nil, nil) == (nil, nil), the right-only row with ITS two keys
            expect_equal(o, NewBowFromColBasedInterfaces({"time", "series", "a", "b"}, {Float64, Int64, Int64, Float64},
                                                         {{F(10.), F(10.), F(10.), F(-0.0), N, F(20.), F(30.)},
                                                          {I(1), I(2), I(2), I(1), N, I(1), I(1)},
                                                          {I(1), I(2), I(2), I(3), N, I(5), N},
                                                          {N, F(.5), F(4.5), F(1.5), F(2.5), N, F(3.5)}}).first);
            CHECK(bits(o, 0, 3) == 0x8000000000000000ull);   // the key keeps the LEFT row's bits
            null_slots_hold_zero(o);
        }
        auto [i, e2] = a->InnerJoinAll(b);
        CHECK(!e2);
        if (!e2)
            expect_equal(i, NewBowFromColBasedInterfaces({"time", "series", "a", "b"}, {Float64, Int64, Int64, Float64},
                                                         {{F(10.), F(10.), F(-0.0), N}, {I(2), I(2), I(1), N}, {I(2), I(2), I(3), N},
                                                          {F(.5), F(4.5), F(1.5), F(2.5)}}).first);
        // with one common column and with none: exactly what InnerJoin / OuterJoin return
        const BowPtr one = NewBowFromColBasedInterfaces({"time", "c"}, {Float64, Int64}, {{F(10.), F(40.), N}, {I(7), I(8), I(9)}}).first;
        const BowPtr none = NewBowFromColBasedInterfaces({"x"}, {Int64}, {{I(1), I(2)}}).first;
        for (const BowPtr &other : {one, none}) {
            auto [p, e3] = a->OuterJoin(other);
            auto [q, e4] = a->OuterJoinAll(other);
            CHECK(!e3 && !e4 && p && q && p->Equal(*q));
            auto [p2, e5] = a->InnerJoin(other);
            auto [q2, e6] = a->InnerJoinAll(other);
            CHECK(!e5 && !e6 && p2 && q2 && p2->Equal(*q2));
        }
        // a NaN among the valid keys of a key pair, on the right: the device declines it, and the Error names the side
        const BowPtr nan = NewBowFromColBasedInterfaces({"series", "time"}, {Int64, Float64}, {{I(1), I(2)}, {F(1.), F(std::nan(""))}}).first;
        auto [bad1, e7] = a->OuterJoinAll(nan);
        CHECK((bool)e7 && bad1 == nullptr && e7.msg.find("NaN") != std::string::npos && e7.msg.find("right") != std::string::npos);
        // where the reference panics: no bow, a name twice in the right bow, a common column of different types (named)
        auto [bad2, e8] = a->InnerJoinAll(nullptr);
        CHECK((bool)e8 && bad2 == nullptr);
        const BowPtr twice = NewBowFromColBasedInterfaces({"time", "series", "time"}, {Float64, Int64, Float64}, {{F(1.)}, {I(1)}, {F(1.)}}).first;
        auto [bad3, e9] = a->OuterJoinAll(twice);
        CHECK((bool)e9 && bad3 == nullptr && e9.msg.rfind("too many columns have the same name", 0) == 0);
        const BowPtr typed = NewBowFromColBasedInterfaces({"time", "series"}, {Float64, Float64}, {{F(1.)}, {F(1.)}}).first;
        auto [bad4, e10] = a->OuterJoinAll(typed);
        CHECK((bool)e10 && bad4 == nullptr && e10.msg == "left and right bow on join columns are of incompatible types: series");
    }
    printf("%d checks, %d failures, %d cases of bowjoin_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
