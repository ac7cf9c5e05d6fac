// test_convert.cpp — Bow.Convert (reference bowsetters.go:52-56; Type.Convert, bowtypes.go:64-81; bowconvert.go) among Int64, Float64
// and Boolean through the C++ mirror of the reference's interface (bow_amd/host/bow_rolling.hpp): the nine pairs over a column with
// nulls, names and the other columns kept, a Boolean series in through its Arrow bits and out through the unpacking, the amd64
// result of an out-of-range Float64 -> Int64, and the String decline.  Needs a GPU (run by tests/test_gpu_convert.py).
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../bow_amd/host/bow_rolling.hpp"

using namespace bow;

static int g_fail = 0, g_checks = 0;
static std::string g_test;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        g_checks++;                                                                     \
        if (!(cond)) { g_fail++; printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_test.c_str(), #cond); } \
    } while (0)

static Value B(bool v) { return Scalar(v); }

static BowPtr frame(const std::vector<Value> &v, Type vt) {
    return NewBowFromColBasedInterfaces({"time", "value"}, {Int64, vt}, {{I(10), I(11), I(12), I(13), I(14)}, v}).first;
}
static void expectEqual(const BowPtr &got, const BowPtr &want) {
    g_checks++;
    if (!got || !want || !got->Equal(*want)) {
        g_fail++;
        printf("FAIL [%s]\n expect:\n%s have:\n%s", g_test.c_str(), want ? want->String().c_str() : "<nil>\n", got ? got->String().c_str() : "<nil>\n");
    }
}
static void runTestCase(const std::string &name, const std::vector<Value> &in, Type from, Type to, const std::vector<Value> &want) {
    g_test = name;
    auto [got, err] = frame(in, from)->Convert(1, to);
    CHECK(!err);
    if (err) printf("  error: %s\n", err.msg.c_str());
    expectEqual(got, frame(want, to));
}

int main() {
    const std::vector<Value> ints = {I(0), N, I(-3), I(1), I(9007199254740993)};   // 2^53 + 1: a tie, to even
    const std::vector<Value> flts = {F(-0.0), N, F(-1.9), F(0.5), F(1e19)};
    const std::vector<Value> bools = {B(true), N, B(false), B(true), B(false)};
    runTestCase("Int64/Int64", ints, Int64, Int64, ints);
    runTestCase("Int64/Float64", ints, Int64, Float64, {F(0.), N, F(-3.), F(1.), F(9007199254740992.)});
    runTestCase("Int64/Boolean", ints, Int64, Boolean, {B(false), N, B(true), B(true), B(true)});
    runTestCase("Float64/Int64", flts, Float64, Int64, {I(0), N, I(-1), I(0), I(std::numeric_limits<int64_t>::min())});
    runTestCase("Float64/Float64", flts, Float64, Float64, flts);
    runTestCase("Float64/Boolean", flts, Float64, Boolean, {B(false), N, B(true), B(true), B(true)});
    runTestCase("Boolean/Int64", bools, Boolean, Int64, {I(1), N, I(0), I(1), I(0)});
    runTestCase("Boolean/Float64", bools, Boolean, Float64, {F(1.), N, F(0.), F(1.), F(0.)});
    runTestCase("Boolean/Boolean", bools, Boolean, Boolean, bools);
    {   // NaN and the infinities: true as a Boolean, the amd64 "integer indefinite" as an Int64; the other column is untouched
        g_test = "Float64 specials";
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        auto b = frame({F(nan), F(inf), F(-inf), F(9223372036854775808.), F(-9223372036854775808.)}, Float64);
        auto [asInt, e1] = b->Convert(1, Int64);
        CHECK(!e1);
        for (int r = 0; r < 5 && asInt; r++) CHECK(asInt->GetInt64(1, r) == std::make_pair(std::numeric_limits<int64_t>::min(), true));
        auto [asBool, e2] = b->Convert(1, Boolean);
        CHECK(!e2);
        for (int r = 0; r < 5 && asBool; r++) CHECK(asBool->GetValue(1, r) == B(true));
        CHECK(asBool && asBool->ColumnName(1) == "value" && asBool->ColumnType(1) == Boolean && asBool->ColumnType(0) == Int64);
        CHECK(asBool && asBool->GetValue(0, 4) == I(14));
    }
    {   // a chain: Int64 flags -> Boolean -> Float64
        g_test = "chain";
        auto [asBool, e1] = frame({I(1), I(0), N, I(1), I(0)}, Int64)->Convert(1, Boolean);
        CHECK(!e1);
        auto [asFloat, e2] = asBool->Convert(1, Float64);
        CHECK(!e2);
        expectEqual(asFloat, frame({F(1.), F(0.), N, F(1.), F(0.)}, Float64));
    }
    {   // declines: a String target, a column outside the frame
        g_test = "declines";
        auto [r1, e1] = frame(ints, Int64)->Convert(1, String);
        CHECK(!r1 && bool(e1) && e1.msg.find("String") != std::string::npos);
        auto [r2, e2] = frame(ints, Int64)->Convert(2, Int64);
        CHECK(!r2 && bool(e2));
        auto [r3, e3] = frame(ints, Int64)->Convert(1, Type::Unknown);
        CHECK(!r3 && bool(e3));
    }
    printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
