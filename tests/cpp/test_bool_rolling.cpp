// test_bool_rolling.cpp — the reference's "sparse bool" cases (sparseBoolBow, rolling/aggregation/core_test.go, and the "sparse bool"
// case of every rolling/aggregation/*_test.go) replayed through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp): a
// Boolean series reaches the library as Arrow bits, Boolean results come back as a Boolean series.  Needs a GPU (run by
// tests/test_gpu_bool_mirror.py).
#include <cstdio>
#include <string>
#include <vector>

#include "../../bow_amd/host/bow_rolling.hpp"

using namespace bow;
namespace rl = bow::rolling;
namespace ag = bow::rolling::aggregation;
namespace tr = bow::rolling::transformation;

static int g_fail = 0, g_checks = 0;
static std::string g_test;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        g_checks++;                                                                     \
        if (!(cond)) { g_fail++; printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_test.c_str(), #cond); } \
    } while (0)

static const std::string timeCol = "time", valueCol = "value";
static Value B(bool v) { return Scalar(v); }

static BowPtr tv(const std::vector<Value> &t, const std::vector<Value> &v, Type vt) {
    return NewBowFromColBasedInterfaces({timeCol, valueCol}, {Int64, vt}, {t, v}).first;
}
static void expectEqual(const BowPtr &got, const BowPtr &want) {
    g_checks++;
    if (!got || !want || !got->Equal(*want)) {
        g_fail++;
        printf("FAIL [%s]\n expect:\n%s have:\n%s", g_test.c_str(), want ? want->String().c_str() : "<nil>\n", got ? got->String().c_str() : "<nil>\n");
    }
}
static BowPtr sparseBoolBow() {
    return tv({I(10), I(11), I(20), I(40), I(41), I(50), I(51), I(61), I(69)}, {B(true), N, N, N, B(false), B(true), B(false), B(true), B(false)}, Boolean);
}
static BowPtr win6(const std::vector<Value> &v, Type t) { return tv({I(10), I(20), I(30), I(40), I(50), I(60)}, v, t); }
static void runTestCase(const std::string &name, rl::ColAggregationConstruct construct, BowPtr expected) {
    g_test = name;
    auto [r, err] = rl::IntervalRolling(sparseBoolBow(), timeCol, 10, {});
    CHECK(!err);
    auto [aggregated, e] = r->Aggregate({ag::WindowStart(timeCol), construct(valueCol)})->Bow();
    CHECK(!e);
    if (e) printf("  error: %s\n", e.msg.c_str());
    expectEqual(aggregated, expected);
}

int main() {
    runTestCase("Sum/sparse bool", ag::Sum, win6({F(1.), F(0.), F(0.), F(0.), F(1.), F(1.)}, Float64));
    runTestCase("ArithmeticMean/sparse bool", ag::ArithmeticMean, win6({F(1.), N, N, F(0.), F(.5), F(.5)}, Float64));
    runTestCase("Min/sparse bool", ag::Min, win6({F(1.), N, N, F(0.), F(0.), F(0.)}, Float64));
    runTestCase("Max/sparse bool", ag::Max, win6({F(1.), N, N, F(0.), F(1.), F(1.)}, Float64));
    runTestCase("Count/sparse bool", ag::Count, win6({I(1), I(0), I(0), I(1), I(2), I(2)}, Int64));
    runTestCase("First/sparse bool", ag::First, win6({B(true), N, N, B(false), B(true), B(true)}, Boolean));
    runTestCase("Last/sparse bool", ag::Last, win6({B(true), N, N, B(false), B(false), B(false)}, Boolean));
    runTestCase("Mode/sparse bool", ag::Mode, win6({B(true), N, N, B(false), B(true), B(true)}, Boolean));
    runTestCase("IntegralStep/sparse bool", ag::IntegralStep, win6({F(10.), N, N, F(0.), F(1.), F(8.)}, Float64));
    runTestCase("IntegralTrapezoid/sparse bool", ag::IntegralTrapezoid, win6({N, N, N, F(4.5), F(.5), F(4.)}, Float64));
    runTestCase("WeightedAverageStep/sparse bool", ag::WeightedAverageStep, win6({F(1.), N, N, F(0.), F(.1), F(.8)}, Float64));
    runTestCase("WeightedAverageLinear/sparse bool", ag::WeightedAverageLinear, win6({N, N, N, F(.45), F(.05), F(.4)}, Float64));
    {   // transformation.Factor on a Boolean result: the reference's error, carried by the library's decline
        g_test = "First/Factor on bool";
        auto [r, err] = rl::IntervalRolling(sparseBoolBow(), timeCol, 10, {});
        CHECK(!err);
        auto [aggregated, e] = r->Aggregate({ag::WindowStart(timeCol), ag::First(valueCol).SetTransformations({tr::Factor(2.)})})->Bow();
        CHECK(bool(e) && e.msg.find("factor: invalid type bool") != std::string::npos);
    }
    printf("%d checks, %d failures\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
