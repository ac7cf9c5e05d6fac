// test_equal.cpp — Bow::EqualOnDevice against the mirror's host loop Bow::Equal (bow.go:227-275), and IsColEmpty / GetPrevRowIndex /
// GetNextRowIndex / GetPrevValue(s) / GetNextValue(s) against the reference's loops (bowgetters.go:65-151, bowassertion.go:84-86) written
// out here over the mirror's GetValue, through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp), i.e. through the C ABI
// and the HIP kernels.  Needs a GPU (run by tests/test_gpu_equal.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// ---- the reference's loops, statement by statement
static std::pair<Value, int> RefPrevValue(const Bow &b, int colIndex, int rowIndex) {   // bowgetters.go:67-77
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        Value value = b.GetValue(colIndex, rowIndex);
        if (value) return {value, rowIndex};
        rowIndex--;
    }
    return {Nil(), -1};
}
static std::pair<Value, int> RefNextValue(const Bow &b, int colIndex, int rowIndex) {   // bowgetters.go:81-91
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        Value value = b.GetValue(colIndex, rowIndex);
        if (value) return {value, rowIndex};
        rowIndex++;
    }
    return {Nil(), -1};
}
static std::tuple<Value, Value, int> RefPrevValues(const Bow &b, int colIndex1, int colIndex2, int rowIndex) {   // bowgetters.go:95-107
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        Value v1;
        std::tie(v1, rowIndex) = RefPrevValue(b, colIndex1, rowIndex);
        auto [v2, rowIndex2] = RefPrevValue(b, colIndex2, rowIndex);
        if (rowIndex == rowIndex2) return {v1, v2, rowIndex};
        rowIndex--;
    }
    return {Nil(), Nil(), -1};
}
static std::tuple<Value, Value, int> RefNextValues(const Bow &b, int colIndex1, int colIndex2, int rowIndex) {   // bowgetters.go:111-123
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        Value v1;
        std::tie(v1, rowIndex) = RefNextValue(b, colIndex1, rowIndex);
        auto [v2, rowIndex2] = RefNextValue(b, colIndex2, rowIndex);
        if (rowIndex == rowIndex2) return {v1, v2, rowIndex};
        rowIndex++;
    }
    return {Nil(), Nil(), -1};
}
static int RefPrevRowIndex(const Bow &b, int colIndex, int rowIndex) {   // bowgetters.go:127-137
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        if (b.cols[colIndex].IsValid(rowIndex)) return rowIndex;
        rowIndex--;
    }
    return -1;
}
static int RefNextRowIndex(const Bow &b, int colIndex, int rowIndex) {   // bowgetters.go:141-151
    while (rowIndex >= 0 && rowIndex < b.NumRows()) {
        if (b.cols[colIndex].IsValid(rowIndex)) return rowIndex;
        rowIndex++;
    }
    return -1;
}

// two boxed values as the tests compare them: nil with nil, else the same type and the same bits (a NaN is itself here)
static bool SameValue(const Value &a, const Value &b) {
    if (!a || !b) return !a && !b;
    if (a->index() != b->index()) return false;
    if (std::holds_alternative<double>(*a)) {
        const double x = std::get<double>(*a), y = std::get<double>(*b);
        return memcmp(&x, &y, 8) == 0;
    }
    return *a == *b;
}

static std::shared_ptr<Bow> Frame(int n, uint32_t seed, double p_null) {
    auto b = std::make_shared<Bow>();
    std::vector<int64_t> iv((size_t)n);
    std::vector<double> fv((size_t)n);
    std::vector<int> bv((size_t)n);
    std::vector<bool> v0((size_t)n), v1((size_t)n), v2((size_t)n);
    uint32_t s = seed;
    auto next = [&s]() { s = s * 1664525u + 1013904223u; return (s >> 8) / (double)(1u << 24); };
    for (int i = 0; i < n; i++) {
        iv[(size_t)i] = (int64_t)(next() * 1000) - 500;
        fv[(size_t)i] = next() * 8 - 4;
        bv[(size_t)i] = next() < 0.5;
        v0[(size_t)i] = next() >= p_null;
        v1[(size_t)i] = next() >= p_null;
        v2[(size_t)i] = next() >= p_null;
    }
    b->cols.push_back(NewSeries("time", Type::Int64, iv, v0));
    b->cols.push_back(NewSeries("value", Type::Float64, fv, v1));
    b->cols.push_back(NewSeries("flag", Type::Boolean, bv, v2));
    return b;
}

static void SetFloat(Bow &b, int col, int row, double x, bool valid = true) {
    memcpy(&b.cols[(size_t)col].data[(size_t)row], &x, 8);
    uint8_t &byte = b.cols[(size_t)col].validity[(size_t)(row >> 3)];
    byte = valid ? (uint8_t)(byte | (1u << (row & 7))) : (uint8_t)(byte & ~(1u << (row & 7)));
}

// EqualOnDevice in the reference's mode is what the host loop says
static void CheckAgainstHost(const Bow &a, const Bow &b, bool want) {
    auto [got, err] = a.EqualOnDevice(b);
    CHECK(!err);
    if (err) printf("  %s\n", err.msg.c_str());
    CHECK(got == a.Equal(b));
    CHECK(got == want);
}

static void TestEqual() {
    for (int n : {1, 64, 300, 5000}) {
        g_test = "equal n=" + std::to_string(n);
        auto a = Frame(n, 17, 0.3);
        {
            Bow b = *a;
            CheckAgainstHost(*a, b, true);
            auto [bits, err] = a->EqualOnDevice(b, BOWGPU_EQUAL_BITS);
            CHECK(!err && bits);
        }
        const int row = n - 1;
        {   // one value off
            Bow b = *a;
            SetFloat(*a, 1, row, 1.25);
            b = *a;
            SetFloat(b, 1, row, 1.5);
            CheckAgainstHost(*a, b, false);
            int64_t x = 77;
            b = *a;
            b.cols[0].validity[0] |= 1;
            Bow a2 = b;
            memcpy(&b.cols[0].data[0], &x, 8);
            x = 78;
            memcpy(&a2.cols[0].data[0], &x, 8);
            CheckAgainstHost(a2, b, false);
            b = a2;
            b.cols[2].validity[0] |= 1;
            a2 = b;
            b.cols[2].data[0] = !b.cols[2].data[0];
            CheckAgainstHost(a2, b, false);
        }
        {   // one null off; a value that differs under a null on both sides is no difference
            Bow b = *a;
            SetFloat(b, 1, row, 1.25, false);
            CheckAgainstHost(*a, b, false);
            Bow a2 = b;
            SetFloat(a2, 1, row, -9.0, false);
            CheckAgainstHost(a2, b, true);
        }
        {   // NaN: the frame differs from itself under the reference's rule, not bit for bit
            Bow b = *a;
            SetFloat(b, 1, row, std::numeric_limits<double>::quiet_NaN());
            CheckAgainstHost(b, b, false);
            auto [bits, err] = b.EqualOnDevice(b, BOWGPU_EQUAL_BITS);
            CHECK(!err && bits);
        }
        {   // -0.0 against +0.0
            Bow x = *a, y = *a;
            SetFloat(x, 1, row, -0.0);
            SetFloat(y, 1, row, 0.0);
            CheckAgainstHost(x, y, true);
            auto [bits, err] = x.EqualOnDevice(y, BOWGPU_EQUAL_BITS);
            CHECK(!err && !bits);
        }
        {   // names differ; types differ; another number of columns
            Bow b = *a;
            b.cols[1].Name = "other";
            CheckAgainstHost(*a, b, false);
            b = *a;
            b.cols[1].typ = Type::Int64;
            CheckAgainstHost(*a, b, false);
            b = *a;
            b.cols.pop_back();
            CheckAgainstHost(*a, b, false);
        }
    }
    g_test = "equal empty";
    Bow e;
    CheckAgainstHost(e, e, true);
    auto z = Frame(5, 3, 0.3)->NewEmptySlice();
    CheckAgainstHost(*z, *z, true);
}

static void TestGetters() {
    for (int n : {1, 63, 65, 700, 9000}) {
        for (double p_null : {0.0, 0.5, 0.97, 1.0}) {
            g_test = "getters n=" + std::to_string(n) + " p=" + std::to_string(p_null);
            auto b = Frame(n, (uint32_t)n + 5, p_null);
            for (int c = 0; c < 3; c++) CHECK(b->IsColEmpty(c) == (b->cols[(size_t)c].NullN() == b->cols[(size_t)c].length));
            for (int start : {-1, 0, n / 3, n / 2, n - 1, n, n + 4}) {
                for (int c = 0; c < 3; c++) {
                    CHECK(b->GetPrevRowIndex(c, start) == RefPrevRowIndex(*b, c, start));
                    CHECK(b->GetNextRowIndex(c, start) == RefNextRowIndex(*b, c, start));
                    auto got = b->GetPrevValue(c, start), want = RefPrevValue(*b, c, start);
                    CHECK(got.second == want.second && SameValue(got.first, want.first));
                    got = b->GetNextValue(c, start), want = RefNextValue(*b, c, start);
                    CHECK(got.second == want.second && SameValue(got.first, want.first));
                }
                for (auto pair : {std::pair<int, int>{0, 1}, {1, 2}, {2, 0}, {1, 1}}) {
                    auto got = b->GetPrevValues(pair.first, pair.second, start), want = RefPrevValues(*b, pair.first, pair.second, start);
                    CHECK(std::get<2>(got) == std::get<2>(want) && SameValue(std::get<0>(got), std::get<0>(want)) && SameValue(std::get<1>(got), std::get<1>(want)));
                    got = b->GetNextValues(pair.first, pair.second, start), want = RefNextValues(*b, pair.first, pair.second, start);
                    CHECK(std::get<2>(got) == std::get<2>(want) && SameValue(std::get<0>(got), std::get<0>(want)) && SameValue(std::get<1>(got), std::get<1>(want)));
                }
            }
        }
    }
    g_test = "is col empty, zero rows";
    auto z = Frame(5, 3, 0.3)->NewEmptySlice();
    CHECK(z->IsColEmpty(0));
}

int main() {
    TestEqual();
    TestGetters();
    printf("%d failures, %d checks\n", g_fail, g_checks);
    return g_fail ? 1 : 0;
}
