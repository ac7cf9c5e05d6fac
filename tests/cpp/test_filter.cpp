// test_filter.cpp — the reference's table-driven test of Bow.Filter (bowsetters_test.go:56-135), read from tests/golden/filter_vectors.json and
// replayed through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp), i.e. through the C ABI and the HIP kernels; plus
// one user closure.  Needs a GPU (run by tests/test_gpu_filter.py).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
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

// ---- just enough JSON for the fixture: objects, arrays, strings without escapes beyond \" and \\, numbers, true / false / null
struct J {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    bool b = false;
    double num = 0;
    bool integral = false;
    int64_t inum = 0;
    std::string str;
    std::vector<J> arr;
    std::map<std::string, J> obj;
    const J &operator[](const std::string &k) const { return obj.at(k); }
    bool has(const std::string &k) const { return obj.count(k) != 0; }
};
struct Parser {
    const std::string &s;
    size_t i = 0;
    explicit Parser(const std::string &text) : s(text) {}
    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) i++; }
    [[noreturn]] void die(const char *what) { printf("filter_vectors.json: %s at byte %zu\n", what, i); exit(2); }
    std::string string() {
        if (s[i] != '"') die("string expected");
        std::string out;
        for (i++; i < s.size() && s[i] != '"'; i++) {
            if (s[i] == '\\') i++;
            out.push_back(s[i]);
        }
        i++;
        return out;
    }
    J value() {
        ws();
        J j;
        if (i >= s.size()) die("unexpected end");
        const char ch = s[i];
        if (ch == '{') {
            j.kind = J::Obj;
            i++;
            for (ws(); s[i] != '}'; ws()) {
                const std::string k = string();
                ws();
                if (s[i] != ':') die("':' expected");
                i++;
                j.obj[k] = value();
                ws();
                if (s[i] == ',') i++;
            }
            i++;
        } else if (ch == '[') {
            j.kind = J::Arr;
            i++;
            for (ws(); s[i] != ']'; ws()) {
                j.arr.push_back(value());
                ws();
                if (s[i] == ',') i++;
            }
            i++;
        } else if (ch == '"') {
            j.kind = J::Str;
            j.str = string();
        } else if (s.compare(i, 4, "null") == 0) {
            i += 4;
        } else if (s.compare(i, 4, "true") == 0) {
            j.kind = J::Bool; j.b = true; i += 4;
        } else if (s.compare(i, 5, "false") == 0) {
            j.kind = J::Bool; i += 5;
        } else {
            const size_t b = i;
            while (i < s.size() && (isdigit((unsigned char)s[i]) || s[i] == '-' || s[i] == '+' || s[i] == '.' || s[i] == 'e' || s[i] == 'E')) i++;
            if (i == b) die("value expected");
            const std::string t = s.substr(b, i - b);
            j.kind = J::Num;
            j.num = strtod(t.c_str(), nullptr);
            j.integral = t.find_first_of(".eE") == std::string::npos;
            if (j.integral) j.inum = strtoll(t.c_str(), nullptr, 10);
        }
        return j;
    }
};

static BowPtr frame(const J &cols) {
    std::vector<std::string> names;
    std::vector<Type> types;
    std::vector<std::vector<Value>> data;
    for (const J &c : cols.arr) {
        names.push_back(c["name"].str);
        const bool is_int = c["type"].str == "int64";
        types.push_back(is_int ? Int64 : Float64);
        std::vector<Value> v;
        for (const J &x : c["data"].arr) {
            if (x.kind == J::Null) v.push_back(N);
            else if (is_int) v.push_back(I(x.inum));
            else v.push_back(F(x.num));
        }
        data.push_back(std::move(v));
    }
    return NewBowFromColBasedInterfaces(names, types, data).first;
}

static void expect_equal(const BowPtr &have, const BowPtr &want) {
    g_checks++;
    if (!have || !have->Equal(*want)) {
        g_fail++;
        printf("FAIL [%s]\n expect:\n%s have:\n%s", g_test.c_str(), want->String().c_str(), have ? have->String().c_str() : "<nil>\n");
    }
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    std::ifstream f(dir + "/filter_vectors.json");
    if (!f) { printf("cannot open %s/filter_vectors.json\n", dir.c_str()); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const J doc = Parser(text).value();
    int ran = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = "Filter/" + c["name"].str + " (" + c["source"].str + ")";
        const BowPtr b = frame(c["cols"]);
        CHECK(b != nullptr);
        if (!b) continue;
        std::vector<RowCmp> cmps;
        for (const J &p : c["preds"].arr) {
            std::vector<FilterArg> values;
            for (const J &v : p["values"].arr) {
                if (v.kind == J::Str) values.push_back(FilterArg(v.str));
                else if (v.integral) values.push_back(FilterArg((long long)v.inum));
                else values.push_back(FilterArg(v.num));
            }
            cmps.push_back(b->MakeFilterValuesV((int)p["col"].inum, values));
        }
        auto [res, err] = b->FilterV(cmps);
        ran++;
        CHECK(!err);
        if (err) { printf("   error: %s\n", err.msg.c_str()); continue; }
        if (c["contiguous"].b) {
            const int first = (int)c["first"].inum, count = (int)c["count"].inum;
            expect_equal(res, count ? b->NewSlice(first, first + count) : b->NewEmptySlice());
            continue;
        }
        expect_equal(res, frame(c["expected"]));
        CHECK(res->NumRows() == (int)c["count"].inum);
    }
    CHECK(ran == 8);
    {   // a user closure beside a built-in comparator: rows with an even time AND sensor 7; nulls dropped with their row
        g_test = "Filter/user closure";
        const BowPtr b = NewBowFromColBasedInterfaces({"time", "sensor", "value"}, {Int64, Int64, Float64},
                                                      {{I(10), I(11), I(12), I(13), I(14), I(16)},
                                                       {I(7), I(7), I(8), I(7), I(7), I(7)},
                                                       {F(1.5), F(2.5), F(3.5), F(4.5), N, F(6.5)}}).first;
        const RowCmp even = [](const Bow &bw, int i) { return bw.GetInt64(0, i).first % 2 == 0; };
        auto [res, err] = b->Filter(even, b->MakeFilterValues(1, 7));
        CHECK(!err);
        const BowPtr want = NewBowFromColBasedInterfaces({"time", "sensor", "value"}, {Int64, Int64, Float64},
                                                         {{I(10), I(14), I(16)}, {I(7), I(7), I(7)}, {F(1.5), N, F(6.5)}}).first;
        if (!err) {
            expect_equal(res, want);
            for (const Series &s : res->cols)
                for (int64_t r = 0; r < s.length; r++)
                    if (!s.IsValid(r)) CHECK(s.data[(size_t)r] == 0);   // null slots hold 0 (Buffer.SetOrDropStrict on a fresh buffer)
        }
        // the closure alone selects consecutive rows 2 .. 2 of a narrower range: a slice
        const RowCmp only12 = [](const Bow &bw, int i) { return bw.GetInt64(0, i).first == 12; };
        auto [r2, e2] = b->Filter(only12);
        CHECK(!e2);
        if (!e2) expect_equal(r2, b->NewSlice(2, 3));
        // a value that is not convertible holds on null rows: the one null of `value`
        auto [r3, e3] = b->Filter(b->MakeFilterValues(2, "x"));
        CHECK(!e3);
        if (!e3) expect_equal(r3, b->NewSlice(4, 5));
        // no comparator: the whole frame
        auto [r4, e4] = b->Filter();
        CHECK(!e4);
        if (!e4) expect_equal(r4, b);
    }
    printf("%d checks, %d failures, %d tables of bowsetters_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
