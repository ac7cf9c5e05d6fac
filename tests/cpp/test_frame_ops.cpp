// test_frame_ops.cpp — the reference's tests of Bow.DropNils (bow_test.go:165-285), Bow.Diff (bowdiff_test.go:10-94) and Bow.Distinct
// (bowgetters_test.go:34-69), read from tests/golden/frame_ops_vectors.json and replayed through the C++ mirror of its interface
// (bow_amd/host/bow_rolling.hpp), i.e. through the C ABI and the HIP kernels.  Needs a GPU (run by tests/test_gpu_frame_ops.py).
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
    [[noreturn]] void die(const char *what) { printf("frame_ops_vectors.json: %s at byte %zu\n", what, i); exit(2); }
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
    std::ifstream f(dir + "/frame_ops_vectors.json");
    if (!f) { printf("cannot open %s/frame_ops_vectors.json\n", dir.c_str()); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const J doc = Parser(text).value();
    int ran = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = c["name"].str + " (" + c["source"].str + ")";
        const BowPtr b = frame(c["cols"]);
        CHECK(b != nullptr);
        if (!b) continue;
        std::vector<int> idx;
        if (c.has("col_idx"))
            for (const J &x : c["col_idx"].arr) idx.push_back((int)x.inum);
        const std::string op = c["op"].str;
        std::pair<BowPtr, Error> r = op == "drop_nils" ? b->DropNils(idx) : op == "diff" ? b->Diff(idx) : b->Distinct((int)c["col"].inum);
        ran++;
        if (c.has("error")) {
            CHECK((bool)r.second && r.first == nullptr);
            continue;
        }
        CHECK(!r.second);
        if (r.second) { printf("   error: %s\n", r.second.msg.c_str()); continue; }
        expect_equal(r.first, frame(c["expected"]));
        if (c.has("unchanged") && c["unchanged"].b) CHECK(r.first == b);   // the receiver itself (bow.go:210-212)
        if (c.has("unchanged") && !c["unchanged"].b) CHECK(r.first != b);
        for (const Series &s : r.first->cols)
            for (int64_t row = 0; row < s.length; row++)
                if (!s.IsValid(row)) CHECK(s.data[(size_t)row] == 0);   // null slots hold 0 (Buffer.SetOrDropStrict on a fresh buffer)
    }
    CHECK(ran == 13);
    {   // a long-format frame on its way to a rolling call: the series it holds, its rows without a value, per-step consumption
        g_test = "DropNils + Diff + Distinct";
        const BowPtr b = NewBowFromColBasedInterfaces({"time", "sensor", "index"}, {Int64, Int64, Float64},
                                                      {{I(10), I(11), I(12), I(13), I(14), I(15)},
                                                       {I(7), I(3), I(7), N, I(3), I(7)},
                                                       {F(1.5), F(2.5), N, F(4.5), F(6.5), F(-0.0)}}).first;
        auto [d, e1] = b->Distinct(1);
        CHECK(!e1);
        if (!e1) expect_equal(d, NewBowFromColBasedInterfaces({"sensor"}, {Int64}, {{I(3), I(7)}}).first);
        auto [k, e2] = b->DropNils({2, 2});   // a repeated index is the same as naming it once
        CHECK(!e2);
        const BowPtr want = NewBowFromColBasedInterfaces({"time", "sensor", "index"}, {Int64, Int64, Float64},
                                                         {{I(10), I(11), I(13), I(14), I(15)}, {I(7), I(3), N, I(3), I(7)},
                                                          {F(1.5), F(2.5), F(4.5), F(6.5), F(-0.0)}}).first;
        if (!e2) expect_equal(k, want);
        auto [s, e3] = b->DropNils({1, 2});   // rows 2 and 3 go: two runs
        CHECK(!e3);
        if (!e3) CHECK(s->NumRows() == 4);
        auto [t, e4] = b->NewSlice(0, 2)->DropNils();   // nothing to drop in a slice that shares no shared_ptr with its result
        CHECK(!e4);
        if (!e4) expect_equal(t, b->NewSlice(0, 2));
        auto [df, e5] = want->Diff({0, 2});
        CHECK(!e5);
        if (!e5)
            expect_equal(df, NewBowFromColBasedInterfaces({"time", "sensor", "index"}, {Int64, Int64, Float64},
                                                          {{N, I(1), I(2), I(1), I(1)}, {I(7), I(3), N, I(3), I(7)},
                                                           {N, F(1.0), F(2.0), F(2.0), F(-6.5)}}).first);
        auto [bad, e6] = b->DropNils({3});
        CHECK((bool)e6 && bad == nullptr);
        auto [bad2, e7] = b->Distinct(-1);
        CHECK((bool)e7 && bad2 == nullptr);
    }
    printf("%d checks, %d failures, %d cases of bow_test.go / bowdiff_test.go / bowgetters_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
