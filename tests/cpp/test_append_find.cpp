// test_append_find.cpp — the reference's tests of AppendBows (bowappend_test.go:11-176) and Bow.Find / FindNext / Contains
// (bowfind_test.go:9-44), read from tests/golden/append_find_vectors.json and replayed through the C++ mirror of its interface
// (bow_amd/host/bow_rolling.hpp), i.e. through the C ABI and the HIP kernels.  Needs a GPU (run by tests/test_gpu_append_find.py).
#include <cmath>
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
    [[noreturn]] void die(const char *what) { printf("append_find_vectors.json: %s at byte %zu\n", what, i); exit(2); }
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

// one lookup of the fixture on b's only column: a number of the column's type, null for nil, a string for toto(0) - a value boxed
// as a type of its own, which this mirror writes as a value of the OTHER numeric type
static void lookups(const BowPtr &b, const J &list, bool is_int) {
    for (const J &lk : list.arr) {
        const J &v = lk["value"];
        const Value value = v.kind == J::Null ? N : v.kind == J::Str ? (is_int ? F(0.) : I(0)) : is_int ? I(v.inum) : F(v.num);
        const int start = (int)lk["row_start"].inum, want = (int)lk["expect"].inum;
        CHECK(b->FindNext(0, start, value) == want);
        if (start == 0) {
            CHECK(b->Find(0, value) == want);
            CHECK(b->Contains(0, value) == (want != -1));
        }
    }
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    std::ifstream f(dir + "/append_find_vectors.json");
    if (!f) { printf("cannot open %s/append_find_vectors.json\n", dir.c_str()); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const J doc = Parser(text).value();
    int ran = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = c["name"].str + " (" + c["source"].str + ")";
        ran++;
        if (c["op"].str == "find") {
            J one;
            one.kind = J::Arr;
            one.arr.push_back(c["col"]);
            const BowPtr b = frame(one);
            CHECK(b != nullptr);
            if (!b) continue;
            const bool is_int = c["col"]["type"].str == "int64";
            lookups(b, c["lookups"], is_int);
            lookups(b->NewEmptySlice(), c["empty_lookups"], is_int);
            continue;
        }
        std::vector<BowPtr> bows;
        for (const J &fr : c["frames"].arr) bows.push_back(frame(fr));
        std::pair<BowPtr, Error> r = AppendBows(bows);
        if (c.has("error")) {
            CHECK((bool)r.second && r.first == nullptr && r.second.msg == c["error"].str);
            continue;
        }
        CHECK(!r.second);
        if (r.second) { printf("   error: %s\n", r.second.msg.c_str()); continue; }
        expect_equal(r.first, frame(c["expected"]));
        CHECK((r.first == bows[0]) == c["unchanged"].b);   // one bow: the bow itself (bowappend.go:19-21)
        for (const Series &s : r.first->cols)
            for (int64_t row = 0; row < s.length; row++)
                if (!s.IsValid(row)) CHECK(s.data[(size_t)row] == 0);
    }
    CHECK(ran == 7);
    {   // a month of daily pieces, some of them empty, put together and searched by timestamp and for the first missing value
        g_test = "AppendBows + Find";
        const std::vector<std::string> names = {"time", "value"};
        const std::vector<Type> types = {Int64, Float64};
        const BowPtr d1 = NewBowFromColBasedInterfaces(names, types, {{I(10), I(11), I(12)}, {F(1.5), N, F(-0.0)}}).first;
        const BowPtr d2 = NewBowFromColBasedInterfaces(names, types, {{}, {}}).first;
        const BowPtr d3 = NewBowFromColBasedInterfaces(names, types, {{I(13), I(14)}, {F(0.0), F(1.5)}}).first;
        auto [none, e0] = AppendBows({});   // no bows: nil and no error (bowappend.go:15-17)
        CHECK(!e0 && none == nullptr);
        auto [all, e1] = AppendBows({d2, d1, d2, d3, d2});
        CHECK(!e1);
        if (!e1) {
            expect_equal(all, NewBowFromColBasedInterfaces(names, types, {{I(10), I(11), I(12), I(13), I(14)}, {F(1.5), N, F(-0.0), F(0.0), F(1.5)}}).first);
            CHECK(all->Find(0, I(13)) == 3 && all->Contains(0, I(14)) && !all->Contains(0, I(15)));
            CHECK(all->Find(1, N) == 1 && all->FindNext(1, 3, N) == 1);   // nil: from row 0, whatever rowIndex says
            CHECK(all->Find(1, F(0.0)) == 2 && all->FindNext(1, 3, F(-0.0)) == 3);   // -0.0 == +0.0
            CHECK(all->FindNext(1, 1, F(1.5)) == 4 && all->FindNext(1, 5, F(1.5)) == -1);
            CHECK(all->Find(0, F(13.)) == -1 && all->Find(1, I(0)) == -1);   // another type than the column's
            CHECK(all->Find(1, F(std::nan(""))) == -1 && all->Find(0, N) == -1 && all->Find(7, I(1)) == -1);
        }
        auto [empty, e2] = AppendBows({d2, d2});
        CHECK(!e2 && empty && empty->NumRows() == 0 && empty->NumCols() == 2 && empty->ColumnType(1) == Float64);
        // schema mismatches: an error where the reference panics
        const BowPtr narrow = NewBowFromColBasedInterfaces({"time"}, {Int64}, {{I(1)}}).first;
        auto [bad1, e3] = AppendBows({d1, narrow});
        CHECK((bool)e3 && bad1 == nullptr);
        auto [bad2, e4] = AppendBows({d1, nullptr});
        CHECK((bool)e4 && bad2 == nullptr);
        const BowPtr ints = NewBowFromColBasedInterfaces(names, {Int64, Int64}, {{I(1)}, {I(1)}}).first;
        auto [bad3, e5] = AppendBows({d1, d3, ints});
        CHECK((bool)e5 && bad3 == nullptr && e5.msg == "incompatible types 'float64' and 'int64'");
    }
    printf("%d checks, %d failures, %d cases of bowappend_test.go / bowfind_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
