// test_sort.cpp — the reference's table-driven tests of Bow.SortByCol (bowsort_test.go:11-204), read from tests/golden/sort_vectors.json and
// replayed through the C++ mirror of its interface (bow_amd/host/bow_rolling.hpp), i.e. through the C ABI and the HIP kernels.
// Needs a GPU (run by tests/test_gpu_sort.py).
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
    [[noreturn]] void die(const char *what) { printf("sort_vectors.json: %s at byte %zu\n", what, i); exit(2); }
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

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    std::ifstream f(dir + "/sort_vectors.json");
    if (!f) { printf("cannot open %s/sort_vectors.json\n", dir.c_str()); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const J doc = Parser(text).value();
    int ran = 0;
    for (const J &c : doc["cases"].arr) {
        g_test = "SortByCol/" + c["name"].str + " (" + c["source"].str + ")";
        const BowPtr b = frame(c["cols"]);
        CHECK(b != nullptr);
        if (!b) continue;
        auto [sorted, err] = b->SortByCol((int)c["key_col"].inum);
        ran++;
        if (c.has("error")) {
            CHECK((bool)err);
            CHECK(sorted == nullptr);
            CHECK(err.msg == c["error"]["message"].str);
            continue;
        }
        CHECK(!err);
        if (err) { printf("   error: %s\n", err.msg.c_str()); continue; }
        if (c.has("unchanged")) {
            CHECK(sorted.get() == b.get());   // the receiver itself (bowsort.go:19-21)
            continue;
        }
        const BowPtr want = frame(c["expected"]);
        g_checks++;
        if (!sorted || !sorted->Equal(*want)) {
            g_fail++;
            printf("FAIL [%s]\n expect:\n%s have:\n%s", g_test.c_str(), want->String().c_str(), sorted ? sorted->String().c_str() : "<nil>\n");
        }
        CHECK(sorted->IsColSorted((int)c["key_col"].inum));
        for (int i = 0; i < sorted->NumCols(); i++) {   // null slots hold 0 (Buffer.SetOrDropStrict on a fresh buffer)
            const Series &s = sorted->cols[(size_t)i];
            for (int64_t r = 0; r < s.length; r++)
                if (!s.IsValid(r)) CHECK(s.data[(size_t)r] == 0);
        }
    }
    {   // a column index outside the Bow
        g_test = "SortByCol/bad column";
        const BowPtr b = NewBowFromColBasedInterfaces({"time"}, {Int64}, {{I(2), I(1)}}).first;
        auto [s1, e1] = b->SortByCol(1);
        CHECK((bool)e1 && s1 == nullptr);
        auto [s2, e2] = b->SortByCol(-1);
        CHECK((bool)e2 && s2 == nullptr);
    }
    CHECK(ran == 9);
    printf("%d checks, %d failures, %d tables of bowsort_test.go\n", g_checks, g_fail, ran);
    return g_fail ? 1 : 0;
}
