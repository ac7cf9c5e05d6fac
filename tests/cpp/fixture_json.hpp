// fixture_json.hpp — what a C++ test needs to read a fixture of tests/golden: a small JSON reader and the fixture's column-based frames
// as bow::Bow.  (The earlier tests each carry their own copy of the reader; new ones include this.)
#pragma once

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../bow_amd/host/bow_rolling.hpp"

namespace fixture {
using namespace bow;

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
    [[noreturn]] void die(const char *what) { printf("fixture: %s at byte %zu\n", what, i); exit(2); }
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

inline J load(const std::string &path) {
    std::ifstream f(path);
    if (!f) { printf("cannot open %s\n", path.c_str()); exit(2); }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    return Parser(text).value();
}

// [{"name", "type": "int64" | "float64", "data": [number | null, ...]}, ...] -> a Bow
inline BowPtr frame(const J &cols) {
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
}  // namespace fixture
