// bow_rolling.hpp — C++ mirror of the reference's Go interface for the rolling path, above the C ABI.
//
// The reference is Go (no Go toolchain in this image), so the host side above include/bowgpu.h is
// written in C++ with the SAME names, argument meaning and error strings as the reference:
//   bow::Bow / Series / Type, AppendBows       <- bow.go, bowseries.go, bowtypes.go, bowappend.go, bowfind.go, bowjoin.go,
//                                                  bowsetters.go (Filter, Convert)
//   bow::rolling::IntervalRolling, Rolling, Options, Window, ColAggregation, NewColAggregation,
//        ColInterpolation, NewColInterpolation  <- rolling/rolling.go, window.go, aggregation.go, interpolation.go
//   bow::rolling::aggregation::{WindowStart,Sum,ArithmeticMean,Min,Max,Count,First,Last,Mode,IntegralStep,
//        IntegralTrapezoid,WeightedAverageStep,WeightedAverageLinear}   <- rolling/aggregation/*.go
//   bow::rolling::interpolation::{WindowStart,Linear,StepPrevious,None} <- rolling/interpolation/*.go
//   bow::rolling::transformation::Factor                                 <- rolling/transformation/factor.go
// Go's (value, error) returns become std::pair<T, Error>; interface{} becomes bow::Value.
//
// Everything that touches column data goes through libbowgpu.so (HIP kernels).  The only host loops are
// the user's OWN closures (NewColAggregation with a custom func), which are called per window with
// Window slices whose row ranges come from the device (bowgpu_window_bounds).
#pragma once

#include <stdint.h>
#include <string.h>

#include <errno.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <optional>
#include <sstream>
#include <string>
#include <tuple>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/bowgpu.h"

namespace bow {

// ----------------------------------------------------------------------------- errors, values, types
struct Error {
    bool set = false;
    std::string msg;
    Error() = default;
    explicit Error(std::string m) : set(true), msg(std::move(m)) {}
    explicit operator bool() const { return set; }
    const std::string &Error_() const { return msg; }
};
inline Error Errorf(const std::string &m) { return Error(m); }
inline Error Wrap(const std::string &prefix, const Error &e) { return Error(prefix + ": " + e.msg); }

using Scalar = std::variant<int64_t, double, bool>;
using Value = std::optional<Scalar>;  // interface{}: nil | int64 | float64 | bool
inline Value Nil() { return std::nullopt; }

enum class Type : int32_t { Unknown = 0, Float64 = 1, Int64 = 2, Boolean = 3, String = 4, InputDependent = 5, IteratorDependent = 6 };
constexpr Type Float64 = Type::Float64, Int64 = Type::Int64, Boolean = Type::Boolean, String = Type::String,
               InputDependent = Type::InputDependent, IteratorDependent = Type::IteratorDependent;

inline std::string TypeString(Type t) {  // bowtypes.go:89-96 (arrow type names)
    switch (t) {
    case Type::Float64: return "float64";
    case Type::Int64: return "int64";
    case Type::Boolean: return "bool";
    case Type::String: return "utf8";
    default: return "undefined";
    }
}

inline int64_t GoInt64(double x) {  // float64 -> int64 on amd64
    if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return INT64_MIN;
    return (int64_t)x;
}

// ----------------------------------------------------------------------------- Series / Bow
struct Series {
    std::string Name;
    Type typ = Type::Unknown;
    std::vector<uint64_t> data;     // 8-byte slots: int64 or float64 bit patterns (Arrow values buffer); a Boolean series holds 0 / 1
    mutable std::vector<uint8_t> arrow_bits;   // a Boolean series as Arrow holds it - bit i, LSB first - packed by Bow::ArrowCol for the C ABI
    std::vector<uint8_t> validity;  // Arrow LSB-first bitmap, ceil(n/8) bytes (bowseries.go:191-220)
    int64_t length = 0;

    bool IsValid(int64_t i) const { return (validity[i >> 3] >> (i & 7)) & 1; }
    int64_t NullN() const {
        int64_t c = 0;
        for (int64_t i = 0; i < length; i++) c += !IsValid(i);
        return c;
    }
};

inline Series NewSeriesRaw(const std::string &name, Type typ, std::vector<uint64_t> data, std::vector<uint8_t> validity) {
    Series s;
    s.Name = name; s.typ = typ; s.length = (int64_t)data.size(); s.data = std::move(data); s.validity = std::move(validity);
    s.validity.resize((size_t)((s.length + 7) / 8));
    return s;
}

// NewSeries(name, typ, dataArray, validityArray): validity empty => all valid (bowseries.go:27-29, :196-200)
template <typename T>
inline Series NewSeries(const std::string &name, Type typ, const std::vector<T> &values, const std::vector<bool> &valid = {}) {
    std::vector<uint64_t> d(values.size());
    for (size_t i = 0; i < values.size(); i++) {
        if (typ == Type::Int64) { int64_t v = (int64_t)values[i]; memcpy(&d[i], &v, 8); }
        else if (typ == Type::Boolean) d[i] = values[i] ? 1 : 0;
        else { double v = (double)values[i]; memcpy(&d[i], &v, 8); }
    }
    std::vector<uint8_t> bm((values.size() + 7) / 8, 0);
    for (size_t i = 0; i < values.size(); i++)
        if (valid.empty() || valid[i]) bm[i >> 3] |= (uint8_t)(1u << (i & 7));
    return NewSeriesRaw(name, typ, std::move(d), std::move(bm));
}

class Bow;
using BowPtr = std::shared_ptr<const Bow>;

// one argument of MakeFilterValues (an interface{} there): nil, a number, a bool or a string
struct FilterArg {
    enum Kind { KNil, KInt, KFloat, KBool, KStr } kind = KNil;
    int64_t i = 0;
    double f = 0;
    bool b = false;
    std::string s;
    FilterArg() = default;
    FilterArg(int v) : kind(KInt), i(v) {}
    FilterArg(long v) : kind(KInt), i(v) {}
    FilterArg(long long v) : kind(KInt), i(v) {}
    FilterArg(float v) : kind(KFloat), f(v) {}
    FilterArg(double v) : kind(KFloat), f(v) {}
    FilterArg(bool v) : kind(KBool), b(v) {}
    FilterArg(const char *v) : kind(KStr), s(v) {}
    FilterArg(std::string v) : kind(KStr), s(std::move(v)) {}
    FilterArg(const Value &v) {
        if (!v) return;
        if (std::holds_alternative<int64_t>(*v)) { kind = KInt; i = std::get<int64_t>(*v); }
        else if (std::holds_alternative<double>(*v)) { kind = KFloat; f = std::get<double>(*v); }
        else { kind = KBool; b = std::get<bool>(*v); }
    }
};
// Type.Convert for the numeric column types (bowtypes.go:64-81, bowconvert.go:11-73): numbers, bools and numeric strings; anything
// else becomes nil
Value Convert(Type t, const FilterArg &a);

// RowCmp: bowsetters.go:58-61.  Either a user closure over (bow, row) or what MakeFilterValues prepares: a column, the converted
// values and whether one of them became nil (the comparator then holds on null rows) - the form the device evaluates
struct RowCmp {
    std::function<bool(const Bow &, int)> fn;   // set: a user closure
    int col = -1;
    Type typ = Type::Unknown;
    std::vector<uint64_t> values;               // 64-bit payloads of `typ`
    bool match_null = false;
    RowCmp() = default;
    template <typename Fn, typename = decltype(std::declval<Fn &>()(std::declval<const Bow &>(), 0))>
    RowCmp(Fn f) : fn(std::move(f)) {}
};

class Bow : public std::enable_shared_from_this<Bow> {
  public:
    std::vector<Series> cols;
    // a slice shares nothing here (copies): slices are only made for the user's closures
    int NumCols() const { return (int)cols.size(); }
    int NumRows() const { return cols.empty() ? 0 : (int)cols[0].length; }
    const std::string &ColumnName(int i) const { return cols[i].Name; }
    Type ColumnType(int i) const { return cols[i].typ; }

    // ColumnIndex: bowgetters.go:320-331
    std::pair<int, Error> ColumnIndex(const std::string &name) const {
        int found = -1, n = 0;
        for (int i = 0; i < NumCols(); i++)
            if (cols[i].Name == name) { if (found < 0) found = i; n++; }
        if (n == 0) return {-1, Errorf("no column '" + name + "'")};
        if (n > 1) return {-1, Errorf("several columns '" + name + "'")};
        return {found, Error()};
    }

    // GetValue: bowgetters.go:46-63
    Value GetValue(int col, int row) const {
        const Series &s = cols[col];
        if (row < 0 || row >= s.length || !s.IsValid(row)) return Nil();
        if (s.typ == Type::Int64) { int64_t v; memcpy(&v, &s.data[row], 8); return Scalar(v); }
        if (s.typ == Type::Boolean) return Scalar(s.data[row] != 0);
        double v; memcpy(&v, &s.data[row], 8); return Scalar(v);
    }
    // GetFloat64: bowgetters.go:218-247
    std::pair<double, bool> GetFloat64(int col, int row) const {
        const Series &s = cols[col];
        if (row < 0 || row >= s.length) return {0., false};
        if (s.typ == Type::Int64) { int64_t v; memcpy(&v, &s.data[row], 8); return {(double)v, s.IsValid(row)}; }
        if (s.typ == Type::Boolean) return {s.data[row] != 0 ? 1. : 0., s.IsValid(row)};   // ToFloat64 of a bool (bowconvert.go)
        double v; memcpy(&v, &s.data[row], 8); return {v, s.IsValid(row)};
    }
    std::pair<int64_t, bool> GetInt64(int col, int row) const {
        const Series &s = cols[col];
        if (row < 0 || row >= s.length) return {0, false};
        if (s.typ == Type::Int64) { int64_t v; memcpy(&v, &s.data[row], 8); return {v, s.IsValid(row)}; }
        double v; memcpy(&v, &s.data[row], 8); return {GoInt64(v), s.IsValid(row)};
    }

    // NewSlice: bow.go:279-283
    BowPtr NewSlice(int i, int j) const {
        auto b = std::make_shared<Bow>();
        for (const Series &s : cols) {
            Series t;
            t.Name = s.Name; t.typ = s.typ; t.length = j - i;
            t.data.assign(s.data.begin() + i, s.data.begin() + j);
            t.validity.assign((size_t)((t.length + 7) / 8), 0);
            for (int r = i; r < j; r++)
                if (s.IsValid(r)) t.validity[(r - i) >> 3] |= (uint8_t)(1u << ((r - i) & 7));
            b->cols.push_back(std::move(t));
        }
        return b;
    }
    BowPtr NewEmptySlice() const { return NewSlice(0, 0); }

    // Equal: bow.go:227-275 (schema + per-row values; floats compared exactly)
    bool Equal(const Bow &o) const {
        if (NumCols() != o.NumCols() || NumRows() != o.NumRows()) return false;
        for (int c = 0; c < NumCols(); c++) {
            if (cols[c].Name != o.cols[c].Name || cols[c].typ != o.cols[c].typ) return false;
            for (int r = 0; r < NumRows(); r++) {
                Value a = GetValue(c, r), b = o.GetValue(c, r);
                if (a.has_value() != b.has_value()) return false;
                if (a && *a != *b) return false;
            }
        }
        return true;
    }

    std::string String() const {
        std::ostringstream os;
        for (int c = 0; c < NumCols(); c++) {
            os << cols[c].Name << ":" << TypeString(cols[c].typ) << " [";
            for (int r = 0; r < NumRows(); r++) {
                Value v = GetValue(c, r);
                if (r) os << " ";
                if (!v) os << "<nil>";
                else if (std::holds_alternative<int64_t>(*v)) os << std::get<int64_t>(*v);
                else if (std::holds_alternative<double>(*v)) os << std::get<double>(*v);
                else os << (std::get<bool>(*v) ? "true" : "false");
            }
            os << "]\n";
        }
        return os.str();
    }

    // Arrow view of a column for the C ABI (what b.ArrowRecord().Column(i).Data() exposes: bow.go:183-186)
    bowgpu_col ArrowCol(int i) const {
        const Series &s = cols[i];
        bowgpu_col c;
        memset(&c, 0, sizeof c);
        c.values = s.data.empty() ? nullptr : s.data.data();
        if (s.typ == Type::Boolean) {   // the library reads Arrow bits, not slots
            s.arrow_bits.assign((size_t)((s.length + 7) / 8), 0);
            for (int64_t r = 0; r < s.length; r++)
                if (s.data[(size_t)r]) s.arrow_bits[(size_t)(r >> 3)] |= (uint8_t)(1u << (r & 7));
            c.values = s.arrow_bits.empty() ? nullptr : s.arrow_bits.data();
        }
        c.validity = s.validity.empty() ? nullptr : s.validity.data();
        c.offset = 0; c.length = s.length; c.null_count = s.NullN();
        c.type = (int32_t)s.typ; c.residency = BOWGPU_HOST;
        return c;
    }

    // FillLinear: bowfill.go:14-103 (device) ; IsColSorted: bowassertion.go:15-81 (device)
    std::pair<BowPtr, Error> FillLinear(int refColIndex, int toFillColIndex) const;
    bool IsColSorted(int colIndex) const;
    // FillPrevious / FillNext: bowfill.go:162-253 ; FillMean: bowfill.go:105-160 (device; colIndices defaults to all columns)
    std::pair<BowPtr, Error> FillPrevious(std::vector<int> colIndices = {}) const { return fill(BOWGPU_FILL_PREVIOUS, colIndices); }
    std::pair<BowPtr, Error> FillNext(std::vector<int> colIndices = {}) const { return fill(BOWGPU_FILL_NEXT, colIndices); }
    std::pair<BowPtr, Error> FillMean(std::vector<int> colIndices = {}) const { return fill(BOWGPU_FILL_MEAN, colIndices); }
    // SortByCol: bowsort.go:10-41 (device; stable); returns the receiver when the column is already sorted
    std::pair<BowPtr, Error> SortByCol(int colIndex) const;
    // MakeFilterValues: bowsetters.go:111-132 ; Filter: bowsetters.go:63-100 (device).  Built-in comparators are evaluated by
    // bowgpu_filter; user closures are evaluated here into a row bitmap that the call ANDs in.  Consecutive selected rows come back as
    // a slice of the receiver, none as the empty slice.  (The reference's Filter returns a Bow alone and panics; the Error carries
    // what the device path can answer, e.g. no device.)
    RowCmp MakeFilterValuesV(int colIndex, const std::vector<FilterArg> &values) const;
    template <typename... V> RowCmp MakeFilterValues(int colIndex, V... values) const;
    std::pair<BowPtr, Error> FilterV(const std::vector<RowCmp> &cmps) const;
    template <typename... C> std::pair<BowPtr, Error> Filter(const C &...cmps) const;
    // DropNils: bow.go:188-224 ; Diff: bowdiff.go:8-73 ; Distinct: bowgetters.go:333-358 (device; colIndices defaults to all columns).
    // DropNils returns the receiver when nothing is dropped, a slice when the kept rows are consecutive.  (The reference's Distinct
    // returns a Bow alone and panics; the Error carries what the device path can answer, e.g. a NaN in the column.)
    std::pair<BowPtr, Error> DropNils(std::vector<int> colIndices = {}) const;
    std::pair<BowPtr, Error> Diff(std::vector<int> colIndices = {}) const;
    std::pair<BowPtr, Error> Distinct(int colIndex) const;
    // Convert: bowsetters.go:52-56 (device, among Int64, Float64 and Boolean): the receiver with that column converted, names kept as
    // Apply keeps them.  A String source or target is an Error that says so: the reference's own loop serves those.
    std::pair<BowPtr, Error> Convert(int colIndex, Type t) const;
    // Find / FindNext / Contains: bowfind.go:3-32 (device).  nil finds the first null row, whatever rowIndex says, as the reference
    // does; a value boxed as another type than the column's finds nothing, without a device call (bowfind_test.go:31-32).  A failed
    // device call (e.g. no device) finds nothing: the reference's signature has no error to carry it.
    int Find(int colIndex, const Value &value) const { return FindNext(colIndex, 0, value); }
    int FindNext(int colIndex, int rowIndex, const Value &value) const;
    bool Contains(int colIndex, const Value &value) const { return Find(colIndex, value) != -1; }
    // Equal on the device: the number of columns, names and types are compared here (this mirror models no Arrow metadata), the rows by
    // bowgpu_equal.  mode BOWGPU_EQUAL_GO is what Equal above computes; BOWGPU_EQUAL_BITS compares the 64-bit patterns.
    std::pair<bool, Error> EqualOnDevice(const Bow &o, int mode = BOWGPU_EQUAL_GO) const;
    // IsColEmpty: bowassertion.go:84-86 ; GetPrevRowIndex / GetNextRowIndex / GetPrevValue(s) / GetNextValue(s): bowgetters.go:65-151
    // (device: bowgpu_is_col_empty, bowgpu_valid_row; the value(s) at the row found come from GetValue).  A failed device call (e.g. no
    // device) finds nothing: the reference's signatures have no error to carry it.
    bool IsColEmpty(int colIndex) const;
    int GetPrevRowIndex(int colIndex, int rowIndex) const { return validRow({colIndex}, rowIndex, -1); }
    int GetNextRowIndex(int colIndex, int rowIndex) const { return validRow({colIndex}, rowIndex, +1); }
    std::pair<Value, int> GetPrevValue(int colIndex, int rowIndex) const {
        const int r = validRow({colIndex}, rowIndex, -1);
        return {r < 0 ? Nil() : GetValue(colIndex, r), r};
    }
    std::pair<Value, int> GetNextValue(int colIndex, int rowIndex) const {
        const int r = validRow({colIndex}, rowIndex, +1);
        return {r < 0 ? Nil() : GetValue(colIndex, r), r};
    }
    std::tuple<Value, Value, int> GetPrevValues(int colIndex1, int colIndex2, int rowIndex) const {
        const int r = validRow({colIndex1, colIndex2}, rowIndex, -1);
        return {r < 0 ? Nil() : GetValue(colIndex1, r), r < 0 ? Nil() : GetValue(colIndex2, r), r};
    }
    std::tuple<Value, Value, int> GetNextValues(int colIndex1, int colIndex2, int rowIndex) const {
        const int r = validRow({colIndex1, colIndex2}, rowIndex, +1);
        return {r < 0 ? Nil() : GetValue(colIndex1, r), r < 0 ? Nil() : GetValue(colIndex2, r), r};
    }
    // InnerJoin: bowjoin.go:12-62 ; OuterJoin: bowjoin.go:66-125 (device).  The common columns are found by name as getCommonCols does
    // (bowjoin.go:128-155); none: no pair, an OuterJoin is all left rows then all right rows.  Where the reference panics - a name twice in
    // the right bow, common columns of different types - this returns an Error with the reference's text.  More than one common column
    // is an Error too: these two take one key per side (InnerJoinAll / OuterJoinAll below join on all).  (This mirror models no Arrow
    // metadata.)
    std::pair<BowPtr, Error> InnerJoin(const BowPtr &other) const { return join(other, BOWGPU_JOIN_INNER); }
    std::pair<BowPtr, Error> OuterJoin(const BowPtr &other) const { return join(other, BOWGPU_JOIN_OUTER); }
    // InnerJoinAll / OuterJoinAll: the reference's join as it stands - on EVERY common column (getCommonCols collects them all,
    // getCommonRows bowjoin.go:161-186 calls a row pair common when it agrees on all of them; each key column of a right-only row takes
    // its own right partner's value, bowjoin.go:383-400), through bowgpu_join_keys.  The same Errors; with no or one common column
    // exactly what InnerJoin / OuterJoin return.
    std::pair<BowPtr, Error> InnerJoinAll(const BowPtr &other) const { return join(other, BOWGPU_JOIN_INNER, true); }
    std::pair<BowPtr, Error> OuterJoinAll(const BowPtr &other) const { return join(other, BOWGPU_JOIN_OUTER, true); }

private:
    std::pair<BowPtr, Error> fill(int method, const std::vector<int> &colIndices) const;
    std::pair<BowPtr, Error> join(const BowPtr &other, int32_t kind, bool all_common = false) const;
    int validRow(const std::vector<int> &colIndices, int rowIndex, int direction) const;
};

// NewBow: bow.go:109-116 (all series must have the same length)
inline std::pair<BowPtr, Error> NewBow(std::vector<Series> series) {
    auto b = std::make_shared<Bow>();
    for (size_t i = 1; i < series.size(); i++)
        if (series[i].length != series[0].length) return {nullptr, Errorf("bow.NewBow: Series have different lengths")};
    b->cols = std::move(series);
    return {b, Error()};
}

// NewBowFromColBasedInterfaces: one vector<Value> per column, nil = null
inline std::pair<BowPtr, Error> NewBowFromColBasedInterfaces(const std::vector<std::string> &names, const std::vector<Type> &types,
                                                              const std::vector<std::vector<Value>> &colsv) {
    std::vector<Series> ss;
    for (size_t c = 0; c < names.size(); c++) {
        std::vector<uint64_t> d(colsv[c].size(), 0);
        std::vector<uint8_t> bm((colsv[c].size() + 7) / 8, 0);
        for (size_t r = 0; r < colsv[c].size(); r++) {
            const Value &v = colsv[c][r];
            if (!v) continue;
            if (types[c] == Type::Int64) {
                int64_t x = std::holds_alternative<int64_t>(*v) ? std::get<int64_t>(*v) : GoInt64(std::get<double>(*v));
                memcpy(&d[r], &x, 8);
            } else if (types[c] == Type::Boolean) {
                d[r] = std::holds_alternative<bool>(*v) ? (std::get<bool>(*v) ? 1 : 0) : std::holds_alternative<int64_t>(*v) ? std::get<int64_t>(*v) != 0 : std::get<double>(*v) != 0;
            } else {
                double x = std::holds_alternative<double>(*v) ? std::get<double>(*v) : (double)std::get<int64_t>(*v);
                memcpy(&d[r], &x, 8);
            }
            bm[r >> 3] |= (uint8_t)(1u << (r & 7));
        }
        ss.push_back(NewSeriesRaw(names[c], types[c], std::move(d), std::move(bm)));
    }
    return NewBow(std::move(ss));
}

inline std::pair<BowPtr, Error> NewBowFromRowBasedInterfaces(const std::vector<std::string> &names, const std::vector<Type> &types,
                                                              const std::vector<std::vector<Value>> &rows) {
    std::vector<std::vector<Value>> colsv(names.size());
    for (const auto &row : rows)
        for (size_t c = 0; c < names.size(); c++) colsv[c].push_back(row[c]);
    return NewBowFromColBasedInterfaces(names, types, colsv);
}

// convenience literals for the table-driven tests: I(10), F(1.5), N
inline Value I(int64_t v) { return Scalar(v); }
inline Value F(double v) { return Scalar(v); }
static const Value N = std::nullopt;

namespace detail {
inline Error AbiError(int rc) { (void)rc; return Error(bowgpu_last_error()); }

// caller-owned output storage: what bow.NewBuffer(W, typ) allocates (bowbuffer.go:22-40)
struct OutStore {
    std::vector<uint64_t> data;
    std::vector<uint8_t> validity;
    bowgpu_out Make(int64_t slots) {
        data.assign((size_t)slots + 1, 0);
        validity.assign((size_t)((slots + 7) / 8) + 1, 0);
        bowgpu_out o;
        memset(&o, 0, sizeof o);
        o.values = data.data(); o.validity = validity.data(); o.length = slots; o.residency = BOWGPU_HOST;
        return o;
    }
    Series ToSeries(const std::string &name, const bowgpu_out &o) {
        if (o.type == BOWGPU_BOOLEAN) {   // a Boolean result arrives bit-packed (ceil(length / 8) bytes): back into 0 / 1 slots
            const uint8_t *bits = reinterpret_cast<const uint8_t *>(data.data());
            std::vector<uint64_t> slots((size_t)o.length);
            for (int64_t r = 0; r < o.length; r++) slots[(size_t)r] = (bits[r >> 3] >> (r & 7)) & 1u;
            data = std::move(slots);
        }
        data.resize((size_t)o.length);
        validity.resize((size_t)((o.length + 7) / 8));
        return NewSeriesRaw(name, (Type)o.type, data, validity);
    }
};
}  // namespace detail

inline std::pair<BowPtr, Error> Bow::FillLinear(int refColIndex, int toFillColIndex) const {
    if (refColIndex < 0 || refColIndex > NumCols() - 1) return {nullptr, Errorf("refColIndex is out of range")};
    if (toFillColIndex < 0 || toFillColIndex > NumCols() - 1) return {nullptr, Errorf("toFillColIndex is out of range")};
    std::vector<bowgpu_col> c;
    for (int i = 0; i < NumCols(); i++) c.push_back(ArrowCol(i));
    detail::OutStore st;
    bowgpu_out o = st.Make(NumRows());
    int32_t unchanged = 0;
    int rc = bowgpu_fill_linear(c.data(), NumCols(), refColIndex, toFillColIndex, &o, &unchanged);
    if (rc) return {nullptr, detail::AbiError(rc)};
    auto out = std::make_shared<Bow>(*this);
    if (!unchanged) out->cols[toFillColIndex] = st.ToSeries(cols[toFillColIndex].Name, o);
    return {out, Error()};
}

// NewBowFromParquet: bowparquet.go:44-153, with the columns decoded on the device (bowgpu_parquet_*): Int64 / Float64 columns
// through bowgpu_parquet_read_column.  ParquetBooleans::Read sends a column whose reported type is BOWGPU_BOOLEAN to
// bowgpu_parquet_read_bool_column, so a file with a flag column becomes a Bow with a Boolean series (bit-packed on arrival,
// unpacked by OutStore::ToSeries); the default, ParquetBooleans::Skip, is what this mirror always did with such a column, and what
// its callers that index the result's columns rely on.  The reference's String columns are outside the device path and are skipped.
enum class ParquetBooleans { Skip, Read };
inline std::pair<BowPtr, Error> NewBowFromParquet(const std::string &path, ParquetBooleans booleans = ParquetBooleans::Skip) {
    bowgpu_parquet *h = nullptr;
    int rc = bowgpu_parquet_open(path.c_str(), &h);
    if (rc) return {nullptr, Wrap("bow.NewBowFromParquet", detail::AbiError(rc))};
    int64_t rows = 0;
    int32_t ncols = 0;
    bowgpu_parquet_info(h, &rows, &ncols);
    std::vector<Series> series;
    for (int32_t i = 0; i < ncols && !rc; i++) {
        char name[256];
        int32_t type = -1, optional = 0;
        bowgpu_parquet_column(h, i, name, (int32_t)sizeof name, &type, &optional);
        const bool flag = type == BOWGPU_BOOLEAN && booleans == ParquetBooleans::Read;
        if (type != BOWGPU_INT64 && type != BOWGPU_FLOAT64 && !flag) continue;
        detail::OutStore st;
        bowgpu_out o = st.Make(rows);
        rc = flag ? bowgpu_parquet_read_bool_column(h, i, &o) : bowgpu_parquet_read_column(h, i, &o);
        if (!rc) series.push_back(st.ToSeries(name, o));
    }
    const Error err = rc ? Wrap("bow.NewBowFromParquet", detail::AbiError(rc)) : Error();
    bowgpu_parquet_close(h);
    if (rc) return {nullptr, err};
    return NewBow(std::move(series));
}

inline std::pair<BowPtr, Error> Bow::fill(int method, const std::vector<int> &colIndices) const {
    std::vector<bool> selected(NumCols(), colIndices.empty());  // selectCols: bowfill.go:268-288
    for (int ci : colIndices) {
        if (ci < 0 || ci > NumCols() - 1) return {nullptr, Errorf("selectCols: colIndex '" + std::to_string(ci) + "' out of range")};
        selected[ci] = true;
    }
    for (int ci = 0; ci < NumCols(); ci++)  // FillMean checks types first (bowfill.go:114-125); this mirror holds Int64 / Float64 only
        if (selected[ci] && cols[ci].typ != Type::Int64 && cols[ci].typ != Type::Float64)
            return {nullptr, Errorf("column '" + cols[ci].Name + "' is of unsupported type '" + TypeString(cols[ci].typ) + "'")};
    auto out = std::make_shared<Bow>(*this);
    for (int ci = 0; ci < NumCols(); ci++) {
        if (!selected[ci] || cols[ci].NullN() == 0) continue;  // passed through: bowfill.go:130-133, :186-189
        bowgpu_col c = ArrowCol(ci);
        detail::OutStore st;
        bowgpu_out o = st.Make(NumRows());
        int32_t unchanged = 0;
        int rc = bowgpu_fill(&c, method, &o, &unchanged);
        if (rc) return {nullptr, detail::AbiError(rc)};
        out->cols[ci] = st.ToSeries(cols[ci].Name, o);
    }
    return {out, Error()};
}

inline std::pair<BowPtr, Error> Bow::SortByCol(int colIndex) const {
    if (colIndex < 0 || colIndex > NumCols() - 1) return {nullptr, Errorf("no column '" + std::to_string(colIndex) + "'")};
    if (cols[colIndex].NullN() != 0)   // bowsort.go:11-15
        return {nullptr, Errorf("column to sort by has " + std::to_string(cols[colIndex].NullN()) + " nil values")};
    std::vector<bowgpu_col> c;
    for (int i = 0; i < NumCols(); i++) c.push_back(ArrowCol(i));
    std::vector<detail::OutStore> st((size_t)NumCols());
    std::vector<bowgpu_out> o;
    for (int i = 0; i < NumCols(); i++) o.push_back(st[(size_t)i].Make(NumRows()));
    int32_t unchanged = 0;
    int rc = bowgpu_sort_by_col(c.data(), NumCols(), colIndex, o.data(), &unchanged);
    if (rc) return {nullptr, detail::AbiError(rc)};
    if (unchanged) {   // bowsort.go:19-21 returns b itself (a copy where the receiver is not held by a shared_ptr)
        BowPtr self = weak_from_this().lock();
        return {self ? self : std::make_shared<Bow>(*this), Error()};
    }
    auto out = std::make_shared<Bow>();
    for (int i = 0; i < NumCols(); i++) out->cols.push_back(st[(size_t)i].ToSeries(cols[i].Name, o[(size_t)i]));
    return {out, Error()};
}

inline Value Convert(Type t, const FilterArg &a) {
    if (t != Type::Int64 && t != Type::Float64) return Nil();
    const bool to_int = t == Type::Int64;
    switch (a.kind) {
    case FilterArg::KInt: return to_int ? Scalar(a.i) : Scalar((double)a.i);
    case FilterArg::KFloat: return to_int ? Scalar(GoInt64(a.f)) : Scalar(a.f);
    case FilterArg::KBool: return to_int ? Scalar((int64_t)(a.b ? 1 : 0)) : Scalar(a.b ? 1. : 0.);
    case FilterArg::KStr: {   // strconv.ParseInt(s, 10, 64) / strconv.ParseFloat(s, 64): the whole string, no surrounding space
        if (a.s.empty() || isspace((unsigned char)a.s[0])) return Nil();
        char *end = nullptr;
        errno = 0;
        if (to_int) {
            const long long v = strtoll(a.s.c_str(), &end, 10);
            if (errno == ERANGE || *end != '\0') return Nil();
            return Scalar((int64_t)v);
        }
        const double v = strtod(a.s.c_str(), &end);
        if (*end != '\0' || (errno == ERANGE && std::isinf(v))) return Nil();
        return Scalar(v);
    }
    default: return Nil();
    }
}

inline RowCmp Bow::MakeFilterValuesV(int colIndex, const std::vector<FilterArg> &values) const {
    RowCmp r;
    r.col = colIndex;
    r.typ = ColumnType(colIndex);
    for (const FilterArg &a : values) {
        const Value v = bow::Convert(r.typ, a);   // (Type.Convert of one value: the member of the same name is the column's)
        if (!v) { r.match_null = true; continue; }
        uint64_t bits;
        if (r.typ == Type::Int64) { const int64_t x = std::get<int64_t>(*v); memcpy(&bits, &x, 8); }
        else { const double x = std::get<double>(*v); memcpy(&bits, &x, 8); }
        r.values.push_back(bits);
    }
    return r;
}
template <typename... V> inline RowCmp Bow::MakeFilterValues(int colIndex, V... values) const {
    return MakeFilterValuesV(colIndex, std::vector<FilterArg>{FilterArg(values)...});
}

inline std::pair<BowPtr, Error> Bow::FilterV(const std::vector<RowCmp> &cmps) const {
    const int n = NumRows();
    std::vector<bowgpu_filter_pred> preds;
    std::vector<uint8_t> closure_rows;   // the user closures, ANDed: bit i of byte i / 8
    for (const RowCmp &r : cmps) {
        if (r.fn) {
            if (closure_rows.empty() && n > 0) {
                closure_rows.assign((size_t)((n + 7) / 8), 0xFF);
                if (n & 7) closure_rows.back() = (uint8_t)((1u << (n & 7)) - 1u);
            }
            for (int i = 0; i < n; i++)
                if (((closure_rows[(size_t)i >> 3] >> (i & 7)) & 1) && !r.fn(*this, i)) closure_rows[(size_t)i >> 3] &= (uint8_t)~(1u << (i & 7));
            continue;
        }
        bowgpu_filter_pred p;
        memset(&p, 0, sizeof p);
        p.col = r.col;
        p.match_null = r.match_null;
        // (values boxed as another type than the column's never equal its values: only nil == nil is left of such a comparator)
        if (r.col >= 0 && r.col < NumCols() && r.typ == ColumnType(r.col)) {
            p.n_values = (int32_t)r.values.size();
            p.values = r.values.empty() ? nullptr : r.values.data();
        }
        preds.push_back(p);
    }
    std::vector<bowgpu_col> c;
    for (int i = 0; i < NumCols(); i++) c.push_back(ArrowCol(i));
    std::vector<detail::OutStore> st((size_t)NumCols());
    std::vector<bowgpu_out> o;
    for (int i = 0; i < NumCols(); i++) o.push_back(st[(size_t)i].Make(n));
    int64_t first = 0, count = 0;
    int32_t contiguous = 0;
    const int rc = bowgpu_filter(c.data(), NumCols(), preds.data(), (int32_t)preds.size(), closure_rows.empty() ? nullptr : closure_rows.data(),
                                 BOWGPU_HOST, o.data(), &first, &count, &contiguous);
    if (rc) return {nullptr, detail::AbiError(rc)};
    if (contiguous) return {count == 0 ? NewEmptySlice() : NewSlice((int)first, (int)(first + count)), Error()};   // bowsetters.go:74-82
    auto out = std::make_shared<Bow>();
    for (int i = 0; i < NumCols(); i++) out->cols.push_back(st[(size_t)i].ToSeries(cols[i].Name, o[(size_t)i]));
    return {out, Error()};
}
template <typename... C> inline std::pair<BowPtr, Error> Bow::Filter(const C &...cmps) const {
    return FilterV(std::vector<RowCmp>{RowCmp(cmps)...});
}

inline std::pair<BowPtr, Error> Bow::DropNils(std::vector<int> colIndices) const {
    const int n = NumRows();
    std::vector<int32_t> idx(colIndices.begin(), colIndices.end());
    std::vector<bowgpu_col> c;
    for (int i = 0; i < NumCols(); i++) c.push_back(ArrowCol(i));
    std::vector<detail::OutStore> st((size_t)NumCols());
    std::vector<bowgpu_out> o;
    for (int i = 0; i < NumCols(); i++) o.push_back(st[(size_t)i].Make(n));
    int64_t first = 0, count = 0;
    int32_t contiguous = 0;
    const int rc = bowgpu_drop_nils(c.data(), NumCols(), idx.data(), (int32_t)idx.size(), o.data(), &first, &count, &contiguous);
    if (rc) return {nullptr, detail::AbiError(rc)};
    if (contiguous) {
        if (count == n) {   // bow.go:210-212 returns b itself (a copy where the receiver is not held by a shared_ptr)
            BowPtr self = weak_from_this().lock();
            return {self ? self : std::make_shared<Bow>(*this), Error()};
        }
        return {NewSlice((int)first, (int)(first + count)), Error()};
    }
    auto out = std::make_shared<Bow>();
    for (int i = 0; i < NumCols(); i++) out->cols.push_back(st[(size_t)i].ToSeries(cols[i].Name, o[(size_t)i]));
    return {out, Error()};
}

inline std::pair<BowPtr, Error> Bow::Diff(std::vector<int> colIndices) const {
    std::vector<bool> selected(NumCols(), colIndices.empty());  // selectCols: bowfill.go:268-288
    for (int ci : colIndices) {
        if (ci < 0 || ci > NumCols() - 1) return {nullptr, Errorf("selectCols: colIndex '" + std::to_string(ci) + "' out of range")};
        selected[ci] = true;
    }
    std::vector<int32_t> idx(colIndices.begin(), colIndices.end());
    std::vector<bowgpu_col> c;
    for (int i = 0; i < NumCols(); i++) c.push_back(ArrowCol(i));
    int nsel = 0;
    for (int i = 0; i < NumCols(); i++) nsel += selected[i];
    std::vector<detail::OutStore> st((size_t)nsel);
    std::vector<bowgpu_out> o;
    for (int i = 0; i < nsel; i++) o.push_back(st[(size_t)i].Make(NumRows()));
    const int rc = bowgpu_diff(c.data(), NumCols(), idx.data(), (int32_t)idx.size(), o.data());
    if (rc) return {nullptr, detail::AbiError(rc)};
    auto out = std::make_shared<Bow>(*this);   // unselected columns pass through: bowdiff.go:33-36
    for (int ci = 0, k = 0; ci < NumCols(); ci++)
        if (selected[ci]) { out->cols[ci] = st[(size_t)k].ToSeries(cols[ci].Name, o[(size_t)k]); k++; }
    return {out, Error()};
}

inline std::pair<BowPtr, Error> Bow::Distinct(int colIndex) const {
    if (colIndex < 0 || colIndex > NumCols() - 1) return {nullptr, Errorf("no column '" + std::to_string(colIndex) + "'")};
    bowgpu_col c = ArrowCol(colIndex);
    detail::OutStore st;
    bowgpu_out o = st.Make(NumRows());
    int64_t nd = 0;
    const int rc = bowgpu_distinct(&c, &o, &nd);
    if (rc) return {nullptr, detail::AbiError(rc)};
    if (nd == 0) { o.length = 0; o.null_count = 0; o.type = c.type; }   // (nothing was written)
    auto out = std::make_shared<Bow>();
    out->cols.push_back(st.ToSeries(cols[colIndex].Name, o));
    return {out, Error()};
}

inline std::pair<BowPtr, Error> Bow::Convert(int colIndex, Type t) const {
    if (colIndex < 0 || colIndex > NumCols() - 1) return {nullptr, Errorf("no column '" + std::to_string(colIndex) + "'")};
    if (cols[colIndex].typ == Type::String || t == Type::String)
        return {nullptr, Errorf("Convert: a String source or target is not served by the device path (" + TypeString(cols[colIndex].typ) + " to " +
                                TypeString(t) + ")")};
    const bowgpu_col c = ArrowCol(colIndex);   // (a Boolean series goes in as Arrow bits)
    const int32_t to = (int32_t)t;
    detail::OutStore st;
    bowgpu_out o = st.Make(NumRows());
    const int rc = bowgpu_convert(&c, &to, 1, &o);
    if (rc) return {nullptr, detail::AbiError(rc)};
    auto out = std::make_shared<Bow>(*this);
    out->cols[colIndex] = st.ToSeries(cols[colIndex].Name, o);
    return {out, Error()};
}

inline int Bow::FindNext(int colIndex, int rowIndex, const Value &value) const {
    if (colIndex < 0 || colIndex > NumCols() - 1 || rowIndex < 0) return -1;
    const Type typ = ColumnType(colIndex);
    uint64_t bits = 0;
    if (value) {
        if (typ == Type::Int64 && std::holds_alternative<int64_t>(*value)) { const int64_t x = std::get<int64_t>(*value); memcpy(&bits, &x, 8); }
        else if (typ == Type::Float64 && std::holds_alternative<double>(*value)) { const double x = std::get<double>(*value); memcpy(&bits, &x, 8); }
        else return -1;   // another type than the column's: Go's == on the boxed values is false on every row
    }
    const bowgpu_col c = ArrowCol(colIndex);
    int64_t row = -1;
    if (bowgpu_find_next(&c, rowIndex, value ? &bits : nullptr, &row)) return -1;
    return (int)row;
}

inline std::pair<bool, Error> Bow::EqualOnDevice(const Bow &o, int mode) const {
    if (NumCols() != o.NumCols()) return {false, Error()};
    std::vector<bowgpu_col> l, r;
    for (int i = 0; i < NumCols(); i++) {
        if (cols[i].Name != o.cols[i].Name || cols[i].typ != o.cols[i].typ) return {false, Error()};
        l.push_back(ArrowCol(i));
        r.push_back(o.ArrowCol(i));
    }
    bowgpu_equal_info info;
    const int rc = bowgpu_equal(l.data(), r.data(), NumCols(), mode, &info);
    if (rc) return {false, detail::AbiError(rc)};
    return {info.equal != 0, Error()};
}

inline bool Bow::IsColEmpty(int colIndex) const {
    const bowgpu_col c = ArrowCol(colIndex);
    int32_t empty = 0;
    if (bowgpu_is_col_empty(&c, &empty)) return false;
    return empty != 0;
}

inline int Bow::validRow(const std::vector<int> &colIndices, int rowIndex, int direction) const {
    std::vector<bowgpu_col> c;
    for (int ci : colIndices) {
        if (ci < 0 || ci > NumCols() - 1) return -1;
        c.push_back(ArrowCol(ci));
    }
    int64_t row = -1;
    if (bowgpu_valid_row(c.data(), (int32_t)c.size(), rowIndex, direction, &row)) return -1;
    return (int)row;
}

// AppendBows: bowappend.go:11-103 (device).  No bows: a null pointer and no error; one bow: the bow itself.  Column names come from the
// first bow (this mirror models no Arrow metadata).  Where the reference panics on bows of different schemas - a missing bow, another
// number of columns - this returns an Error, as FilterV does.
inline std::pair<BowPtr, Error> AppendBows(const std::vector<BowPtr> &bows) {
    if (bows.empty()) return {nullptr, Error()};
    if (bows.size() == 1) return {bows[0], Error()};
    for (const BowPtr &b : bows)
        if (!b || b->NumCols() != bows[0]->NumCols()) return {nullptr, Errorf("bow.AppendBows: bows have different schemas")};
    const BowPtr &ref = bows[0];
    const int ncols = ref->NumCols();
    for (int ci = 0; ci < ncols; ci++)
        for (const BowPtr &b : bows)   // bowappend.go:40-42
            if (b->ColumnType(ci) != ref->ColumnType(ci))
                return {nullptr, Errorf("incompatible types '" + TypeString(ref->ColumnType(ci)) + "' and '" + TypeString(b->ColumnType(ci)) + "'")};
    std::vector<std::vector<bowgpu_col>> pieces;
    std::vector<const bowgpu_col *> frames;
    int64_t total = 0;
    for (const BowPtr &b : bows) {
        std::vector<bowgpu_col> c;
        for (int i = 0; i < ncols; i++) c.push_back(b->ArrowCol(i));
        pieces.push_back(std::move(c));
        total += b->NumRows();
    }
    for (const auto &p : pieces) frames.push_back(p.data());
    std::vector<detail::OutStore> st((size_t)ncols);
    std::vector<bowgpu_out> o;
    for (int i = 0; i < ncols; i++) o.push_back(st[(size_t)i].Make(total));
    int32_t unchanged = 0;
    const int rc = bowgpu_append(frames.data(), (int32_t)frames.size(), ncols, o.data(), &unchanged);
    if (rc) return {nullptr, detail::AbiError(rc)};
    auto out = std::make_shared<Bow>();
    for (int i = 0; i < ncols; i++) {
        if (total == 0) o[(size_t)i].type = (int32_t)ref->ColumnType(i);
        out->cols.push_back(st[(size_t)i].ToSeries(ref->ColumnName(i), o[(size_t)i]));
    }
    return {out, Error()};
}

inline std::pair<BowPtr, Error> Bow::join(const BowPtr &other, int32_t kind, bool all_common) const {
    if (!other) return {nullptr, Errorf("non bow object passed as argument")};
    const Bow &right = *other;
    if (kind == BOWGPU_JOIN_INNER && (NumCols() == 0 || right.NumCols() == 0))   // bowjoin.go:19-29
        return {NumCols() == 0 && right.NumCols() > 0 ? right.NewEmptySlice() : NewEmptySlice(), Error()};
    std::vector<int32_t> lks, rks;   // every common column, in the left bow's order
    for (int i = 0; i < NumCols(); i++) {   // getCommonCols: bowjoin.go:128-155
        int found = -1, n = 0;
        for (int j = 0; j < right.NumCols(); j++)
            if (right.cols[j].Name == cols[i].Name) { if (found < 0) found = j; n++; }
        if (n == 0) continue;
        if (n > 1) return {nullptr, Errorf("too many columns have the same name: right:" + right.String() + " left:" + String())};
        if (right.cols[found].typ != cols[i].typ)
            return {nullptr, Errorf("left and right bow on join columns are of incompatible types: " + cols[i].Name)};
        lks.push_back(i);
        rks.push_back(found);
    }
    const int32_t common = (int32_t)lks.size();
    if (common > 1 && !all_common)
        return {nullptr, Errorf("bow.Join: " + std::to_string(common) + " common columns, the device join takes one")};
    if (common > BOWGPU_JOIN_MAX_KEYS)
        return {nullptr, Errorf("bow.Join: " + std::to_string(common) + " common columns, the device join takes at most " +
                                std::to_string(BOWGPU_JOIN_MAX_KEYS))};
    // any number of common columns through the several-keys entry points: none and one are the one-key join there
    std::vector<bowgpu_col> lc, rc, lkc, rkc;
    for (int i = 0; i < NumCols(); i++) lc.push_back(ArrowCol(i));
    for (int i = 0; i < right.NumCols(); i++) rc.push_back(right.ArrowCol(i));
    for (int32_t k = 0; k < common; k++) {
        lkc.push_back(lc[(size_t)lks[(size_t)k]]);
        rkc.push_back(rc[(size_t)rks[(size_t)k]]);
    }
    // no input size bounds a join's rows: the count call sizes the outputs (without a common column it is not told the frames' lengths)
    int64_t rows = kind == BOWGPU_JOIN_OUTER ? (int64_t)NumRows() + right.NumRows() : 0, pairs = 0;
    if (common > 0)
        if (int rcode = bowgpu_join_keys_rows(lkc.data(), rkc.data(), common, kind, nullptr, nullptr, 0, BOWGPU_HOST, &rows, &pairs))
            return {nullptr, detail::AbiError(rcode)};
    std::vector<std::string> names;
    for (int i = 0; i < NumCols(); i++) names.push_back(cols[i].Name);
    for (int i = 0; i < right.NumCols(); i++)
        if (std::find(rks.begin(), rks.end(), i) == rks.end()) names.push_back(right.cols[i].Name);
    std::vector<detail::OutStore> st(names.size());
    std::vector<bowgpu_out> o(names.size() + 1);
    for (size_t i = 0; i < names.size(); i++) o[i] = st[i].Make(rows);
    int64_t got = 0;
    const int rcode = bowgpu_join_keys(lc.data(), NumCols(), lks.data(), rc.data(), right.NumCols(), rks.data(), common, kind, o.data(), &got);
    if (rcode) return {nullptr, detail::AbiError(rcode)};
    auto out = std::make_shared<Bow>();
    for (size_t i = 0; i < names.size(); i++) out->cols.push_back(st[i].ToSeries(names[i], o[i]));
    return {out, Error()};
}

inline bool Bow::IsColSorted(int colIndex) const {
    bowgpu_col c = ArrowCol(colIndex);
    int32_t s = 0;
    if (bowgpu_is_col_sorted(&c, &s)) return false;
    return s != 0;
}

// ============================================================================ rolling
namespace rolling {

namespace transformation {
// Func: rolling/transformation/factor.go:5 ; Factor: :7-20.  A Factor carries its multiplier so the device
// can fuse it; any other Func is applied to the reducer's results on the host afterwards.
struct Func {
    std::function<std::pair<Value, Error>(Value)> fn;
    bool is_factor = false;
    double factor = 1.0;
    std::pair<Value, Error> operator()(Value x) const { return fn(std::move(x)); }
};
inline Func Factor(double n) {
    Func f;
    f.is_factor = true;
    f.factor = n;
    f.fn = [n](Value x) -> std::pair<Value, Error> {
        if (!x) return {x, Error()};
        if (std::holds_alternative<double>(*x)) return {Scalar(std::get<double>(*x) * n), Error()};
        if (std::holds_alternative<int64_t>(*x)) return {Scalar(GoInt64((double)std::get<int64_t>(*x) * n)), Error()};
        return {Nil(), Errorf("factor: invalid type bool")};
    };
    return f;
}
}  // namespace transformation

// Options: rolling.go:49-53
struct Options {
    int64_t Offset = 0;
    bool Inclusive = false;
    BowPtr PrevRow;
};

// Window: window.go:12-19
struct Window {
    BowPtr Bow;
    int FirstIndex = 0;
    int IntervalColIndex = 0;
    int64_t FirstValue = 0;
    int64_t LastValue = 0;
    bool IsInclusive = false;
    // UnsetInclusive: window.go:23-31
    Window UnsetInclusive() const {
        if (!IsInclusive) return *this;
        Window w = *this;
        w.IsInclusive = false;
        w.Bow = w.Bow->NewSlice(0, w.Bow->NumRows() - 1);
        return w;
    }
};

using ColAggregationFunc = std::function<std::pair<Value, Error>(int colIndex, const Window &w)>;

// ColAggregation: aggregation.go:11-61 (value type with shared state, like the Go pointer receiver)
class ColAggregationImpl {
  public:
    std::string inputName;
    int inputIndex = -1;
    bool needInclusiveWindow = false;
    ColAggregationFunc aggregationFn;
    std::vector<transformation::Func> transformationFns;
    std::string outputName;
    Type typ = Type::Unknown;
    int32_t gpuKind = -1;  // BOWGPU_AGG_* for the built-in constructors, -1 for user closures
};

class ColAggregation {
  public:
    std::shared_ptr<ColAggregationImpl> p;
    ColAggregation() : p(std::make_shared<ColAggregationImpl>()) {}
    const std::string &InputName() const { return p->inputName; }
    int InputIndex() const { return p->inputIndex; }
    void SetInputIndex(int i) const { p->inputIndex = i; }  // mutates the caller's aggregator (aggregation.go:181)
    const std::string &OutputName() const { return p->outputName; }
    ColAggregation RenameOutput(const std::string &name) const {  // returns a copy: aggregation.go:82-86
        ColAggregation c;
        *c.p = *p;
        c.p->outputName = name;
        return c;
    }
    bool NeedInclusiveWindow() const { return p->needInclusiveWindow; }
    Type GetType() const { return p->typ; }
    Type GetReturnType(Type inputType, Type iteratorType) const {  // aggregation.go:110-121
        if (p->typ == Type::InputDependent) return inputType;
        if (p->typ == Type::IteratorDependent) return iteratorType;
        return p->typ;
    }
    const ColAggregationFunc &Func() const { return p->aggregationFn; }
    const std::vector<transformation::Func> &Transformations() const { return p->transformationFns; }
    ColAggregation SetTransformations(std::vector<transformation::Func> t) const {  // copy: aggregation.go:104-108
        ColAggregation c;
        *c.p = *p;
        c.p->transformationFns = std::move(t);
        return c;
    }
    int32_t GPUKind() const { return p->gpuKind; }
};

// NewColAggregation: aggregation.go:53-61
inline ColAggregation NewColAggregation(const std::string &inputName, bool needInclusiveWindow, Type typ, ColAggregationFunc fn) {
    ColAggregation a;
    a.p->inputName = inputName;
    a.p->needInclusiveWindow = needInclusiveWindow;
    a.p->typ = typ;
    a.p->aggregationFn = std::move(fn);
    return a;
}
using ColAggregationConstruct = std::function<ColAggregation(const std::string &)>;

// ColInterpolation: interpolation.go:10-28
using ColInterpolationFunc = std::function<std::pair<Value, Error>(int colIndex, const Window &w, const Bow &fullBow, BowPtr prevRow)>;
struct ColInterpolation {
    std::string colName;
    std::vector<Type> inputTypes;
    ColInterpolationFunc fn;
    int colIndex = -1;
    int32_t gpuKind = -1;
    double constValue = 0;
};
inline ColInterpolation NewColInterpolation(const std::string &colName, std::vector<Type> inputTypes, ColInterpolationFunc fn) {
    ColInterpolation c;
    c.colName = colName; c.inputTypes = std::move(inputTypes); c.fn = std::move(fn);
    return c;
}

class Rolling;
using RollingPtr = std::shared_ptr<Rolling>;

// Rolling: rolling.go:14-29 ; intervalRolling: rolling.go:31-43
class Rolling {
  public:
    BowPtr bow;
    int intervalColIndex = 0;
    int64_t interval = 0;
    Options options;
    int numWindows = 0;
    int64_t currWindowFirstValue = 0;
    int currWindowIndex = 0;
    Error err;
    // iterator state served from the device (all windows' bounds at once)
    bool boundsReady = false;
    std::vector<int64_t> firstIndex, sliceBegin, sliceEnd;
    std::vector<uint8_t> isIncl;
    int64_t s0 = 0;

    // A Rolling that Interpolate returned and whose interpolated Bow nobody has asked for yet (the Go shim: rolling/gpu_lazy.go,
    // patches/0006).  Aggregate on it is ONE call to the library (bowgpu_rolling_interpolate_aggregate); every other use first makes
    // the Rolling the reference's Interpolate returns (interpolation.go:57-68) and then IS that Rolling.
    struct Lazy {
        std::shared_ptr<const Rolling> base;   // the Rolling Interpolate was called on
        std::vector<ColInterpolation> interps; // validated: every colIndex is set
        int newIntervalCol = -1;
    };
    std::shared_ptr<Lazy> lazy;

    std::pair<int, Error> NumWindows() const { materialise(); return {numWindows, err}; }
    std::pair<BowPtr, Error> Bow() const { materialise(); return {bow, err}; }

    Error loadBounds() {
        materialise();
        if (boundsReady) return Error();
        firstIndex.assign((size_t)numWindows + 1, 0);
        sliceBegin = firstIndex; sliceEnd = firstIndex;
        isIncl.assign((size_t)numWindows + 1, 0);
        if (numWindows > 0) {
            bowgpu_col ts = bow->ArrowCol(intervalColIndex);
            bowgpu_options o = {options.Offset, options.Inclusive ? 1 : 0, 0};
            int rc = bowgpu_window_bounds(&ts, interval, &o, firstIndex.data(), sliceBegin.data(), sliceEnd.data(), isIncl.data(), BOWGPU_HOST);
            if (rc) return detail::AbiError(rc);
        }
        boundsReady = true;
        return Error();
    }

    // HasNext / Next: rolling.go:162-239, served from the device-computed bounds
    bool HasNext() {
        if (loadBounds()) return false;
        return currWindowIndex < numWindows;
    }
    struct NextResult { int windowIndex; std::optional<Window> window; Error err; };
    NextResult Next() {
        if (!HasNext()) return {currWindowIndex, std::nullopt, Error()};
        const int k = currWindowIndex++;
        Window w;
        w.FirstIndex = (int)firstIndex[k];
        w.IntervalColIndex = intervalColIndex;
        w.FirstValue = s0 + (int64_t)k * interval;
        w.LastValue = w.FirstValue + interval;
        w.IsInclusive = isIncl[k] != 0;
        w.Bow = sliceEnd[k] > sliceBegin[k] ? bow->NewSlice((int)sliceBegin[k], (int)sliceEnd[k]) : bow->NewEmptySlice();
        return {k, w, Error()};
    }

    RollingPtr Aggregate(const std::vector<ColAggregation> &aggrs) const;
    RollingPtr Interpolate(std::vector<ColInterpolation> interps) const;

  private:
    RollingPtr interpolated(const std::vector<ColInterpolation> &interps, int newIntervalCol) const;   // the tail of Interpolate (interpolation.go:57-68)
    RollingPtr interpolateAggregateGPU(const std::vector<ColAggregation> &aggrs) const;                // nullptr: make the two steps
    std::vector<bowgpu_interp> describeInterps(const std::vector<ColInterpolation> &interps, bool *all_builtin) const;
    void materialise() const {
        if (!lazy) return;
        Rolling *self = const_cast<Rolling *>(this);
        std::shared_ptr<Lazy> l = self->lazy;
        self->lazy = nullptr;
        RollingPtr real = l->base->interpolated(l->interps, l->newIntervalCol);
        *self = *real;
    }
    RollingPtr withError(const Error &e) const {
        auto r = std::make_shared<Rolling>(*this);
        r->err = e;
        return r;
    }
    friend std::pair<RollingPtr, Error> newIntervalRolling(BowPtr, int, int64_t, Options);
};

// newIntervalRolling: rolling.go:69-112
inline std::pair<RollingPtr, Error> newIntervalRolling(BowPtr b, int intervalColIndex, int64_t interval, Options options) {
    if (b->ColumnType(intervalColIndex) != Type::Int64)
        return {nullptr, Errorf("impossible to create a new intervalRolling on column of type " + TypeString(b->ColumnType(intervalColIndex)))};
    int64_t off = 0;
    if (bowgpu_enforce_interval_and_offset(interval, options.Offset, &off))
        return {nullptr, Wrap("enforceIntervalAndOffset", Error(bowgpu_last_error()))};
    options.Offset = off;
    if (options.PrevRow && options.PrevRow->NumRows() == 0) options.PrevRow = nullptr;  // enforcePrevRow: rolling.go:130-141
    if (options.PrevRow && options.PrevRow->NumRows() != 1)
        return {nullptr, Wrap("enforcePrevRow", Errorf("prevRow must have only one row, have " + std::to_string(options.PrevRow->NumRows())))};
    bowgpu_col ts = b->ArrowCol(intervalColIndex);
    int64_t s0 = 0, W = 0;
    if (bowgpu_plan_windows(&ts, interval, options.Offset, &s0, &W)) return {nullptr, Error(bowgpu_last_error())};
    auto r = std::make_shared<Rolling>();
    r->bow = b; r->intervalColIndex = intervalColIndex; r->interval = interval; r->options = options;
    r->numWindows = (int)W; r->currWindowFirstValue = s0; r->s0 = s0;
    return {r, Error()};
}

// IntervalRolling: rolling.go:60-67
inline std::pair<RollingPtr, Error> IntervalRolling(BowPtr b, const std::string &colName, int64_t interval, Options options) {
    auto [colIndex, err] = b->ColumnIndex(colName);
    if (err) return {nullptr, err};
    return newIntervalRolling(b, colIndex, interval, options);
}

// SetGPUDevices: the devices ONE Aggregate / Interpolate(...).Aggregate(...) call is spread over (process-wide; none or one id: one device) -
// the C++ twin of shim/go/rolling/gpu_cgo.go's SetGPUDevices (bowgpu_set_devices; a Go application gets the node's devices from the shim's
// init(), a C++ one calls this once).  Nothing else changes: r->Aggregate(...) is the same call with the same result.
inline Error SetGPUDevices(const std::vector<int> &ids) {
    if (bowgpu_set_devices(ids.empty() ? nullptr : ids.data(), (int)ids.size())) return Error(bowgpu_last_error());
    return Error();
}

// ----------------------------------------------------------------------------- Aggregate
inline RollingPtr Rolling::Aggregate(const std::vector<ColAggregation> &aggrs) const {
    if (lazy) {   // r.Interpolate(...).Aggregate(...): both steps in one call to the library when it takes them
        if (RollingPtr r = interpolateAggregateGPU(aggrs)) return r;
        materialise();
    }
    if (err) return std::make_shared<Rolling>(*this);  // aggregation.go:124-126
    // indexedAggregations + validateAggregation: aggregation.go:147-188
    auto fail = [&](const std::string &prefix, const Error &e) { return withError(Wrap(prefix, e)); };
    if (aggrs.empty()) return fail("intervalRolling.indexedAggregations", Errorf("at least one column aggregation is required"));
    Options opts = options;
    int newIntervalCol = -1;
    for (size_t i = 0; i < aggrs.size(); i++) {
        if (aggrs[i].InputName().empty())
            return fail("intervalRolling.indexedAggregations", Errorf("aggregation " + std::to_string(i) + " has no column name"));
        auto [readIndex, e] = bow->ColumnIndex(aggrs[i].InputName());
        if (e) return fail("intervalRolling.indexedAggregations", e);
        aggrs[i].SetInputIndex(readIndex);
        if (aggrs[i].NeedInclusiveWindow()) opts.Inclusive = true;
        if (readIndex == intervalColIndex) newIntervalCol = (int)i;
    }
    if (newIntervalCol == -1)
        return fail("intervalRolling.indexedAggregations", Errorf("must keep interval column '" + bow->ColumnName(intervalColIndex) + "'"));

    // aggregateWindows: aggregation.go:190-238.  Built-in reducers (with Factor chains) run fused on the device;
    // user closures are called per window with slices whose bounds come from the device.
    const size_t A = aggrs.size();
    std::vector<Series> series(A);
    std::vector<int> gpu_idx;
    for (size_t i = 0; i < A; i++) {
        bool fusable = aggrs[i].GPUKind() >= 0;
        for (const auto &t : aggrs[i].Transformations()) fusable = fusable && t.is_factor;
        fusable = fusable && aggrs[i].Transformations().size() <= BOWGPU_MAX_FACTORS;
        if (aggrs[i].GPUKind() >= 0) gpu_idx.push_back((int)i);
        (void)fusable;
    }
    auto outName = [&](size_t i) { return aggrs[i].OutputName().empty() ? bow->ColumnName(aggrs[i].InputIndex()) : aggrs[i].OutputName(); };

    if (!gpu_idx.empty()) {
        std::vector<bowgpu_col> cols;
        for (int i = 0; i < bow->NumCols(); i++) cols.push_back(bow->ArrowCol(i));
        std::vector<bowgpu_agg> ga;
        std::vector<bool> host_transform;
        for (int i : gpu_idx) {
            bowgpu_agg g;
            memset(&g, 0, sizeof g);
            g.kind = aggrs[i].GPUKind();
            g.col = aggrs[i].InputIndex();
            bool all_factor = aggrs[i].Transformations().size() <= BOWGPU_MAX_FACTORS;
            for (const auto &t : aggrs[i].Transformations()) all_factor = all_factor && t.is_factor;
            if (all_factor)
                for (const auto &t : aggrs[i].Transformations()) g.factors[g.n_factors++] = t.factor;
            host_transform.push_back(!all_factor);
            ga.push_back(g);
        }
        bool hidden_key = true;  // the ABI wants one aggregator on the interval column (aggregation.go:163-166)
        for (const auto &g : ga) hidden_key = hidden_key && g.col != intervalColIndex;
        if (hidden_key) {
            bowgpu_agg g;
            memset(&g, 0, sizeof g);
            g.kind = BOWGPU_AGG_WINDOW_START; g.col = intervalColIndex;
            ga.push_back(g);
        }
        std::vector<detail::OutStore> stores(ga.size());
        std::vector<bowgpu_out> outs;
        for (auto &s : stores) outs.push_back(s.Make(numWindows));
        bowgpu_options o = {opts.Offset, opts.Inclusive ? 1 : 0, 0};
        bowgpu_agg_info info;
        int rc = bowgpu_rolling_aggregate(cols.data(), bow->NumCols(), intervalColIndex, interval, &o, ga.data(), (int32_t)ga.size(), outs.data(), &info);
        if (rc) return fail("intervalRolling.aggregateWindows", detail::AbiError(rc));
        for (size_t k = 0; k < gpu_idx.size(); k++) {
            const int i = gpu_idx[k];
            Series s = stores[k].ToSeries(outName((size_t)i), outs[k]);
            if (host_transform[k]) {  // arbitrary transformation.Func: applied to each window's result (aggregation.go:216-227)
                const Type typ = s.typ;
                for (int64_t w = 0; w < s.length; w++) {
                    Value v;
                    if (s.IsValid(w)) {
                        if (typ == Type::Int64) { int64_t x; memcpy(&x, &s.data[w], 8); v = Scalar(x); }
                        else if (typ == Type::Boolean) v = Scalar(s.data[w] != 0);
                        else { double x; memcpy(&x, &s.data[w], 8); v = Scalar(x); }
                    }
                    for (const auto &t : aggrs[i].Transformations()) {
                        auto [nv, e] = t(v);
                        if (e) return fail("intervalRolling.aggregateWindows", e);
                        v = nv;
                    }
                    uint64_t bits = 0;
                    bool valid = v.has_value();
                    if (valid) {
                        if (typ == Type::Int64) { int64_t x = std::holds_alternative<int64_t>(*v) ? std::get<int64_t>(*v) : GoInt64(std::get<double>(*v)); memcpy(&bits, &x, 8); }
                        else if (typ == Type::Boolean && std::holds_alternative<bool>(*v)) bits = std::get<bool>(*v) ? 1 : 0;
                        else { double x = std::holds_alternative<double>(*v) ? std::get<double>(*v) : (double)std::get<int64_t>(*v); memcpy(&bits, &x, 8); }
                    }
                    s.data[w] = bits;
                    if (valid) s.validity[w >> 3] |= (uint8_t)(1u << (w & 7)); else s.validity[w >> 3] &= (uint8_t)~(1u << (w & 7));
                }
            }
            series[(size_t)i] = std::move(s);
        }
    }

    // user closures
    bool any_closure = false;
    for (size_t i = 0; i < A; i++) any_closure = any_closure || aggrs[i].GPUKind() < 0;
    if (any_closure) {
        Rolling it = *this;
        it.options = opts;
        it.currWindowIndex = 0;
        it.boundsReady = false;
        std::vector<std::vector<Value>> results(A, std::vector<Value>((size_t)numWindows));
        while (it.HasNext()) {
            auto nx = it.Next();
            if (nx.err) return fail("intervalRolling.aggregateWindows", nx.err);
            for (size_t i = 0; i < A; i++) {
                if (aggrs[i].GPUKind() >= 0) continue;
                const Window &w = *nx.window;
                auto [val, e] = (!aggrs[i].NeedInclusiveWindow() && w.IsInclusive) ? aggrs[i].Func()(aggrs[i].InputIndex(), w.UnsetInclusive())
                                                                                   : aggrs[i].Func()(aggrs[i].InputIndex(), w);
                if (e) return fail("intervalRolling.aggregateWindows", e);
                Value v = val;
                for (const auto &t : aggrs[i].Transformations()) {
                    auto [nv, e2] = t(v);
                    if (e2) return fail("intervalRolling.aggregateWindows", e2);
                    v = nv;
                }
                results[i][(size_t)nx.windowIndex] = v;
            }
        }
        if (it.err) return fail("intervalRolling.aggregateWindows", it.err);
        for (size_t i = 0; i < A; i++) {
            if (aggrs[i].GPUKind() >= 0) continue;
            const Type typ = aggrs[i].GetReturnType(bow->ColumnType(aggrs[i].InputIndex()), bow->ColumnType(intervalColIndex));
            auto [b1, e] = NewBowFromColBasedInterfaces({outName(i)}, {typ}, {results[i]});  // SetOrDrop conversions
            if (e) return fail("intervalRolling.aggregateWindows", e);
            series[i] = b1->cols[0];
        }
    }

    auto [b, e] = NewBow(std::move(series));
    if (e) return fail("intervalRolling.aggregateWindows", e);
    auto [newR, e2] = newIntervalRolling(b, newIntervalCol, interval, opts);  // aggregation.go:139
    if (e2) return fail("newIntervalRolling", e2);
    return newR;
}

// ----------------------------------------------------------------------------- Interpolate
inline RollingPtr Rolling::Interpolate(std::vector<ColInterpolation> interps) const {
    materialise();
    if (err) return std::make_shared<Rolling>(*this);  // interpolation.go:31-33
    if (interps.empty()) return withError(Errorf("at least one column interpolation is required"));
    int newIntervalCol = -1;
    for (size_t i = 0; i < interps.size(); i++) {  // validateInterpolation: interpolation.go:71-96
        if (interps[i].colName.empty())
            return withError(Wrap("intervalRolling.validateInterpolation", Errorf("interpolation " + std::to_string(i) + " has no column name")));
        auto [idx, e] = bow->ColumnIndex(interps[i].colName);
        if (e) return withError(Wrap("intervalRolling.validateInterpolation", e));
        interps[i].colIndex = idx;
        bool ok = false;
        for (Type t : interps[i].inputTypes) ok = ok || t == bow->ColumnType(idx);
        if (!ok) {
            std::string acc = "[";
            for (size_t k = 0; k < interps[i].inputTypes.size(); k++) acc += (k ? " " : "") + TypeString(interps[i].inputTypes[k]);
            acc += "]";
            return withError(Wrap("intervalRolling.validateInterpolation", Errorf("accepts types " + acc + ", got type " + TypeString(bow->ColumnType(idx)))));
        }
        if (idx == intervalColIndex) newIntervalCol = (int)i;
    }
    if (newIntervalCol == -1) return withError(Errorf("must keep interval column '" + bow->ColumnName(intervalColIndex) + "'"));

    // every interpolator a built-in, a Rolling nobody has stepped, a Bow with windows: the interpolated Bow is made when first asked for
    bool all_builtin = true;
    for (const auto &ip : interps) all_builtin = all_builtin && ip.gpuKind >= 0;
    if (all_builtin && currWindowIndex == 0 && numWindows > 0) {
        materialise();
        auto r = std::make_shared<Rolling>(*this);
        r->lazy = std::make_shared<Lazy>();
        r->lazy->base = std::make_shared<const Rolling>(*this);
        r->lazy->interps = interps;
        r->lazy->newIntervalCol = newIntervalCol;
        return r;
    }
    return interpolated(interps, newIntervalCol);
}

inline std::vector<bowgpu_interp> Rolling::describeInterps(const std::vector<ColInterpolation> &interps, bool *all_builtin) const {
    std::vector<bowgpu_interp> gi;
    *all_builtin = true;
    for (const auto &ip : interps) {
        if (ip.gpuKind < 0) { *all_builtin = false; return gi; }
        bowgpu_interp g;
        memset(&g, 0, sizeof g);
        g.kind = ip.gpuKind; g.col = ip.colIndex; g.const_value = ip.constValue;
        if (options.PrevRow) {  // linear.go:14-18, stepprevious.go:13-15
            const int last = options.PrevRow->NumRows() - 1;
            auto [pt, tv] = options.PrevRow->GetFloat64(intervalColIndex, last);
            auto [pv, vv] = options.PrevRow->GetFloat64(ip.colIndex, last);
            g.has_prev_row = 1; g.prev_t = pt; g.prev_t_valid = tv; g.prev_v = pv; g.prev_v_valid = vv;
            g.prev_v_i64 = options.PrevRow->GetInt64(ip.colIndex, last).first;
        }
        gi.push_back(g);
    }
    return gi;
}

// interpolateWindows + newIntervalRolling on the result: interpolation.go:57-68, :98-161
inline RollingPtr Rolling::interpolated(const std::vector<ColInterpolation> &interps, int newIntervalCol) const {
    bool all_builtin = true;
    std::vector<bowgpu_interp> gi = describeInterps(interps, &all_builtin);
    if (!all_builtin)
        return withError(Wrap("intervalRolling.interpolateWindows", Errorf("custom ColInterpolation closures are outside the device path")));
    std::vector<bowgpu_col> cols;
    for (int i = 0; i < bow->NumCols(); i++) cols.push_back(bow->ArrowCol(i));
    bowgpu_options o = {options.Offset, options.Inclusive ? 1 : 0, 0};
    int64_t n_out = 0;
    int rc = bowgpu_rolling_interpolate_count(cols.data(), bow->NumCols(), intervalColIndex, interval, &o, gi.data(), (int32_t)gi.size(), &n_out);
    if (rc) return withError(Wrap("intervalRolling.interpolateWindows", detail::AbiError(rc)));
    std::vector<detail::OutStore> stores(gi.size());
    std::vector<bowgpu_out> outs;
    for (auto &s : stores) outs.push_back(s.Make(n_out));
    rc = bowgpu_rolling_interpolate_fill(cols.data(), bow->NumCols(), intervalColIndex, interval, &o, gi.data(), (int32_t)gi.size(), outs.data());
    if (rc) return withError(Wrap("intervalRolling.interpolateWindows", detail::AbiError(rc)));
    std::vector<Series> series;
    for (size_t i = 0; i < gi.size(); i++) {
        if (outs[i].length == 0) outs[i].type = (int32_t)bow->ColumnType(interps[i].colIndex);
        series.push_back(stores[i].ToSeries(bow->ColumnName(interps[i].colIndex), outs[i]));
    }
    auto [b, e] = NewBow(std::move(series));
    if (e) return withError(Wrap("intervalRolling.interpolateWindows", e));
    auto [newR, e2] = newIntervalRolling(b, newIntervalCol, interval, options);  // interpolation.go:63
    if (e2) return withError(Wrap("newIntervalRolling", e2));
    return newR;
}

// Interpolate(...).Aggregate(...) as one call (Go shim: interpolateAggregateGPU in rolling/gpu_cgo.go).  Mirrors Aggregate
// (aggregation.go:123-145) on the interpolated Rolling, whose Bow has the input's columns and types: indexedAggregations, the call,
// newIntervalRolling on the result.  nullptr = anything that is not a plain success: the caller makes the reference's two steps, which
// word every error.
inline RollingPtr Rolling::interpolateAggregateGPU(const std::vector<ColAggregation> &aggrs) const {
    const Rolling &b0 = *lazy->base;
    const std::vector<ColInterpolation> &interps = lazy->interps;
    if ((int)interps.size() != b0.bow->NumCols() || aggrs.empty()) return nullptr;
    for (size_t i = 0; i < interps.size(); i++)
        if (interps[i].colIndex != (int)i) return nullptr;
    Options opts = b0.options;
    int newIntervalCol = -1;
    std::vector<bowgpu_agg> ga;
    for (size_t i = 0; i < aggrs.size(); i++) {
        if (aggrs[i].InputName().empty()) return nullptr;
        auto [readIndex, e] = b0.bow->ColumnIndex(aggrs[i].InputName());
        if (e) return nullptr;
        aggrs[i].SetInputIndex(readIndex);
        if (aggrs[i].NeedInclusiveWindow()) opts.Inclusive = true;
        if (readIndex == b0.intervalColIndex) newIntervalCol = (int)i;
        if (aggrs[i].GPUKind() < 0 || aggrs[i].Transformations().size() > BOWGPU_MAX_FACTORS) return nullptr;
        bowgpu_agg g;
        memset(&g, 0, sizeof g);
        g.kind = aggrs[i].GPUKind(); g.col = readIndex;
        for (const auto &t : aggrs[i].Transformations()) {
            if (!t.is_factor) return nullptr;
            g.factors[g.n_factors++] = t.factor;
        }
        ga.push_back(g);
    }
    if (newIntervalCol == -1) return nullptr;
    bool all_builtin = true;
    std::vector<bowgpu_interp> gi = b0.describeInterps(interps, &all_builtin);
    if (!all_builtin) return nullptr;
    std::vector<bowgpu_col> cols;
    for (int i = 0; i < b0.bow->NumCols(); i++) cols.push_back(b0.bow->ArrowCol(i));
    std::vector<detail::OutStore> stores(ga.size());
    std::vector<bowgpu_out> outs;
    for (auto &s : stores) outs.push_back(s.Make(b0.numWindows));   // the interpolated frame keeps the window grid; the library checks the capacity
    bowgpu_options o = {opts.Offset, opts.Inclusive ? 1 : 0, 0};
    bowgpu_agg_info info;
    if (bowgpu_rolling_interpolate_aggregate(cols.data(), b0.bow->NumCols(), b0.intervalColIndex, b0.interval, &o, gi.data(), (int32_t)gi.size(),
                                             ga.data(), (int32_t)ga.size(), outs.data(), &info) != 0)
        return nullptr;
    std::vector<Series> series;
    for (size_t i = 0; i < ga.size(); i++) {
        const std::string name = aggrs[i].OutputName().empty() ? b0.bow->ColumnName(aggrs[i].InputIndex()) : aggrs[i].OutputName();   // aggregation.go:230-234
        series.push_back(stores[i].ToSeries(name, outs[i]));
    }
    auto [b, e] = NewBow(std::move(series));
    if (e) return nullptr;
    auto [newR, e2] = newIntervalRolling(b, newIntervalCol, b0.interval, opts);  // aggregation.go:139
    if (e2) return b0.withError(Wrap("newIntervalRolling", e2));
    return newR;
}

// ----------------------------------------------------------------------------- rolling/aggregation
namespace aggregation {
namespace detail2 {
inline ColAggregation builtin(const std::string &col, bool incl, Type typ, int32_t kind) {
    // the closure is never called for built-ins (the device computes them); it reports misuse loudly
    ColAggregation a = NewColAggregation(col, incl, typ, [](int, const Window &) -> std::pair<Value, Error> {
        return {Nil(), Errorf("built-in aggregation closures run on the device")};
    });
    a.p->gpuKind = kind;
    return a;
}
}  // namespace detail2
inline ColAggregation WindowStart(const std::string &col) { return detail2::builtin(col, false, IteratorDependent, BOWGPU_AGG_WINDOW_START); }
inline ColAggregation Sum(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_SUM); }
inline ColAggregation ArithmeticMean(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_MEAN); }
inline ColAggregation Min(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_MIN); }
inline ColAggregation Max(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_MAX); }
inline ColAggregation Count(const std::string &col) { return detail2::builtin(col, false, Int64, BOWGPU_AGG_COUNT); }
inline ColAggregation First(const std::string &col) { return detail2::builtin(col, false, InputDependent, BOWGPU_AGG_FIRST); }
inline ColAggregation Last(const std::string &col) { return detail2::builtin(col, false, InputDependent, BOWGPU_AGG_LAST); }
inline ColAggregation Mode(const std::string &col) { return detail2::builtin(col, false, InputDependent, BOWGPU_AGG_MODE); }  // mode.go:8-32
inline ColAggregation IntegralStep(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_INTEGRAL_STEP); }
inline ColAggregation IntegralTrapezoid(const std::string &col) { return detail2::builtin(col, true, Float64, BOWGPU_AGG_INTEGRAL_TRAPEZOID); }
inline ColAggregation WeightedAverageStep(const std::string &col) { return detail2::builtin(col, false, Float64, BOWGPU_AGG_WAVG_STEP); }
inline ColAggregation WeightedAverageLinear(const std::string &col) { return detail2::builtin(col, true, Float64, BOWGPU_AGG_WAVG_LINEAR); }

// Aggregate (whole frame): rolling/aggregation/whole.go:12-93
inline std::pair<BowPtr, Error> Aggregate(BowPtr b, const std::string &intervalColName, const std::vector<ColAggregation> &aggrs) {
    if (!b) return {nullptr, Errorf("nil bow")};
    if (aggrs.empty()) return {nullptr, Errorf("at least one column aggregation is required")};
    auto [intervalColIndex, err] = b->ColumnIndex(intervalColName);
    if (err) return {nullptr, err};
    std::vector<bowgpu_agg> ga;
    std::vector<std::string> names;
    for (size_t i = 0; i < aggrs.size(); i++) {
        if (aggrs[i].InputName().empty()) return {nullptr, Errorf("column aggregation " + std::to_string(i) + ": no input name")};
        auto [idx, e] = b->ColumnIndex(aggrs[i].InputName());
        if (e) return {nullptr, Wrap("column aggregation " + std::to_string(i), e)};
        aggrs[i].SetInputIndex(idx);
        if (aggrs[i].GPUKind() < 0) return {nullptr, Errorf("column aggregation " + std::to_string(i) + ": custom closures are outside the device path")};
        bowgpu_agg g;
        memset(&g, 0, sizeof g);
        g.kind = aggrs[i].GPUKind(); g.col = idx;
        for (const auto &t : aggrs[i].Transformations())
            if (t.is_factor && g.n_factors < BOWGPU_MAX_FACTORS) g.factors[g.n_factors++] = t.factor;
        ga.push_back(g);
        names.push_back(aggrs[i].OutputName().empty() ? b->ColumnName(idx) : aggrs[i].OutputName());
    }
    std::vector<bowgpu_col> cols;
    for (int i = 0; i < b->NumCols(); i++) cols.push_back(b->ArrowCol(i));
    std::vector<bow::detail::OutStore> stores(ga.size());
    std::vector<bowgpu_out> outs;
    for (auto &s : stores) outs.push_back(s.Make(1));
    int rc = bowgpu_aggregate_whole(cols.data(), b->NumCols(), intervalColIndex, ga.data(), (int32_t)ga.size(), outs.data());
    if (rc) return {nullptr, bow::detail::AbiError(rc)};
    std::vector<Series> series;
    for (size_t i = 0; i < ga.size(); i++) series.push_back(stores[i].ToSeries(names[i], outs[i]));
    return NewBow(std::move(series));
}
}  // namespace aggregation

// ----------------------------------------------------------------------------- rolling/interpolation
namespace interpolation {
namespace detail3 {
inline ColInterpolation builtin(const std::string &col, std::vector<Type> types, int32_t kind) {
    ColInterpolation c = NewColInterpolation(col, std::move(types), nullptr);
    c.gpuKind = kind;
    return c;
}
}  // namespace detail3
inline ColInterpolation WindowStart(const std::string &col) { return detail3::builtin(col, {Int64}, BOWGPU_INTERP_WINDOW_START); }               // windowstart.go:8-14
inline ColInterpolation Linear(const std::string &col) { return detail3::builtin(col, {Int64, Float64}, BOWGPU_INTERP_LINEAR); }                  // linear.go:8-38
inline ColInterpolation StepPrevious(const std::string &col) { return detail3::builtin(col, {Int64, Float64, Boolean, String}, BOWGPU_INTERP_STEP_PREVIOUS); }
inline ColInterpolation None(const std::string &col) { return detail3::builtin(col, {Int64, Float64, Boolean}, BOWGPU_INTERP_NONE); }
// the constant-valued closure of rolling/interpolation_test.go:16-19, as a tagged interpolator
inline ColInterpolation Const(const std::string &col, std::vector<Type> types, double value) {
    ColInterpolation c = detail3::builtin(col, std::move(types), BOWGPU_INTERP_CONST);
    c.constValue = value;
    return c;
}
}  // namespace interpolation

}  // namespace rolling
}  // namespace bow
