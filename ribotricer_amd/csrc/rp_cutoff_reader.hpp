// learn-cutoff's column reader: ORF_type, transcript_type and phase_score of a ribotricer
// `*_translating_ORFs.tsv`, the way `pandas.read_csv(path, sep="\t", usecols=[...])` reads them
// (learn_cutoff.py:60-76 of the reference).
//
// Per row: a category code for each of the two text columns (first-seen order within the file)
// and the phase as float64 with pandas' DEFAULT float converter (precise_xstrtod: at most 17
// significant digits, leading zeros included, scaled by one correctly rounded power of ten --
// not a correctly rounded conversion).  The distinct raw category strings go back to Python,
// which applies str.lower(), the NA tokens and isin to them.
//
// Anything the reader does not model is reported (kFallback*) and the caller hands that file to
// pandas itself: a '"' byte, a lone '\r', a UTF-8 BOM, a row whose field count differs from the
// header's, a duplicated wanted column, or a phase text outside
// [+-]digits[.digits][(e|E)[+-]digits] and the NA tokens (plus integer-only texts past 15 digits
// and exponents that leave the finite range, where pandas' int path or ERANGE would apply).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

namespace rpcut {

enum { kOk = 0, kMissingColumns = 1, kFallbackQuote = 2, kFallbackCR = 3, kFallbackFields = 4,
       kFallbackPhase = 5, kFallbackHeader = 6 };

// pandas' default NA tokens (pandas._libs.parsers.STR_NA_VALUES)
inline bool is_na_token(const char *s, size_t n)
{
    static const char *const kNa[] = {"", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND",
                                      "1.#QNAN", "<NA>", "N/A", "NA", "NULL", "NaN", "None", "n/a", "nan", "null"};
    for (const char *t : kNa)
        if (std::strlen(t) == n && std::memcmp(t, s, n) == 0) return true;
    return false;
}

// pandas' default converter on a text already known to match the grammar.  Returns false where
// pandas would not produce this double (ERANGE, or an integer column past 15 digits).
inline bool precise_xstrtod(const char *p, const char *end, double *out)
{
    static double e10[309];
    static const bool init = [] {  // correctly rounded powers of ten, as pandas' table of literals
        char text[8];
        for (int i = 0; i < 309; ++i) std::snprintf(text, sizeof(text), "1e%d", i), e10[i] = std::strtod(text, nullptr);
        return true;
    }();
    (void)init;
    constexpr int kMaxDigits = 17;
    bool negative = false;
    if (*p == '-' || *p == '+') negative = *p++ == '-';
    double number = 0.;
    int exponent = 0, num_digits = 0, num_decimals = 0, int_digits = 0;
    while (p < end && *p >= '0' && *p <= '9') {
        if (num_digits < kMaxDigits) {
            number = number * 10. + (*p - '0');
            ++num_digits;
        } else {
            ++exponent;
        }
        ++int_digits;
        ++p;
    }
    bool is_int = true;
    if (p < end && *p == '.') {
        is_int = false;
        ++p;
        while (num_digits < kMaxDigits && p < end && *p >= '0' && *p <= '9') {
            number = number * 10. + (*p - '0');
            ++p;
            ++num_digits;
            ++num_decimals;
        }
        while (p < end && *p >= '0' && *p <= '9') ++p;
        exponent -= num_decimals;
    }
    if (negative) number = -number;
    if (p < end && (*p == 'e' || *p == 'E')) {
        is_int = false;
        ++p;
        bool eneg = false;
        if (*p == '-' || *p == '+') eneg = *p++ == '-';
        int n = 0, nd = 0;
        while (p < end && *p >= '0' && *p <= '9') {
            n = n * 10 + (*p - '0');
            ++p;
            if (++nd > 9) return false;
        }
        exponent += eneg ? -n : n;
    }
    // pandas reads an all-integer column as int64: exact up to 15 digits, but "-0" becomes +0.0
    if (is_int && (int_digits > 15 || (negative && number == 0.))) return false;
    if (exponent > 308) return false;
    if (exponent > 0) {
        number *= e10[exponent];
    } else if (exponent < -308) {
        if (exponent < -616) {
            number = 0.;  // (+0.0 whatever the sign, as pandas)
        } else {
            number /= e10[-308 - exponent];
            number /= e10[308];
        }
    } else {
        number /= e10[-exponent];
    }
    if (number == __builtin_huge_val() || number == -__builtin_huge_val()) return false;
    *out = number;
    return true;
}

// [+-]digits[.digits][(e|E)[+-]digits]
inline bool phase_grammar(const char *s, const char *end)
{
    const char *p = s;
    if (p < end && (*p == '+' || *p == '-')) ++p;
    const char *d = p;
    while (p < end && *p >= '0' && *p <= '9') ++p;
    if (p == d) return false;
    if (p < end && *p == '.') {
        ++p;
        d = p;
        while (p < end && *p >= '0' && *p <= '9') ++p;
        if (p == d) return false;
    }
    if (p < end && (*p == 'e' || *p == 'E')) {
        ++p;
        if (p < end && (*p == '+' || *p == '-')) ++p;
        d = p;
        while (p < end && *p >= '0' && *p <= '9') ++p;
        if (p == d) return false;
    }
    return p == end;
}

struct Columns {
    std::vector<int32_t> orf_type, tx_type;
    std::vector<double> phase;
    std::vector<std::string> orf_cats, tx_cats;
    int status = kOk;
    int64_t bad_line = 0;  // 1-based line of the first construct not modelled
    int missing = 0;       // bit i: wanted column i absent (ORF_ID, ORF_type, phase_score, transcript_type)
};

struct Dict {
    std::unordered_map<std::string_view, int32_t> map;
    std::vector<std::string_view> keys;
    int32_t code(std::string_view s)
    {
        auto it = map.find(s);
        if (it != map.end()) return it->second;
        const int32_t c = (int32_t)keys.size();
        map.emplace(s, c);
        keys.push_back(s);
        return c;
    }
};

struct Part {
    std::vector<int32_t> o, t;
    std::vector<double> ph;
    Dict od, td;
    int status = kOk;
    int64_t bad_row = -1;  // row (0-based within the part) of the first failure
};

inline void parse_rows(const char *b, const char *e, int nfields, int io, int it, int ip, Part &out)
{
    const int want = std::max(io, std::max(it, ip));
    int64_t row = 0;
    while (b < e) {
        const char *nl = (const char *)std::memchr(b, '\n', (size_t)(e - b));
        const char *le = nl ? nl : e;
        const char *next = nl ? nl + 1 : e;
        if (le > b && le[-1] == '\r') --le;
        if (le == b) {  // blank line: pandas skips it
            b = next;
            continue;
        }
        const char *fs[3] = {nullptr, nullptr, nullptr}, *fe[3] = {nullptr, nullptr, nullptr};
        int f = 0;
        const char *p = b;
        for (;;) {
            const char *tab = (const char *)std::memchr(p, '\t', (size_t)(le - p));
            const char *end = tab ? tab : le;
            if (f == io) fs[0] = p, fe[0] = end;
            else if (f == it) fs[1] = p, fe[1] = end;
            else if (f == ip) fs[2] = p, fe[2] = end;
            ++f;
            if (!tab) break;
            p = tab + 1;
            if (f > want) {  // the rest (the profile, >95 % of the bytes): count its fields only
                ++f;
                for (const char *q = p; (q = (const char *)std::memchr(q, '\t', (size_t)(le - q))); ++q) ++f;
                break;
            }
        }
        if (f != nfields) {
            out.status = kFallbackFields;
            out.bad_row = row;
            return;
        }
        double v;
        const size_t plen = (size_t)(fe[2] - fs[2]);
        if (is_na_token(fs[2], plen)) {
            v = __builtin_nan("");
        } else if (!phase_grammar(fs[2], fe[2]) || !precise_xstrtod(fs[2], fe[2], &v)) {
            out.status = kFallbackPhase;
            out.bad_row = row;
            return;
        }
        out.o.push_back(out.od.code(std::string_view(fs[0], (size_t)(fe[0] - fs[0]))));
        out.t.push_back(out.td.code(std::string_view(fs[1], (size_t)(fe[1] - fs[1]))));
        out.ph.push_back(v);
        ++row;
        b = next;
    }
}

inline int read(const char *text, size_t len, int n_threads, Columns &out)
{
    const char *end = text + len;
    if (len >= 3 && (unsigned char)text[0] == 0xEF && (unsigned char)text[1] == 0xBB && (unsigned char)text[2] == 0xBF)
        return out.status = kFallbackHeader;
    if (std::memchr(text, '"', len)) return out.status = kFallbackQuote;
    for (const char *q = text; (q = (const char *)std::memchr(q, '\r', (size_t)(end - q))); ++q)
        if (q + 1 >= end || q[1] != '\n') return out.status = kFallbackCR;
    // header
    const char *nl = (const char *)std::memchr(text, '\n', len);
    const char *he = nl ? nl : end;
    if (he > text && he[-1] == '\r') --he;
    static const char *const kWant[4] = {"ORF_ID", "ORF_type", "phase_score", "transcript_type"};
    int idx[4] = {-1, -1, -1, -1}, nfields = 0;
    for (const char *p = text;;) {
        const char *tab = (const char *)std::memchr(p, '\t', (size_t)(he - p));
        const char *fe = tab ? tab : he;
        for (int w = 0; w < 4; ++w)
            if ((size_t)(fe - p) == std::strlen(kWant[w]) && std::memcmp(p, kWant[w], (size_t)(fe - p)) == 0) {
                if (idx[w] >= 0) return out.status = kFallbackHeader;  // pandas would mangle the duplicate
                idx[w] = nfields;
            }
        ++nfields;
        if (!tab) break;
        p = tab + 1;
    }
    for (int w = 0; w < 4; ++w)
        if (idx[w] < 0) out.missing |= 1 << w;
    if (out.missing) return out.status = kMissingColumns;
    const char *body = nl ? nl + 1 : end;
    // parts cut at line starts
    const size_t blen = (size_t)(end - body);
    int T = n_threads > 0 ? n_threads : 1;
    if (blen < ((size_t)1 << 20)) T = 1;
    std::vector<const char *> cut(T + 1, end);
    cut[0] = body;
    for (int i = 1; i < T; ++i) {
        const char *c = body + blen * i / T;
        if (c < cut[i - 1]) c = cut[i - 1];
        const char *n2 = c > body ? (const char *)std::memchr(c - 1, '\n', (size_t)(end - (c - 1))) : c;
        cut[i] = n2 ? n2 + 1 : end;
    }
    std::vector<Part> parts(T);
    {
        std::vector<std::thread> th;
        for (int i = 1; i < T; ++i)
            th.emplace_back(parse_rows, cut[i], cut[i + 1], nfields, idx[1], idx[3], idx[2], std::ref(parts[i]));
        parse_rows(cut[0], cut[1], nfields, idx[1], idx[3], idx[2], parts[0]);
        for (auto &t : th) t.join();
    }
    for (int i = 0; i < T; ++i)
        if (parts[i].status != kOk) {
            // line number: header + rows of the parts before (blank lines are not counted: approximate)
            int64_t line = 2;
            for (int j = 0; j < i; ++j) line += (int64_t)parts[j].o.size();
            out.bad_line = line + parts[i].bad_row;
            return out.status = parts[i].status;
        }
    size_t n = 0;
    for (auto &p : parts) n += p.o.size();
    out.orf_type.resize(n);
    out.tx_type.resize(n);
    out.phase.resize(n);
    Dict od, td;
    size_t at = 0;
    for (auto &p : parts) {
        std::vector<int32_t> om(p.od.keys.size()), tm(p.td.keys.size());
        for (size_t c = 0; c < om.size(); ++c) om[c] = od.code(p.od.keys[c]);
        for (size_t c = 0; c < tm.size(); ++c) tm[c] = td.code(p.td.keys[c]);
        for (size_t r = 0; r < p.o.size(); ++r) {
            out.orf_type[at + r] = om[p.o[r]];
            out.tx_type[at + r] = tm[p.t[r]];
        }
        std::memcpy(out.phase.data() + at, p.ph.data(), p.ph.size() * sizeof(double));
        at += p.o.size();
    }
    for (auto s : od.keys) out.orf_cats.emplace_back(s);
    for (auto s : td.keys) out.tx_cats.emplace_back(s);
    return out.status = kOk;
}

}  // namespace rpcut
