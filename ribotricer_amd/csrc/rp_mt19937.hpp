// Host side of the MT19937 stream behind learn-cutoff's bootstrap (numpy's legacy RandomState:
// init_genrand(seed), 32-bit words, masked rejection in choice/randint).
//
// Notation.  x[t] is the UNTEMPERED sequence: x[0..623] is the seeded array, x[t + 624] =
// x[t + 397] ^ twist(x[t], x[t + 1]), and raw output word j is temper(x[624 + j]).  The "window"
// at offset o is x[o .. o + 623]: from it every raw word from j = o on can be generated.
//
// Jump-ahead.  Every bit position of x[t] (t >= 1) is a linear recurring sequence over GF(2)
// whose minimal polynomial p is the generator's characteristic polynomial (degree 19 937).  p is
// derived once per process with Berlekamp-Massey from the generator's own output bits.  With
// q(x) = x^J mod p = sum_m q_m x^m, x[t + J] = XOR_{q_m = 1} x[t + m] for t >= 1, so the window at
// o + J is a correlation of the 19 937 + 624 words after o with q (rp_bootstrap.hpp k_mt_jump
// does the same on the device).  At o = 0 only the low 31 bits of window word 0 come out wrong
// (x[0]'s low bits are not part of the state), and those bits never reach an output.
#pragma once

#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

namespace rpmt {

constexpr int kN = 624, kM = 397, kDeg = 19937;
constexpr uint32_t kUpper = 0x80000000u, kLower = 0x7fffffffu, kMatrixA = 0x9908b0dfu;
constexpr int kPolyWords = (kDeg + 63) / 64 + 1;  // 313 uint64: room for degree <= 20 031

inline void init_genrand(uint32_t seed, uint32_t *mt)
{
    mt[0] = seed;
    for (int i = 1; i < kN; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

inline uint32_t twist(uint32_t a, uint32_t b, uint32_t m)
{
    const uint32_t y = (a & kUpper) | (b & kLower);
    return m ^ (y >> 1) ^ ((y & 1u) ? kMatrixA : 0u);
}

inline uint32_t temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// x[base .. base + count) extended in place: buf holds x[base .. base + 624) on entry and
// x[base .. base + count) on return (count >= 624).
inline void extend(std::vector<uint32_t> &buf, size_t count)
{
    const size_t have = buf.size();
    buf.resize(count);
    for (size_t t = have; t < count; ++t) buf[t] = twist(buf[t - kN], buf[t - kN + 1], buf[t - kN + kM]);
}

// ---- GF(2) polynomials, bit i = coefficient of x^i ------------------------------------------
using Poly = std::vector<uint64_t>;

inline int degree(const Poly &a)
{
    for (int w = (int)a.size() - 1; w >= 0; --w)
        if (a[w]) return w * 64 + 63 - __builtin_clzll(a[w]);
    return -1;
}

inline bool bit(const Poly &a, int i) { return (a[i >> 6] >> (i & 63)) & 1u; }

inline void xor_shifted(Poly &dst, const Poly &src, int shift, int src_bits)
{
    const int ws = shift >> 6, bs = shift & 63, nw = (src_bits + 63) / 64;
    for (int w = 0; w < nw; ++w) {
        const uint64_t v = src[w];
        if (!v) continue;
        dst[w + ws] ^= v << bs;
        if (bs && (size_t)(w + ws + 1) < dst.size()) dst[w + ws + 1] ^= v >> (64 - bs);
    }
}

struct Field {
    Poly p;  // characteristic polynomial, degree kDeg
    std::vector<Poly> pow2;  // x^(2^j) mod p, j = 0..63
    std::vector<Poly> chunk;  // x^(624 * 2^e) mod p, e = 0..kMaxChunkExp
    static constexpr int kMaxChunkExp = 40;

    Poly reduce(Poly a) const  // a mod p
    {
        for (int d = degree(a); d >= kDeg; --d)
            if (bit(a, d)) xor_shifted(a, p, d - kDeg, kDeg + 1);
        a.resize(kPolyWords);
        return a;
    }
    Poly mul(const Poly &a, const Poly &b) const
    {
        Poly r(2 * kPolyWords + 2, 0);
        const int da = degree(a);
        for (int i = 0; i <= da; ++i)
            if (bit(a, i)) xor_shifted(r, b, i, kDeg);
        return reduce(r);
    }
    Poly square(const Poly &a) const
    {
        Poly r(2 * kPolyWords + 2, 0);
        for (int i = 0; i < kDeg; ++i)
            if (bit(a, i)) r[(2 * i) >> 6] |= 1ull << ((2 * i) & 63);
        return reduce(r);
    }
    // x^J mod p
    Poly power(uint64_t J) const
    {
        Poly r(kPolyWords, 0);
        r[0] = 1;
        for (int j = 0; J; ++j, J >>= 1)
            if (J & 1) r = mul(r, pow2[j]);
        return r;
    }
};

// Berlekamp-Massey over GF(2) on 2 * kDeg + 64 output bits (bit 31 of x[t], t >= 624): the
// connection polynomial C has length kDeg; p(x) = x^kDeg C(1/x).
inline Poly characteristic_polynomial()
{
    const int n = 2 * kDeg + 64;
    std::vector<uint32_t> x(kN);
    init_genrand(5489u, x.data());
    extend(x, (size_t)kN + n);
    // s reversed into bits so that s[k - i], i = 0..L, is contiguous at offset n - 1 - k
    const int nw = (n + 63) / 64 + 2;
    std::vector<uint64_t> rs(nw, 0);
    for (int k = 0; k < n; ++k)
        if (x[kN + k] >> 31) {
            const int r = n - 1 - k;
            rs[r >> 6] |= 1ull << (r & 63);
        }
    auto window = [&](int off, int w) -> uint64_t {  // bits off + 64w .. off + 64w + 63 of rs
        const int b = off + 64 * w, wi = b >> 6, sh = b & 63;
        uint64_t v = rs[wi] >> sh;
        if (sh && wi + 1 < nw) v |= rs[wi + 1] << (64 - sh);
        return v;
    };
    const int cw = kPolyWords + 2;
    Poly C(cw, 0), B(cw, 0), T;
    C[0] = B[0] = 1;
    int L = 0, m = 1;
    for (int k = 0; k < n; ++k) {
        const int off = n - 1 - k;  // rs bit off + i = s[k - i]
        uint64_t acc = 0;
        const int words = L / 64 + 1;
        for (int w = 0; w < words; ++w) {
            uint64_t c = C[w];
            if (w == words - 1) {
                const int top = L - 64 * w;  // keep bits 0..top
                if (top < 63) c &= (2ull << top) - 1;
            }
            acc ^= c & window(off, w);
        }
        if (!(__builtin_popcountll(acc) & 1)) {
            ++m;
            continue;
        }
        if (2 * L <= k) {
            T = C;
            xor_shifted(C, B, m, (cw - 1) * 64);
            L = k + 1 - L;
            B = T;
            m = 1;
        } else {
            xor_shifted(C, B, m, (cw - 1) * 64);
            ++m;
        }
    }
    Poly p(kPolyWords + 1, 0);
    for (int i = 0; i <= kDeg; ++i)
        if (bit(C, i)) {
            const int j = kDeg - i;
            p[j >> 6] |= 1ull << (j & 63);
        }
    return p;
}

// Per-process cache: p, x^(2^j) and x^(624 * 2^e).  The first caller pays for it (about a
// tenth of a second of host work); nothing in it depends on the seed or the data.
inline const Field &field(bool *built_now = nullptr)
{
    static std::once_flag once;
    static Field f;
    bool built = false;
    std::call_once(once, [&] {
        f.p = characteristic_polynomial();
        Poly x(kPolyWords, 0);
        x[0] = 2;
        f.pow2.push_back(x);
        for (int j = 1; j < 64; ++j) f.pow2.push_back(f.square(f.pow2.back()));
        f.chunk.push_back(f.power(kN));
        for (int e = 1; e <= Field::kMaxChunkExp; ++e) f.chunk.push_back(f.square(f.chunk.back()));
        built = true;
    });
    if (built_now) *built_now = built;
    return f;
}

// Window at o + J from the window at o (o >= 1 for an exact word 0; see the header comment).
inline void jump_window(const uint32_t *win, const Poly &q, uint32_t *out)
{
    std::vector<uint32_t> buf(win, win + kN);
    extend(buf, (size_t)kDeg + 2 * kN);
    std::memset(out, 0, kN * sizeof(uint32_t));
    for (int m = 0; m < kDeg; ++m)
        if (bit(q, m))
            for (int i = 0; i < kN; ++i) out[i] ^= buf[m + i];
}

// numpy's MT19937 state (key[624], pos) after init_genrand(seed) and `offset` raw words.
inline int state_after(uint32_t seed, uint64_t offset, uint32_t *key)
{
    std::vector<uint32_t> w(kN);
    init_genrand(seed, w.data());
    if (offset == 0) {
        std::memcpy(key, w.data(), kN * sizeof(uint32_t));
        return kN;
    }
    const uint64_t T = (offset + kN - 1) / kN;  // twists done
    const uint64_t base = kN * (T - 1);           // key = x[624 T ..], generated from the window at base
    if (base > 0) {
        std::vector<uint32_t> tmp(kN);
        jump_window(w.data(), field().power(base), tmp.data());
        w.swap(tmp);
    }
    extend(w, 2 * kN);
    std::memcpy(key, w.data() + kN, kN * sizeof(uint32_t));
    return (int)(offset - base);
}

}  // namespace rpmt
