// learn-cutoff's bootstrap on gfx950: numpy's legacy MT19937 stream generated in parallel, the
// masked-rejection draws of RandomState.choice turned into value ranks, and the per-resample
// medians of np.median(..., axis=0) selected from them.
//
// The raw word stream is cut into chunks of L = 624 * 2^s words.  Chunk c starts from the
// untempered window x[cL .. cL + 623] (rp_mt19937.hpp notation); the windows come from a doubling
// tree of jumps (k_mt_jump: level j derives chunks [2^j, 2^(j+1)) from chunks [0, 2^j) with
// q = x^(2^j L) mod p).  k_mt_draws then replays each chunk block by block (the three-phase
// twist, 227 / 227 / 170 words) and either counts the accepted draws of both groups (pass 1) or,
// once the host knows where the Ribo group ends, writes each accepted draw's value rank to its
// row-major (k, reps) position (pass 2).  k_median_select reads the rank matrix column tile by
// column tile and radix-selects the one or two middle ranks.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ribophase.h"
#include "rp_mt19937.hpp"

namespace rpboot {

constexpr int kN = 624, kM = 397;
constexpr int kJumpBlock = 256;
constexpr int kDegree = 19937;       // degree of the characteristic polynomial
constexpr int kJumpHalf = 16 * kN;   // 9 984: coefficients [0, 9 984) in the first half, [9 984, 19 937) in the second
constexpr int kJumpWords = 17 * kN;  // x[base .. base + 10 607]: covers m - base + i for either half
constexpr int kPolyWords = 313;      // rp_mt19937.hpp kPolyWords
constexpr int kDrawBlock = 64;       // one wave per chunk
constexpr int kSelCols = 16, kSelBlock = 256, kSelBins = 256;  // 32 KB of histograms: no more than 64 KB of LDS anywhere

__device__ __forceinline__ uint32_t twist(uint32_t a, uint32_t b, uint32_t m)
{
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return m ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ __forceinline__ uint32_t temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// One tree level: window[dst] = jump(window[dst - stride], q) for dst = first + blockIdx.x < n_chunks.  The
// correlation reads x[o .. o + 20 559]; it runs in two halves of the coefficients over a 17-block LDS buffer (42 KB),
// the second half on the sequence regenerated from x[o + 9 984].
__global__ __launch_bounds__(kJumpBlock) void k_mt_jump(uint32_t *__restrict__ windows, long long first, long long stride,
                                                        long long n_chunks, const unsigned long long *__restrict__ q)
{
    __shared__ uint32_t buf[kJumpWords];
    const long long dst = first + blockIdx.x;
    if (dst >= n_chunks) return;
    const uint32_t *src = windows + (dst - stride) * kN;
    const int tid = threadIdx.x;
    for (int i = tid; i < kN; i += kJumpBlock) buf[i] = src[i];
    const int i0 = tid, i1 = tid + kJumpBlock, i2 = min(tid + 2 * kJumpBlock, kN - 1);
    uint32_t a0 = 0, a1 = 0, a2 = 0;
    for (int half = 0; half < 2; ++half) {
        if (half == 1) {  // restart the buffer at x[o + kJumpHalf]: its last block becomes block 0
            uint32_t keep[3];
            for (int r = 0; r < 3; ++r) {
                const int i = tid + r * kJumpBlock;
                if (i < kN) keep[r] = buf[kJumpHalf + i];
            }
            __syncthreads();
            for (int r = 0; r < 3; ++r) {
                const int i = tid + r * kJumpBlock;
                if (i < kN) buf[i] = keep[r];
            }
        }
        __syncthreads();
        for (int b = 1; b < kJumpWords / kN; ++b) {
            const int r0 = b * kN;
            for (int j = tid; j < 227; j += kJumpBlock) buf[r0 + j] = twist(buf[r0 + j - kN], buf[r0 + j - kN + 1], buf[r0 + j - 227]);
            __syncthreads();
            for (int j = 227 + tid; j < 454; j += kJumpBlock) buf[r0 + j] = twist(buf[r0 + j - kN], buf[r0 + j - kN + 1], buf[r0 + j - 227]);
            __syncthreads();
            for (int j = 454 + tid; j < kN; j += kJumpBlock) buf[r0 + j] = twist(buf[r0 + j - kN], buf[r0 + j - kN + 1], buf[r0 + j - 227]);
            __syncthreads();
        }
        // word i of the new window = XOR over the set coefficients m of q of x[o + m + i]
        const int m_lo = half * kJumpHalf, m_hi = half ? kDegree : kJumpHalf;
        for (int w = m_lo / 64; w * 64 < m_hi; ++w) {
            unsigned long long v = q[w];  // uniform: a scalar load and a scalar loop
            while (v) {
                const int m = w * 64 + __builtin_ctzll(v) - m_lo;
                v &= v - 1;
                a0 ^= buf[m + i0];
                a1 ^= buf[m + i1];
                a2 ^= buf[m + i2];
            }
        }
        __syncthreads();
    }
    uint32_t *out = windows + dst * kN;
    out[i0] = a0;
    out[i1] = a1;
    if (tid + 2 * kJumpBlock < kN) out[i2] = a2;
}

struct DrawGroup {
    uint32_t mask, rng;            // masked rejection: accept (w & mask) <= rng
    const void *rank;              // rank of each of the n values (uint16 or uint32)
    void *out;                     // (k, reps) row-major ranks, same width
    long long n_draws;             // k * reps
    int wide;                      // 1: uint32 ranks
};

struct DrawParams {
    DrawGroup g[2];                // 0 = Ribo, 1 = RNA
    long long last_ribo;           // raw word index of the last Ribo draw (-1: none)
    long long last_word;           // raw word index of the last draw of all (-1: none)
    long long chunk_words;         // L
    int chunk_blocks;              // L / 624
};

// Pass 1 (kCount): per chunk, the words each group's mask would accept (every word of the chunk).
// Pass 2 (!kCount): the draws themselves, words <= last_ribo to the Ribo matrix, the ones after up
// to last_word to the RNA matrix, at base[c] + the running count.
template <bool kCount>
__global__ __launch_bounds__(kDrawBlock) void k_mt_draws(const uint32_t *__restrict__ windows, DrawParams P,
                                                         unsigned long long *__restrict__ counts,
                                                         const long long *__restrict__ base_r, const long long *__restrict__ base_n)
{
    __shared__ uint32_t s0[kN], s1[kN];
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    const long long g0 = c * P.chunk_words;
    if (!kCount && g0 > P.last_word) return;
    for (int i = lane; i < kN; i += kDrawBlock) s0[i] = windows[c * kN + i];
    __syncthreads();
    uint32_t *a = s0, *bn = s1;
    unsigned long long cnt_r = 0, cnt_n = 0;
    long long run_r = kCount ? 0 : base_r[c], run_n = kCount ? 0 : base_n[c];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int blk = 0; blk < P.chunk_blocks; ++blk) {
        const long long gb = g0 + (long long)blk * kN;
        if (!kCount && gb > P.last_word) break;
        for (int j = lane; j < 227; j += kDrawBlock) bn[j] = twist(a[j], a[j + 1], a[j + kM]);
        __syncthreads();
        for (int j = 227 + lane; j < 454; j += kDrawBlock) bn[j] = twist(a[j], a[j + 1], bn[j - 227]);
        __syncthreads();
        for (int j = 454 + lane; j < kN; j += kDrawBlock) bn[j] = twist(a[j], j + 1 < kN ? a[j + 1] : bn[0], bn[j - 227]);
        __syncthreads();
        for (int j0 = 0; j0 < kN; j0 += kDrawBlock) {
            const int j = j0 + lane;
            const long long g = gb + j;
            const uint32_t w = j < kN ? temper(bn[j]) : 0u;
            if (kCount) {
                if (j < kN) {
                    cnt_r += (w & P.g[0].mask) <= P.g[0].rng;
                    cnt_n += (w & P.g[1].mask) <= P.g[1].rng;
                }
            } else {
                const uint32_t vr = w & P.g[0].mask, vn = w & P.g[1].mask;
                const bool fr = j < kN && g <= P.last_ribo && vr <= P.g[0].rng;
                const bool fn = j < kN && g > P.last_ribo && g <= P.last_word && vn <= P.g[1].rng;
                const unsigned long long br = __ballot(fr), bnn = __ballot(fn);
                if (fr) {
                    const long long d = run_r + __popcll(br & lt);
                    if (d >= 0 && d < P.g[0].n_draws) {
                        if (P.g[0].wide) ((uint32_t *)P.g[0].out)[d] = ((const uint32_t *)P.g[0].rank)[vr];
                        else ((uint16_t *)P.g[0].out)[d] = ((const uint16_t *)P.g[0].rank)[vr];
                    }
                }
                if (fn) {
                    const long long d = run_n + __popcll(bnn & lt);
                    if (d >= 0 && d < P.g[1].n_draws) {
                        if (P.g[1].wide) ((uint32_t *)P.g[1].out)[d] = ((const uint32_t *)P.g[1].rank)[vn];
                        else ((uint16_t *)P.g[1].out)[d] = ((const uint16_t *)P.g[1].rank)[vn];
                    }
                }
                run_r += __popcll(br);
                run_n += __popcll(bnn);
            }
        }
        uint32_t *t = a;
        a = bn;
        bn = t;
        __syncthreads();
    }
    if (kCount) {
        for (int off = 32; off > 0; off >>= 1) {
            cnt_r += __shfl_xor(cnt_r, off);
            cnt_n += __shfl_xor(cnt_n, off);
        }
        if (lane == 0) {
            counts[2 * c] = cnt_r;
            counts[2 * c + 1] = cnt_n;
        }
    }
}

// Median of every column of a (k, reps) row-major rank matrix (k >= 1): radix select, 8 bits per
// pass from the top of `bits`, of ranks (k-1)/2 and k/2 at once; a column holding nan_rank is NaN
// (np.median's NaN rule).  table[rank] is the value; table[nan_rank] the NaN itself.
template <typename R>
__global__ __launch_bounds__(kSelBlock) void k_median_select(const R *__restrict__ ranks, long long k, long long reps, int bits,
                                                             uint32_t nan_rank, const double *__restrict__ table, uint32_t table_n,
                                                             double *__restrict__ med)
{
    __shared__ uint32_t hist[2][kSelCols][kSelBins];
    __shared__ uint32_t prefix[2][kSelCols], remain[2][kSelCols];
    __shared__ int has_nan[kSelCols];
    const int tid = threadIdx.x, col = tid % kSelCols, sub = tid / kSelCols;
    constexpr int kRowsPerIter = kSelBlock / kSelCols;
    const long long c = (long long)blockIdx.x * kSelCols + col;
    const bool valid = c < reps;
    const bool two = (k % 2) == 0;
    if (tid < kSelCols) {
        prefix[0][tid] = prefix[1][tid] = 0;
        remain[0][tid] = (uint32_t)((k - 1) / 2);
        remain[1][tid] = (uint32_t)(k / 2);
        has_nan[tid] = 0;
    }
    const int passes = (bits + 7) / 8;
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = 8 * (passes - 1 - pass);
        for (int i = tid; i < 2 * kSelCols * kSelBins; i += kSelBlock) (&hist[0][0][0])[i] = 0;
        __syncthreads();
        const uint32_t p0 = prefix[0][col], p1 = prefix[1][col];
        if (valid) {
            bool nan_seen = false;
            for (long long r = sub; r < k; r += kRowsPerIter) {
                const uint32_t v = (uint32_t)ranks[r * reps + c];
                const uint32_t hi = (uint32_t)((unsigned long long)v >> (shift + 8)), d = (v >> shift) & (kSelBins - 1);
                if (pass == 0) nan_seen |= v == nan_rank;
                if (hi == p0) atomicAdd(&hist[0][col][d], 1u);
                if (two && hi == p1) atomicAdd(&hist[1][col][d], 1u);
            }
            if (nan_seen) has_nan[col] = 1;
        }
        __syncthreads();
        if (tid < 2 * kSelCols) {
            const int t = tid / kSelCols, cc = tid % kSelCols;
            if (t == 0 || two) {
                uint32_t left = remain[t][cc], d = 0;
                for (; d < kSelBins - 1; ++d) {
                    const uint32_t h = hist[t][cc][d];
                    if (left < h) break;
                    left -= h;
                }
                remain[t][cc] = left;
                prefix[t][cc] = (prefix[t][cc] << 8) | d;
            }
        }
        __syncthreads();
    }
    if (!valid || sub != 0) return;
    const uint32_t r0 = min(prefix[0][col], table_n - 1), r1 = min(prefix[1][col], table_n - 1);  // (in range by construction)
    double m;
    if (has_nan[col]) m = table[min(nan_rank, table_n - 1)];
    else if (two) m = (table[r0] + table[r1]) / 2.0;
    else m = table[r0];
    med[c] = m;
}

// ---- host side ----------------------------------------------------------------------------------------------------

#define RPB_HIP(call)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) return fail(RP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                              \
    } while (0)

// The distinct values of one group in increasing order (np.partition's order: -0.0 and +0.0 are one value), NaN as
// one flagged top rank, and each value's rank.
struct RankTable {
    std::vector<double> table;
    std::vector<uint32_t> rank;
    uint32_t nan_rank = 0xffffffffu;
    int bits = 1;
    bool wide = false;
};

RankTable rank_table(const double *v, int64_t n)
{
    RankTable rt;
    std::vector<int64_t> order(n);
    for (int64_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const double x = v[a], y = v[b];
        if (std::isnan(y)) return !std::isnan(x);
        return !std::isnan(x) && x < y;
    });
    rt.rank.resize(n);
    int64_t i = 0;
    for (; i < n && !std::isnan(v[order[i]]); ++i) {
        if (rt.table.empty() || v[order[i]] != rt.table.back()) rt.table.push_back(v[order[i]]);
        rt.rank[order[i]] = (uint32_t)(rt.table.size() - 1);
    }
    if (i < n) {
        rt.nan_rank = (uint32_t)rt.table.size();
        rt.table.push_back(v[order[i]]);
        for (; i < n; ++i) rt.rank[order[i]] = rt.nan_rank;
    }
    const uint64_t top = rt.table.empty() ? 0 : rt.table.size() - 1;
    rt.bits = top ? 64 - __builtin_clzll(top) : 1;
    rt.wide = rt.table.size() > 65536;
    return rt;
}

struct DevMem {
    void *p = nullptr;
    ~DevMem()
    {
        if (p) (void)hipFree(p);
    }
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// raw words [o, o + count) from the untempered window x[o .. o + 623]
void host_words(const uint32_t *win, int64_t count, std::vector<uint32_t> &out)
{
    std::vector<uint32_t> x(win, win + rpmt::kN);
    rpmt::extend(x, (size_t)rpmt::kN + (size_t)count);
    out.resize((size_t)count);
    for (int64_t i = 0; i < count; ++i) out[i] = rpmt::temper(x[rpmt::kN + i]);
}

struct BootGroup {
    const double *values = nullptr;
    int64_t n = 0, k = 0;
    double *med = nullptr;
    long long draws = 0;
    bool uses_words = false;
    uint32_t mask = 0, rng = 0;
    RankTable rt;
    size_t rank_off = 0, out_off = 0, table_off = 0, med_off = 0;
};

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}


// rp_bootstrap_medians_dev (include/ribophase.h) without the device selection: `enter_device` makes the device current
// (its guard lives in the caller) and `fail` formats the caller's error message.
using Fail = int (*)(int, const char *, ...);
template <class EnterDevice>
int bootstrap_medians(const double *ribo_values, int64_t n_ribo, int64_t k_ribo, const double *rna_values, int64_t n_rna,
                      int64_t k_rna, int64_t reps, uint32_t seed, double *ribo_medians, double *rna_medians, uint32_t *end_key,
                      int32_t *end_pos, float *ms, EnterDevice enter_device, Fail fail)
{
    const auto t_call = std::chrono::steady_clock::now();
    if (!end_key || !end_pos) return fail(RP_ERR_NULL, "end_key / end_pos is null");
    if (n_ribo < 0 || n_rna < 0 || k_ribo < 0 || k_rna < 0 || reps < 0) return fail(RP_ERR_SIZE, "negative size");
    if (k_ribo >= (1LL << 31) || k_rna >= (1LL << 31) || reps >= (1LL << 40)) return fail(RP_ERR_SIZE, "k or reps too large");
    float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    BootGroup g[2];
    g[0].values = ribo_values, g[0].n = n_ribo, g[0].k = k_ribo, g[0].med = ribo_medians;
    g[1].values = rna_values, g[1].n = n_rna, g[1].k = k_rna, g[1].med = rna_medians;
    for (BootGroup &G : g) {
        G.draws = (long long)G.k * (long long)reps;
        if (G.draws == 0) continue;
        if (G.n == 0) return fail(RP_ERR_SIZE, "cannot draw from an empty group");
        if (!G.values || !G.med) return fail(RP_ERR_NULL, "values / medians is null");
        if (G.n >= (1LL << 32)) return fail(RP_ERR_SIZE, "group of %lld values: more than 2^32", (long long)G.n);
        G.rng = (uint32_t)(G.n - 1);
        uint32_t m = G.rng;
        m |= m >> 1, m |= m >> 2, m |= m >> 4, m |= m >> 8, m |= m >> 16;
        G.mask = m;
        G.uses_words = G.n >= 2;
        if (!G.uses_words) {  // n == 1: numpy draws index 0 without a word; the median of k copies of v
            const double v = G.values[0];
            const double med = std::isnan(v) || (G.k & 1) ? v : (v + v) / 2.0;
            for (int64_t r = 0; r < reps; ++r) G.med[r] = med;
        }
    }
    if (!g[0].uses_words && !g[1].uses_words) {
        *end_pos = rpmt::state_after(seed, 0, end_key);
        t[5] = (float)ms_since(t_call);
        if (ms) std::memcpy(ms, t, sizeof(t));
        return RP_OK;
    }
    bool built = false;
    const auto t_field = std::chrono::steady_clock::now();
    const rpmt::Field &F = rpmt::field(&built);
    if (built) t[0] = (float)ms_since(t_field);
    if (int rc = enter_device()) return rc;

    // data buffers: value ranks, rank matrices, distinct-value tables, medians
    size_t data_bytes = 0;
    for (BootGroup &G : g) {
        if (!G.uses_words) continue;
        G.rt = rank_table(G.values, G.n);
        const size_t w = G.rt.wide ? 4 : 2;
        G.rank_off = data_bytes, data_bytes += align_up((size_t)G.n * w);
        G.out_off = data_bytes, data_bytes += align_up((size_t)G.draws * w);
        G.table_off = data_bytes, data_bytes += align_up(G.rt.table.size() * sizeof(double));
        G.med_off = data_bytes, data_bytes += align_up((size_t)reps * sizeof(double));
    }
    DevMem data;
    if (hipMalloc(&data.p, data_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RP_ERR_WORKSPACE, "bootstrap: the rank matrices need %zu bytes of device memory", data_bytes);
    }
    char *base = (char *)data.p;
    for (BootGroup &G : g) {
        if (!G.uses_words) continue;
        if (G.rt.wide) {
            RPB_HIP(hipMemcpy(base + G.rank_off, G.rt.rank.data(), (size_t)G.n * 4, hipMemcpyHostToDevice));
        } else {
            std::vector<uint16_t> r16(G.rt.rank.begin(), G.rt.rank.end());
            RPB_HIP(hipMemcpy(base + G.rank_off, r16.data(), (size_t)G.n * 2, hipMemcpyHostToDevice));
        }
        RPB_HIP(hipMemcpy(base + G.table_off, G.rt.table.data(), G.rt.table.size() * sizeof(double), hipMemcpyHostToDevice));
    }

    // words the draws are expected to take (acceptance n / (mask + 1) > 1/2), plus a wide margin; doubled if short
    double mean_words = 0, var_words = 0;
    for (BootGroup &G : g)
        if (G.uses_words) {
            const double a = (double)G.n / ((double)G.mask + 1.0);
            mean_words += (double)G.draws / a;
            var_words += (double)G.draws * (1.0 - a) / (a * a);
        }
    long long want_words = (long long)(mean_words + 12.0 * std::sqrt(var_words)) + 4096;
    hipEvent_t ev[5];
    for (auto &e : ev) RPB_HIP(hipEventCreate(&e));
    struct EvFree {
        hipEvent_t *e;
        ~EvFree()
        {
            for (int i = 0; i < 5; ++i) (void)hipEventDestroy(e[i]);
        }
    } ev_free{ev};

    for (int attempt = 0; attempt < 8; ++attempt, want_words *= 2) {
        int s = 4;
        while ((want_words + ((long long)rpmt::kN << s) - 1) / ((long long)rpmt::kN << s) > 8192) ++s;
        const long long L = (long long)rpmt::kN << s;
        const long long C = (want_words + L - 1) / L;
        int levels = 0;
        while ((1LL << levels) < C) ++levels;
        if (s + levels > rpmt::Field::kMaxChunkExp) return fail(RP_ERR_SIZE, "bootstrap: %lld words is too many", want_words);
        t[6] = (float)C;
        t[7] = (float)L;
        const size_t win_off = 0, cnt_off = align_up((size_t)C * rpmt::kN * 4), br_off = cnt_off + align_up((size_t)C * 16),
                     bn_off = br_off + align_up((size_t)C * 8), q_off = bn_off + align_up((size_t)C * 8),
                     total = q_off + align_up((size_t)(levels + 1) * kPolyWords * 8);
        DevMem stream_mem;
        if (hipMalloc(&stream_mem.p, total) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RP_ERR_WORKSPACE, "bootstrap: the chunk windows need %zu bytes of device memory", total);
        }
        char *sb = (char *)stream_mem.p;
        uint32_t *d_win = (uint32_t *)(sb + win_off);
        unsigned long long *d_cnt = (unsigned long long *)(sb + cnt_off);
        long long *d_br = (long long *)(sb + br_off), *d_bn = (long long *)(sb + bn_off);
        unsigned long long *d_q = (unsigned long long *)(sb + q_off);
        std::vector<uint32_t> win0(rpmt::kN);
        rpmt::init_genrand(seed, win0.data());
        RPB_HIP(hipMemcpy(d_win, win0.data(), rpmt::kN * 4, hipMemcpyHostToDevice));
        for (int j = 0; j < levels; ++j)
            RPB_HIP(hipMemcpy(d_q + (size_t)j * kPolyWords, F.chunk[s + j].data(), kPolyWords * 8, hipMemcpyHostToDevice));

        RPB_HIP(hipEventRecord(ev[0], 0));
        for (int j = 0; j < levels; ++j) {
            const long long first = 1LL << j, count = std::min(first, C - first);
            hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)count), dim3(kJumpBlock), 0, 0, d_win, first, first, C,
                               d_q + (size_t)j * kPolyWords);
            RPB_HIP(hipGetLastError());
        }
        RPB_HIP(hipEventRecord(ev[1], 0));
        DrawParams P{};
        for (int i = 0; i < 2; ++i) {
            P.g[i].mask = g[i].uses_words ? g[i].mask : 0u;
            P.g[i].rng = g[i].uses_words ? g[i].rng : 0u;
            P.g[i].wide = g[i].rt.wide ? 1 : 0;
            P.g[i].n_draws = g[i].uses_words ? g[i].draws : 0;
            P.g[i].rank = g[i].uses_words ? base + g[i].rank_off : nullptr;
            P.g[i].out = g[i].uses_words ? base + g[i].out_off : nullptr;
        }
        P.chunk_words = L;
        P.chunk_blocks = (int)(L / rpmt::kN);
        P.last_ribo = P.last_word = -1;
        hipLaunchKernelGGL(k_mt_draws<true>, dim3((unsigned)C), dim3(kDrawBlock), 0, 0, d_win, P, d_cnt,
                           (const long long *)nullptr, (const long long *)nullptr);
        RPB_HIP(hipGetLastError());
        RPB_HIP(hipEventRecord(ev[2], 0));
        std::vector<unsigned long long> cnt((size_t)C * 2);
        RPB_HIP(hipMemcpy(cnt.data(), d_cnt, cnt.size() * 8, hipMemcpyDeviceToHost));

        // where the Ribo draws end (P.last_ribo) and the RNA draws end (P.last_word)
        std::vector<uint32_t> win(rpmt::kN), words;
        auto chunk_words = [&](long long c) -> int {
            hipError_t e = hipMemcpy(win.data(), d_win + (size_t)c * rpmt::kN, rpmt::kN * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(RP_ERR_HIP, "bootstrap: window copy failed: %s", hipGetErrorString(e));
            host_words(win.data(), L, words);
            return RP_OK;
        };
        std::vector<long long> br((size_t)C, 0), bn((size_t)C, 0);
        long long cb = 0, rna_after = 0, ce = 0;
        bool short_of_words = false;
        if (g[0].uses_words) {
            long long cum = 0, c = 0;
            while (c < C && cum + (long long)cnt[2 * c] < g[0].draws) br[c] = cum, cum += (long long)cnt[2 * c], ++c;
            if (c == C) {
                short_of_words = true;
            } else {
                br[c] = cum;
                cb = c;
                int rc = chunk_words(cb);
                if (rc != RP_OK) return rc;
                long long need = g[0].draws - cum, i = 0;
                for (; i < L; ++i)
                    if ((words[i] & g[0].mask) <= g[0].rng && --need == 0) break;
                P.last_ribo = cb * L + i;
                for (++i; i < L; ++i) rna_after += (words[i] & g[1].mask) <= g[1].rng;
            }
        } else {
            rna_after = (long long)cnt[1];
        }
        P.last_word = P.last_ribo;
        ce = cb;
        if (!short_of_words && g[1].uses_words) {
            long long c = cb;
            bn[cb] = 0;
            long long cum = rna_after;
            if (cum < g[1].draws) {
                for (c = cb + 1; c < C && cum + (long long)cnt[2 * c + 1] < g[1].draws; ++c) bn[c] = cum, cum += (long long)cnt[2 * c + 1];
                if (c == C) short_of_words = true;
                else bn[c] = cum;
            }
            if (!short_of_words) {
                ce = c;
                if (ce != cb || !g[0].uses_words) {
                    int rc = chunk_words(ce);
                    if (rc != RP_OK) return rc;
                }
                long long need = g[1].draws - (ce == cb ? 0 : cum);
                long long i = ce == cb ? P.last_ribo + 1 - ce * L : 0;
                for (; i < L; ++i)
                    if ((words[i] & g[1].mask) <= g[1].rng && --need == 0) break;
                P.last_word = ce * L + i;
            }
        }
        if (short_of_words) continue;

        RPB_HIP(hipMemcpy(d_br, br.data(), (size_t)C * 8, hipMemcpyHostToDevice));
        RPB_HIP(hipMemcpy(d_bn, bn.data(), (size_t)C * 8, hipMemcpyHostToDevice));
        RPB_HIP(hipEventRecord(ev[3], 0));
        hipLaunchKernelGGL(k_mt_draws<false>, dim3((unsigned)(ce + 1)), dim3(kDrawBlock), 0, 0, d_win, P,
                           (unsigned long long *)nullptr, d_br, d_bn);
        RPB_HIP(hipGetLastError());
        RPB_HIP(hipEventRecord(ev[4], 0));
        RPB_HIP(hipEventSynchronize(ev[4]));
        (void)hipEventElapsedTime(&t[1], ev[0], ev[1]);
        (void)hipEventElapsedTime(&t[2], ev[1], ev[2]);
        (void)hipEventElapsedTime(&t[3], ev[3], ev[4]);

        // numpy's state after word P.last_word: key = x[624 T ..], T = ceil((last + 1) / 624)
        {
            const long long used = P.last_word + 1;
            const long long T = (used + rpmt::kN - 1) / rpmt::kN, o = ce * L;
            std::vector<uint32_t> x(rpmt::kN);
            if (ce == 0) {
                x = win0;
            } else {
                RPB_HIP(hipMemcpy(x.data(), d_win + (size_t)ce * rpmt::kN, rpmt::kN * 4, hipMemcpyDeviceToHost));
            }
            rpmt::extend(x, (size_t)(rpmt::kN * T - o + rpmt::kN));
            std::memcpy(end_key, x.data() + (rpmt::kN * T - o), rpmt::kN * 4);
            *end_pos = (int32_t)(used - rpmt::kN * (T - 1));
        }

        RPB_HIP(hipEventRecord(ev[0], 0));
        for (BootGroup &G : g) {
            if (!G.uses_words) continue;
            const unsigned grid = (unsigned)((reps + kSelCols - 1) / kSelCols);
            double *d_med = (double *)(base + G.med_off);
            const double *d_tab = (const double *)(base + G.table_off);
            if (G.rt.wide)
                hipLaunchKernelGGL(k_median_select<uint32_t>, dim3(grid), dim3(kSelBlock), 0, 0,
                                   (const uint32_t *)(base + G.out_off), (long long)G.k, (long long)reps, G.rt.bits, G.rt.nan_rank,
                                   d_tab, (uint32_t)G.rt.table.size(), d_med);
            else
                hipLaunchKernelGGL(k_median_select<uint16_t>, dim3(grid), dim3(kSelBlock), 0, 0,
                                   (const uint16_t *)(base + G.out_off), (long long)G.k, (long long)reps, G.rt.bits, G.rt.nan_rank,
                                   d_tab, (uint32_t)G.rt.table.size(), d_med);
            RPB_HIP(hipGetLastError());
        }
        RPB_HIP(hipEventRecord(ev[1], 0));
        for (BootGroup &G : g)
            if (G.uses_words) RPB_HIP(hipMemcpy(G.med, base + G.med_off, (size_t)reps * 8, hipMemcpyDeviceToHost));
        (void)hipEventElapsedTime(&t[4], ev[0], ev[1]);
        t[5] = (float)ms_since(t_call);
        if (ms) std::memcpy(ms, t, sizeof(t));
        return RP_OK;
    }
    return fail(RP_ERR_SIZE, "bootstrap: the draws did not end within %lld raw words", want_words);
}

#undef RPB_HIP

}  // namespace rpboot
