// noise_level.hip -- the reference's value-based noise level function (utils/raw_util.py:248-322: get_poisson_lambda, get_poisson_lambda_all_images,
// get_regression_result_all_images): the noisy pixels grouped by the clean value they sit on, the unbiased std of every group, and a Theil-Sen
// line of std on clean value.
//
//   moments   one pass over (clean, noisy): per level l = rint(clean * scale) the count, sum q and sum q^2 of q = rint(noisy * 2^30) + 2^32,
//             all integers, added with 64-bit integer atomics.  Integer adds commute: the table does not depend on the order of the elements,
//             on the split into calls or on the grid.  A wave whose 256 elements of a trip sit on one level adds them up in registers and
//             issues the four atomics from one lane (a dark or clipped frame puts every element on one cache line).
//   stats     one thread per level: n * sum q^2 - (sum q)^2 exactly in 128 bits, one conversion, two IEEE divisions, a square root
//   curve     the levels with count >= 1 in ascending order, cut at the lower median on request, NaN stds dropped, compacted on the device
//   fit       sklearn's TheilSenRegressor for one feature: the spatial median (modified Weiszfeld) of the (intercept, slope) of every pair
//             of curve points.  No pair is stored: a step recomputes them.  Every sum has a fixed order: a workgroup's partial goes to its
//             workspace slot, the slots are summed in slot order.  The grid is a constant, so the bits depend on (x, y, m) alone.
//
// No floating-point atomics, no cooperative launch, no kernel that waits for another workgroup, no host read.
#include "nd_common.h"
#include "block_sum.h"
#include "u128.h"
#include <float.h>

// The fit mirrors numpy operation by operation (the order of the long sums apart): a product and a sum stay two roundings.
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int LM_THREADS = 256;
constexpr int LM_VEC = 4;                                  // elements per thread and trip: one float4 of each tensor
constexpr int LM_CHUNK = LM_THREADS * LM_VEC;              // elements of one trip of a workgroup
constexpr int LM_TRIPS = 4;                                // trips per workgroup before the grid is capped
constexpr int LM_MAX_BLOCKS = 2048;                        // eight workgroups per CU
constexpr int LM_MAX_LEVELS = 1 << 24;                     // a level is exact in fp32
constexpr int64_t LM_MAX_N = (1ll << 31) - 1;              // elements of one call, and of one table (the caller counts: see the header)
constexpr float LM_NOISY_LIMIT = 4.0f;
constexpr float LM_GRID_EPS = 1e-6f;                       // the reference's membership test: torch.abs(clean - value) < 1e-6

constexpr int LV_OFF_GRID = -1, LV_BAD_NOISY = -2, LV_ABSENT = -3;

__device__ __forceinline__ void lm_atomic_add(u64* p, u64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// cnt elements with sum q = sq and sum q^2 = hi * 2^64 + lo into level l.  The high word takes the carry of the low word, read from the value
// the low word's atomic returns: the number of wraps of the low word is the number of adds that saw one, in any order.
__device__ __forceinline__ void lm_add(u64* __restrict__ table, int l, u64 cnt, u64 sq, u64 lo, u64 hi) {
    u64* e = table + (size_t)l * 4;
    lm_atomic_add(e, cnt);
    lm_atomic_add(e + 1, sq);
    const u64 old = __hip_atomic_fetch_add(e + 2, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hi += (u64)(old + lo < old);
    if (hi) lm_atomic_add(e + 3, hi);
}

// The level of (clean, noisy), or why the element is left out.  q is defined for a level >= 0 only.
__device__ __forceinline__ int lm_classify(float c, float v, float scale, int n_levels, u64& q) {
    const float lf = rintf(c * scale);
    if (!(lf >= 0.0f && lf < (float)n_levels)) return LV_OFF_GRID;             // NaN and inf fail the first comparison
    if (!(fabsf(c - lf / scale) < LM_GRID_EPS)) return LV_OFF_GRID;            // IEEE division: the value the packer gives that code
    if (!(fabsf(v) < LM_NOISY_LIMIT)) return LV_BAD_NOISY;                     // NaN, inf, |noisy| >= 4
    q = (u64)((long long)rint((double)v * 1073741824.0) + (1ll << 32));        // v * 2^30 is exact; 0 < q < 2^33
    return (int)lf;
}

__global__ __launch_bounds__(LM_THREADS) void level_moments_kernel(const float* __restrict__ clean, const float* __restrict__ noisy, int64_t n,
                                                                   float scale, int n_levels, u64* __restrict__ table, u64* __restrict__ counters) {
    const int t = threadIdx.x;
    const bool vec = ((((uintptr_t)clean) | ((uintptr_t)noisy)) & 15u) == 0;
    const int64_t nchunk = (n + LM_CHUNK - 1) / LM_CHUNK;
    uint32_t off = 0, bad = 0;                                                 // a thread sees fewer than 2^31 elements
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * LM_CHUNK;
        const bool full = base + LM_CHUNK <= n;                                // the same for the whole workgroup
        int l[LM_VEC];
        u64 q[LM_VEC];
        if (vec && full) {
            const f32x4 cv = nd_ld4(clean + base + (int64_t)t * 4), nv = nd_ld4(noisy + base + (int64_t)t * 4);
#pragma unroll
            for (int k = 0; k < LM_VEC; ++k) l[k] = lm_classify(cv[k], nv[k], scale, n_levels, q[k]);
        } else {                                                               // a tensor off 16 bytes, or the last chunk: lane-strided scalars
#pragma unroll
            for (int k = 0; k < LM_VEC; ++k) {
                const int64_t i = base + (int64_t)k * LM_THREADS + t;
                l[k] = i < n ? lm_classify(clean[i], noisy[i], scale, n_levels, q[k]) : LV_ABSENT;
            }
        }
        bool uniform = false;
        int l0 = 0;
        if (full) {                                                            // all 64 lanes are here
            l0 = __builtin_amdgcn_readfirstlane(l[0]);
            uniform = __all(l0 >= 0 && l[0] == l0 && l[1] == l0 && l[2] == l0 && l[3] == l0) != 0;
        }
        if (uniform) {
            u64 sq = 0;
            u128 s2 = 0;
#pragma unroll
            for (int k = 0; k < LM_VEC; ++k) {
                sq += q[k];
                s2 += (u128)q[k] * q[k];
            }
            u64 lo = (u64)s2, hi = (u64)(s2 >> 64);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {                                 // both lanes of a pair form the same sums
                sq += __shfl_xor(sq, o);
                const u64 olo = __shfl_xor(lo, o), ohi = __shfl_xor(hi, o);
                lo += olo;
                hi += ohi + (u64)(lo < olo);
            }
            if ((t & 63) == 0) lm_add(table, l0, (u64)(64 * LM_VEC), sq, lo, hi);
        } else {
#pragma unroll
            for (int k = 0; k < LM_VEC; ++k) {
                if (l[k] >= 0) {
                    const u128 s2 = (u128)q[k] * q[k];
                    lm_add(table, l[k], 1, q[k], (u64)s2, (u64)(s2 >> 64));
                } else {
                    off += l[k] == LV_OFF_GRID;
                    bad += l[k] == LV_BAD_NOISY;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        off += __shfl_xor(off, o);
        bad += __shfl_xor(bad, o);
    }
    if ((t & 63) == 0) {
        if (off) lm_atomic_add(counters, (u64)off);
        if (bad) lm_atomic_add(counters + 1, (u64)bad);
    }
}

// Zeroes the table and the two counters: a plain kernel, so that a reset is a kernel node of a captured graph like every other step.
__global__ __launch_bounds__(256) void level_reset_kernel(u64* __restrict__ table, int64_t n_words, u64* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) table[i] = 0;
    if (i < 2) counters[i] = 0;
}

__global__ __launch_bounds__(256) void level_stats_kernel(const u64* __restrict__ table, int n_levels, int64_t* __restrict__ count,
                                                          double* __restrict__ mean, double* __restrict__ std) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_levels) return;
    const u64* e = table + (size_t)l * 4;
    const u64 n = e[0], s1 = e[1];
    const u128 s2 = ((u128)e[3] << 64) | (u128)e[2];
    const double nan = __builtin_nan("");
    count[l] = (int64_t)n;
    double m = nan, s = nan;
    if (n >= 1) m = (double)(int64_t)(s1 - (n << 32)) / (double)n * 0x1p-30;   // |sum q - n 2^32| < n 2^32 <= 2^63
    if (n >= 2) {
        const u128 num = (u128)n * s2 - (u128)s1 * s1;                         // >= 0 (Cauchy-Schwarz), < 2^128 while n < 2^31
        s = sqrt(nd_u128_to_double(num) / (double)n / (double)(n - 1)) * 0x1p-30;
    }
    mean[l] = m;
    std[l] = s;
}

constexpr int LC_THREADS = 1024;

// Exclusive prefix sum of v over the workgroup; `total` is the sum.  lds: LC_THREADS / 64 + 1 ints.  Ends with every thread past its reads.
__device__ __forceinline__ int lc_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < LC_THREADS / 64; ++k) {
            const int s = lds[k];
            lds[k] = run;
            run += s;
        }
        lds[LC_THREADS / 64] = run;
    }
    __syncthreads();
    const int ex = lds[w] + inc - v;
    total = lds[LC_THREADS / 64];
    __syncthreads();
    return ex;
}

// One workgroup.  Everything past the m kept points is set to NaN, so the outputs are defined in full.
__global__ __launch_bounds__(LC_THREADS) void level_curve_kernel(const int64_t* __restrict__ count, const double* __restrict__ std, int n_levels,
                                                                 float scale, int below_median, double* __restrict__ x, double* __restrict__ y,
                                                                 int* __restrict__ m_out) {
    __shared__ int lds[LC_THREADS / 64 + 1];
    const int t = threadIdx.x;
    int mine = 0, U = 0;
    for (int l = t; l < n_levels; l += LC_THREADS) mine += count[l] >= 1;
    lc_scan(mine, lds, U);
    const int K = below_median ? (U - 1) / 2 + 1 : U;                          // value <= torch.median(unique): the lower median
    int seen = 0, kept = 0;
    for (int base = 0; base < n_levels; base += LC_THREADS) {
        const int l = base + t;
        const bool present = l < n_levels && count[l] >= 1;
        int tot;
        const int rank = seen + lc_scan(present, lds, tot);
        seen += tot;
        const double s = present ? std[l] : 0.0;
        const bool keep = present && rank < K && s == s;
        const int pos = kept + lc_scan(keep, lds, tot);
        kept += tot;
        if (keep) {
            x[pos] = (double)((float)l / scale);                               // the fp32 clean value, as sklearn is given it
            y[pos] = s;
        }
    }
    const double nan = __builtin_nan("");
    for (int i = kept + t; i < n_levels; i += LC_THREADS) {
        x[i] = nan;
        y[i] = nan;
    }
    if (t == 0) *m_out = kept;
}

// ------------------------------------------------------------------ Theil-Sen

constexpr int TS_THREADS = 256;
constexpr int TS_BLOCKS = 1024;                            // a constant: the order of every sum is a function of (x, y, m) or of the pair table
constexpr int TS_SUMS = 6;
constexpr int TS_HEAD = 8;                                 // doubles in front of the slots: old[2], then {done, n_iter} as two ints
constexpr int TS_MAX_M = 1 << 24;
constexpr int TS_MAX_ITER = 1 << 16;

struct ts_head {
    double old[2];
    int done, n_iter;
};

__device__ __forceinline__ int ts_m(const int* m, int max_m) {
    const int v = *m;
    return v < 0 ? 0 : (v > max_m ? max_m : v);
}

// MEAN: sum of the points.  Otherwise the sums of one modified Weiszfeld step about head->old:
// sum d / |d|  (2), sum P / |d|  (2), sum 1 / |d|, and the number of points with |d| < DBL_EPSILON (or NaN), which are left out of the others.
template <bool MEAN>
__global__ __launch_bounds__(TS_THREADS) void ts_partial_kernel(const double* __restrict__ x, const double* __restrict__ y, const int* __restrict__ m_dev,
                                                                int max_m, const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                                double* __restrict__ ws) {
    const ts_head* head = reinterpret_cast<const ts_head*>(ws);
    if (!MEAN && head->done) return;
    __shared__ double red[TS_SUMS][4];
    const int t = threadIdx.x, b = blockIdx.x;
    const int m = ts_m(m_dev, max_m);
    const double o0 = MEAN ? 0.0 : head->old[0], o1 = MEAN ? 0.0 : head->old[1];
    double acc[TS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto point = [&](double xi, double yi, double xj, double yj) {
        const double slope = (yj - yi) / (xj - xi);
        const double icpt = yi - slope * xi;
        if (MEAN) {
            acc[0] += icpt;
            acc[1] += slope;
            return;
        }
        const double d0 = icpt - o0, d1 = slope - o1;
        const double r = sqrt(d0 * d0 + d1 * d1);
        if (r >= DBL_EPSILON) {
            acc[0] += d0 / r;
            acc[1] += d1 / r;
            acc[2] += icpt / r;
            acc[3] += slope / r;
            acc[4] += 1.0 / r;
        } else {
            acc[5] += 1.0;
        }
    };
    if (pairs) {
        const double nan = __builtin_nan("");
        for (int64_t p = (int64_t)b * TS_THREADS + t; p < n_pairs; p += (int64_t)TS_BLOCKS * TS_THREADS) {
            const int i = pairs[2 * p], j = pairs[2 * p + 1];
            if (i >= 0 && i < m && j >= 0 && j < m) point(x[i], y[i], x[j], y[j]);
            else point(nan, nan, nan, nan);                                    // an index outside the curve is never read
        }
    } else {
        for (int i = b; i < m - 1; i += TS_BLOCKS) {                           // rows dealt round-robin: every workgroup gets long and short ones
            const double xi = x[i], yi = y[i];
            for (int j = i + 1 + t; j < m; j += TS_THREADS) point(xi, yi, x[j], y[j]);
        }
    }
    block_sum_all<TS_SUMS>(acc, red);
    if (t == 0) {
        double* s = ws + TS_HEAD + (size_t)b * TS_SUMS;
#pragma unroll
        for (int k = 0; k < TS_SUMS; ++k) s[k] = acc[k];
    }
}

// One workgroup: the slots in slot order (thread t takes t, t + 256, ..., then the tree), then the start (MEAN) or the step of thread 0.
template <bool MEAN>
__global__ __launch_bounds__(TS_THREADS) void ts_finalize_kernel(const int* __restrict__ m_dev, int max_m, int has_pairs, int64_t n_pairs, double tol2,
                                                                 double* __restrict__ ws, double* __restrict__ out) {
    ts_head* head = reinterpret_cast<ts_head*>(ws);
    if (!MEAN && head->done) return;
    __shared__ double red[TS_SUMS][4];
    double S[TS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < TS_BLOCKS; b += TS_THREADS) {
        const double* s = ws + TS_HEAD + (size_t)b * TS_SUMS;
#pragma unroll
        for (int k = 0; k < TS_SUMS; ++k) S[k] += s[k];
    }
    block_sum_all<TS_SUMS>(S, red);
    if (threadIdx.x != 0) return;
    if (MEAN) {
        const int m = ts_m(m_dev, max_m);
        const double nan = __builtin_nan("");
        const double P = has_pairs ? (double)n_pairs : 0.5 * (double)m * (double)(m - 1);      // exact: m < 2^24
        head->n_iter = 0;
        out[2] = 0.0;
        if (m == 0 || (!has_pairs && m == 1)) {                                // the reference returns (0, 0) without points and raises with one
            head->done = 1;
            out[0] = out[1] = m == 0 ? 0.0 : nan;
            out[3] = 0.0;
            return;
        }
        head->done = 0;
        head->old[0] = S[0] / P;
        head->old[1] = S[1] / P;
        out[0] = head->old[0];
        out[1] = head->old[1];
        out[3] = P;
        return;
    }
    const double o0 = head->old[0], o1 = head->old[1];
    const double in_x = S[5] > 0.0 ? 1.0 : 0.0;
    double qn = sqrt(S[0] * S[0] + S[1] * S[1]);
    double dir0 = 1.0, dir1 = 1.0;
    if (qn > DBL_EPSILON) {
        dir0 = S[2] / S[4];
        dir1 = S[3] / S[4];
    } else {
        qn = 1.0;
    }
    const double ratio = in_x / qn;
    const double w_new = fmax(0.0, 1.0 - ratio), w_old = fmin(1.0, ratio);
    const double n0 = w_new * dir0 + w_old * o0, n1 = w_new * dir1 + w_old * o1;
    const double e0 = o0 - n0, e1 = o1 - n1;
    const int it = head->n_iter + 1;
    head->n_iter = it;
    out[0] = n0;
    out[1] = n1;
    out[2] = (double)it;
    if (e0 * e0 + e1 * e1 < tol2) {                                            // NaN never stops: the steps run out, as they do in sklearn
        head->done = 1;
    } else {
        head->old[0] = n0;
        head->old[1] = n1;
    }
}

bool lm_levels_ok(int n_levels, float scale) { return n_levels >= 1 && n_levels <= LM_MAX_LEVELS && scale > 0.0f && scale <= 16777216.0f; }

}  // namespace

extern "C" int64_t nd_level_table_bytes(int n_levels) {
    ND_REQUIRE(n_levels >= 1 && n_levels <= LM_MAX_LEVELS, ND_E_BADARG, "nd_level_table_bytes: n_levels=%d must be in [1, %d]", n_levels, LM_MAX_LEVELS);
    return (int64_t)n_levels * 4 * (int64_t)sizeof(u64);
}

extern "C" int nd_level_moments_reset(uint64_t* table, int n_levels, uint64_t* counters, void* stream) {
    ND_REQUIRE(table && counters, ND_E_BADARG, "nd_level_moments_reset: null pointer");
    ND_REQUIRE(n_levels >= 1 && n_levels <= LM_MAX_LEVELS, ND_E_BADARG, "nd_level_moments_reset: n_levels=%d must be in [1, %d]", n_levels, LM_MAX_LEVELS);
    ND_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)counters & 7u) == 0, ND_E_BADARG, "nd_level_moments_reset: table and counters must be 8-byte aligned");
    const int64_t n_words = (int64_t)n_levels * 4;
    hipLaunchKernelGGL(level_reset_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (u64*)table, n_words, (u64*)counters);
    return nd_launch_status("nd_level_moments_reset");
}

extern "C" int nd_level_moments_f32(const float* clean, const float* noisy, int64_t n, float scale, int n_levels, uint64_t* table, uint64_t* counters,
                                    void* stream) {
    ND_REQUIRE(clean && noisy && table && counters, ND_E_BADARG, "nd_level_moments_f32: null pointer");
    ND_REQUIRE(n >= 1 && n <= LM_MAX_N, ND_E_BADARG, "nd_level_moments_f32: n must be in [1, 2^31 - 1]");
    ND_REQUIRE(lm_levels_ok(n_levels, scale), ND_E_BADARG, "nd_level_moments_f32: n_levels=%d must be in [1, %d] and scale in (0, 2^24]", n_levels, LM_MAX_LEVELS);
    ND_REQUIRE(((uintptr_t)clean & 3u) == 0 && ((uintptr_t)noisy & 3u) == 0, ND_E_BADARG, "nd_level_moments_f32: clean and noisy must be 4-byte aligned");
    ND_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)counters & 7u) == 0, ND_E_BADARG, "nd_level_moments_f32: table and counters must be 8-byte aligned");
    const int64_t nchunk = (n + LM_CHUNK - 1) / LM_CHUNK, want = (nchunk + LM_TRIPS - 1) / LM_TRIPS;
    const unsigned grid = (unsigned)(want < LM_MAX_BLOCKS ? want : LM_MAX_BLOCKS);
    hipLaunchKernelGGL(level_moments_kernel, dim3(grid), dim3(LM_THREADS), 0, (hipStream_t)stream, clean, noisy, n, scale, n_levels, (u64*)table,
                       (u64*)counters);
    return nd_launch_status("nd_level_moments_f32");
}

extern "C" int nd_level_stats_f64(const uint64_t* table, int n_levels, int64_t* count, double* mean, double* std, void* stream) {
    ND_REQUIRE(table && count && mean && std, ND_E_BADARG, "nd_level_stats_f64: null pointer");
    ND_REQUIRE(n_levels >= 1 && n_levels <= LM_MAX_LEVELS, ND_E_BADARG, "nd_level_stats_f64: n_levels=%d must be in [1, %d]", n_levels, LM_MAX_LEVELS);
    ND_REQUIRE((((uintptr_t)table | (uintptr_t)count | (uintptr_t)mean | (uintptr_t)std) & 7u) == 0, ND_E_BADARG,
               "nd_level_stats_f64: pointers must be 8-byte aligned");
    hipLaunchKernelGGL(level_stats_kernel, dim3((unsigned)nd_cdiv(n_levels, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)table, n_levels, count,
                       mean, std);
    return nd_launch_status("nd_level_stats_f64");
}

extern "C" int nd_level_curve_f64(const int64_t* count, const double* std, int n_levels, float scale, int below_median, double* x, double* y, int32_t* m,
                                  void* stream) {
    ND_REQUIRE(count && std && x && y && m, ND_E_BADARG, "nd_level_curve_f64: null pointer");
    ND_REQUIRE(lm_levels_ok(n_levels, scale), ND_E_BADARG, "nd_level_curve_f64: n_levels=%d must be in [1, %d] and scale in (0, 2^24]", n_levels, LM_MAX_LEVELS);
    ND_REQUIRE(below_median == 0 || below_median == 1, ND_E_BADARG, "nd_level_curve_f64: below_median=%d must be 0 or 1", below_median);
    ND_REQUIRE((((uintptr_t)count | (uintptr_t)std | (uintptr_t)x | (uintptr_t)y) & 7u) == 0 && ((uintptr_t)m & 3u) == 0, ND_E_BADARG,
               "nd_level_curve_f64: count, std, x, y must be 8-byte aligned and m 4-byte aligned");
    hipLaunchKernelGGL(level_curve_kernel, dim3(1), dim3(LC_THREADS), 0, (hipStream_t)stream, count, std, n_levels, scale, below_median, x, y, (int*)m);
    return nd_launch_status("nd_level_curve_f64");
}

extern "C" int64_t nd_theil_sen_workspace_bytes(int max_m, int64_t n_pairs) {
    ND_REQUIRE(max_m >= 1 && max_m <= TS_MAX_M && n_pairs >= 0, ND_E_BADARG, "nd_theil_sen_workspace_bytes: max_m must be in [1, 2^24] and n_pairs >= 0");
    return (int64_t)(TS_HEAD + TS_BLOCKS * TS_SUMS) * (int64_t)sizeof(double);
}

extern "C" int nd_theil_sen_f64(const double* x, const double* y, const int32_t* m, int max_m, const int32_t* pairs, int64_t n_pairs, int max_iter,
                                double tol, double* out, void* workspace, void* stream) {
    static_assert(sizeof(ts_head) <= TS_HEAD * sizeof(double), "the head fits in front of the slots");
    ND_REQUIRE(x && y && m && out && workspace, ND_E_BADARG, "nd_theil_sen_f64: null pointer (only pairs may be NULL)");
    ND_REQUIRE(max_m >= 1 && max_m <= TS_MAX_M, ND_E_BADARG, "nd_theil_sen_f64: max_m=%d must be in [1, 2^24]", max_m);
    ND_REQUIRE(pairs ? n_pairs >= 1 : n_pairs == 0, ND_E_BADARG, "nd_theil_sen_f64: n_pairs must be positive with a pair table and 0 without one");
    ND_REQUIRE(max_iter >= 1 && max_iter <= TS_MAX_ITER, ND_E_BADARG, "nd_theil_sen_f64: max_iter=%d must be in [1, %d]", max_iter, TS_MAX_ITER);
    ND_REQUIRE(tol >= 0.0 && tol < 1e150, ND_E_BADARG, "nd_theil_sen_f64: tol must be finite and not negative");
    ND_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)out | (uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)m | (uintptr_t)pairs) & 3u) == 0,
               ND_E_BADARG, "nd_theil_sen_f64: x, y, out, workspace must be 8-byte aligned, m and pairs 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    const int has_pairs = pairs != nullptr;
    const double tol2 = tol * tol;
    hipLaunchKernelGGL(ts_partial_kernel<true>, dim3(TS_BLOCKS), dim3(TS_THREADS), 0, st, x, y, (const int*)m, max_m, pairs, n_pairs, ws);
    hipLaunchKernelGGL(ts_finalize_kernel<true>, dim3(1), dim3(TS_THREADS), 0, st, (const int*)m, max_m, has_pairs, n_pairs, tol2, ws, out);
    int e = nd_launch_status("nd_theil_sen_f64 (start)");
    if (e) return e;
    for (int it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(ts_partial_kernel<false>, dim3(TS_BLOCKS), dim3(TS_THREADS), 0, st, x, y, (const int*)m, max_m, pairs, n_pairs, ws);
        hipLaunchKernelGGL(ts_finalize_kernel<false>, dim3(1), dim3(TS_THREADS), 0, st, (const int*)m, max_m, has_pairs, n_pairs, tol2, ws, out);
    }
    return nd_launch_status("nd_theil_sen_f64 (steps)");
}
