// noise_stats.hip -- scoring of generated noise (utils/util.py:185-255, utils/raw_util.py:161-189): value histograms, the KL divergences of
// two histograms, and the 3 x 3 sliding-window std / mean with the line fit of std on mean per (sample, channel).
//
//   histogram    np.histogram(data, bin_edges) with an explicit edge array: v is in bin i when edges[i] <= (double)v < edges[i + 1], the last
//                bin also takes v == edges[n_bins]; NaN, +-inf and everything outside [edges[0], edges[n_bins]] is counted nowhere
//   KL           p = hist_p / n_p, q = hist_q / n_q; forward sum p log(p / q), inverse sum q log(q / p), their mean; over the bins with p > 0, q > 0
//   patch fit    F.unfold(3, padding 1) + torch.std_mean(dim=2) (zero padding, divisor 8), then LinearRegression().fit(mean, std) in closed form
//
// Determinism: the only atomics are integer adds into a workgroup's LDS histogram, and integer addition is associative.  Every workgroup
// writes its partial (counts, or the four fp64 sums of a tile) to its own workspace slot with plain stores; a finalize kernel sums a set's
// slots in a fixed order.  The slot layout of a set depends on its own size only, so a set's result does not depend on the other sets in the call.
#include "nd_common.h"
#include "block_sum.h"

#ifndef ND_HIST_VARIANT
#define ND_HIST_VARIANT 0      // 0: one LDS histogram per workgroup, one atomic per element (shipped: the measured choice);
#endif                         // 1: one histogram per wave while n_bins <= HIST_WAVE_BINS; 2: a lane folds its run of equal bins into one atomic

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_VEC = 8;                                      // float4 loads per thread and trip
constexpr int HIST_CHUNK = HIST_THREADS * 4 * HIST_VEC;           // elements of one trip of a workgroup: 8192
constexpr int HIST_TRIPS = 2;                                    // trips per workgroup before the grid is capped
constexpr int HIST_MAX_BLOCKS = 1024;                            // workgroups per set at most: four per CU
constexpr int HIST_MAX_BINS = 4096;
constexpr int HIST_WAVE_BINS = 1024;                             // variant 1: four private histograms of this many bins are the 16 KB of one of 4096
constexpr int64_t HIST_MAX_N = 1ll << 40;                        // / HIST_MAX_BLOCKS: a workgroup counts fewer than 2^32 elements, so a uint32 partial cannot wrap

// The bin of v in the n_bins + 1 edges E (LDS), or -1.  A guess from the spacing of the interior edges E[1] .. E[n_bins - 1] is checked against
// the table itself; where it is off (edges that are not evenly spaced, or an element next to an edge) the table is searched.
__device__ __forceinline__ int hist_bin(float v, const double* E, int n_bins, double e_first, double e_last, double lo, double inv_w) {
    const double d = (double)v;
    if (!(d >= e_first && d <= e_last)) return -1;               // the two end edges, kept in registers; NaN fails both
    double t = (d - lo) * inv_w;
    t = t < -1.0 ? -1.0 : (t > (double)n_bins ? (double)n_bins : t);
    int g = (int)floor(t) + 1;                                   // t in [-1, n_bins]: the conversion is defined
    g = g < 0 ? 0 : (g > n_bins - 1 ? n_bins - 1 : g);
    if (E[g] <= d && (d < E[g + 1] || g == n_bins - 1)) return g;
    int a = 0, b = n_bins;                                       // E[a] <= d, and d < E[b] or b == n_bins
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (E[m] <= d) a = m; else b = m;
    }
    return a;
}

// One workgroup counts chunks blockIdx.x, blockIdx.x + gridDim.x, ... of set blockIdx.y into its LDS histogram(s) and stores the sum of them
// as its partial.  COPIES: 1, or 4 = one histogram per wave.  FOLD: a lane keeps (bin, count) of its current run of equal bins in registers.
template <int COPIES, bool FOLD>
__global__ __launch_bounds__(HIST_THREADS) void histogram_partial_kernel(const float* __restrict__ x, int64_t n, const double* __restrict__ edges,
                                                                         int n_bins, uint32_t* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hist_lds[];
    double* E = reinterpret_cast<double*>(hist_lds);                                  // n_bins + 1 edges
    uint32_t* Hs = reinterpret_cast<uint32_t*>(hist_lds + (size_t)(n_bins + 1) * 8);      // COPIES x n_bins counts
    const int t = threadIdx.x, s = blockIdx.y;
    for (int i = t; i <= n_bins; i += HIST_THREADS) E[i] = edges[i];
    for (int i = t; i < COPIES * n_bins; i += HIST_THREADS) Hs[i] = 0u;
    __syncthreads();
    uint32_t* H = Hs + (COPIES > 1 ? (t >> 6) * n_bins : 0);
    const double lo = E[n_bins > 2 ? 1 : 0], hi = E[n_bins > 2 ? n_bins - 1 : n_bins];
    const double inv_w = (double)(n_bins > 2 ? n_bins - 2 : n_bins) / (hi - lo);     // edges are finite and increasing (the caller's contract)
    const double lo_g = n_bins > 2 ? lo : lo + (hi - lo) / n_bins;                    // so that floor(t) + 1 is the guess in both layouts
    const double e_first = E[0], e_last = E[n_bins];
    const float* xs = x + (size_t)s * (size_t)n;
    const bool vec = (((uintptr_t)xs) & 15u) == 0;
    const int64_t nchunk = (n + HIST_CHUNK - 1) / HIST_CHUNK;
    int cur = -1;
    uint32_t run = 0;
    auto count = [&](float v) {
        const int b = hist_bin(v, E, n_bins, e_first, e_last, lo_g, inv_w);
        if (FOLD) {
            if (b == cur) { ++run; return; }
            if (cur >= 0) __hip_atomic_fetch_add(&H[cur], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            cur = b;
            run = 1;
        } else if (b >= 0) {
            __hip_atomic_fetch_add(&H[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t base = c * HIST_CHUNK;
        if (vec && base + HIST_CHUNK <= n) {
            f32x4 v[HIST_VEC];
#pragma unroll
            for (int k = 0; k < HIST_VEC; ++k) v[k] = nd_ld4(xs + base + (int64_t)(k * HIST_THREADS + t) * 4);
#pragma unroll
            for (int k = 0; k < HIST_VEC; ++k) {
                count(v[k][0]);  count(v[k][1]);  count(v[k][2]);  count(v[k][3]);
            }
        } else {                                                  // a set off 16 bytes, or the last chunk of a set
            for (int k = 0; k < HIST_VEC; ++k) {
                const int64_t i = base + (int64_t)(k * HIST_THREADS + t) * 4;
                if (vec && i + 4 <= n) {
                    const f32x4 v = nd_ld4(xs + i);
                    count(v[0]);  count(v[1]);  count(v[2]);  count(v[3]);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (i + e < n) count(xs[i + e]);
                }
            }
        }
    }
    if (FOLD && cur >= 0) __hip_atomic_fetch_add(&H[cur], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    uint32_t* o = part + ((size_t)s * gridDim.x + blockIdx.x) * (size_t)n_bins;
    for (int i = t; i < n_bins; i += HIST_THREADS) {
        uint32_t a = Hs[i];
        if (COPIES > 1) a += Hs[n_bins + i] + Hs[2 * n_bins + i] + Hs[3 * n_bins + i];
        o[i] = a;
    }
}

// One workgroup per (set, 16 bins): thread (slice, bin) sums the partials of workgroups slice, slice + 16, ... of its bin (independent loads: a
// set of 25 M elements has 1024 partials), then the 16 slices of a bin are added in slice order.  Integer sums: any order gives the same counts.
constexpr int HIST_FIN_BINS = 16;
__global__ __launch_bounds__(HIST_THREADS) void histogram_finalize_kernel(const uint32_t* __restrict__ part, int nblk, int n_bins,
                                                                          int64_t* __restrict__ counts) {
    __shared__ int64_t red[HIST_THREADS / HIST_FIN_BINS][HIST_FIN_BINS];
    const int bl = threadIdx.x % HIST_FIN_BINS, sl = threadIdx.x / HIST_FIN_BINS;
    const int i = blockIdx.x * HIST_FIN_BINS + bl, s = blockIdx.y;
    int64_t a = 0;
    if (i < n_bins) {
        const uint32_t* p = part + (size_t)s * nblk * (size_t)n_bins + i;
#pragma unroll 4
        for (int b = sl; b < nblk; b += HIST_THREADS / HIST_FIN_BINS) a += (int64_t)p[(size_t)b * n_bins];
    }
    red[sl][bl] = a;
    __syncthreads();
    if (sl == 0 && i < n_bins) {
#pragma unroll
        for (int k = 1; k < HIST_THREADS / HIST_FIN_BINS; ++k) a += red[k][bl];
        counts[(size_t)s * n_bins + i] = a;
    }
}

int hist_blocks(int64_t n) {
    const int64_t nchunk = (n + HIST_CHUNK - 1) / HIST_CHUNK, want = (nchunk + HIST_TRIPS - 1) / HIST_TRIPS;
    return (int)(want < HIST_MAX_BLOCKS ? want : HIST_MAX_BLOCKS);
}
bool hist_sizes_ok(int S, int64_t n) { return S > 0 && S <= 65535 && n > 0 && n <= HIST_MAX_N; }

__device__ __forceinline__ bool ns_finite(double v) { return v - v == 0.0; }

// One workgroup per set.  COUNTS: p and q are int64 counts divided by n_p, n_q; else fp64 hists, whose NaN and inf entries drop the bin as
// kl_div_forward's first mask does.
template <bool COUNTS>
__global__ __launch_bounds__(256) void kl_div_kernel(const void* __restrict__ pv, const void* __restrict__ qv, double n_p, double n_q, int n_bins,
                                                     int q_sets, double* __restrict__ out) {
    __shared__ double red[2][4];
    const int s = blockIdx.x;
    const size_t po = (size_t)s * n_bins, qo = q_sets == 1 ? (size_t)0 : (size_t)s * n_bins;
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n_bins; i += 256) {
        double p, q;
        if (COUNTS) {
            p = (double)static_cast<const int64_t*>(pv)[po + i] / n_p;
            q = (double)static_cast<const int64_t*>(qv)[qo + i] / n_q;
        } else {
            p = static_cast<const double*>(pv)[po + i];
            q = static_cast<const double*>(qv)[qo + i];
        }
        if (ns_finite(p) && ns_finite(q) && p > 0.0 && q > 0.0) {
            acc[0] += p * log(p / q);
            acc[1] += q * log(q / p);
        }
    }
    block_sum_all<2>(acc, red);
    if (threadIdx.x == 0) {
        out[3 * (size_t)s] = acc[0];
        out[3 * (size_t)s + 1] = acc[1];
        out[3 * (size_t)s + 2] = (acc[1] + acc[0]) / 2.0;
    }
}

constexpr int PS_W = 64;                   // output columns of a tile: one per lane of a wave
constexpr int PS_H = 16;                   // output rows of a tile: four per thread
constexpr int PS_LW = PS_W + 2;            // the staged tile with its halo

// One (image, channel, PS_H x PS_W tile) per workgroup: the tile and its one-pixel halo are staged in LDS with zeros outside the image, each
// thread forms mean and std of four windows in fp32 from the nine values (two passes) and adds its fp32 (m, s) to four fp64 sums.
__global__ __launch_bounds__(256) void patch_std_mean_kernel(const float* __restrict__ x, float* __restrict__ std_out, float* __restrict__ mean_out,
                                                             double* __restrict__ slots, int C, int H, int W, int ntx, int nty) {
    __shared__ float tile[PS_H + 2][PS_LW];
    __shared__ double red[4][4];
    const int tl = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tx = tl % ntx, ty = tl / ntx, x0 = tx * PS_W, y0 = ty * PS_H;
    const size_t plane = ((size_t)b * C + c) * (size_t)H * W;
    const float* xp = x + plane;
    for (int i = threadIdx.x; i < (PS_H + 2) * PS_LW; i += 256) {
        const int r = i / PS_LW, q = i - r * PS_LW, yy = y0 - 1 + r, xx = x0 - 1 + q;
        tile[r][q] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? xp[(size_t)yy * W + xx] : 0.0f;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6, px = x0 + lx;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};        // sum m, sum s, sum m m, sum m s
#pragma unroll
    for (int k = 0; k < PS_H / 4; ++k) {
        const int r = ly + 4 * k, py = y0 + r;
        if (px < W && py < H) {
            float v[9];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) v[3 * dy + dx] = tile[r + dy][lx + dx];
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; ++j) sum += v[j];
            const float m = sum / 9.0f;
            float ss = 0.0f;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const float d = v[j] - m;
                ss = fmaf(d, d, ss);
            }
            const float sd = sqrtf(ss / 8.0f);
            const size_t o = plane + (size_t)py * W + px;
            if (mean_out) mean_out[o] = m;
            if (std_out) std_out[o] = sd;
            const double md = m, sdd = sd;
            acc[0] += md;
            acc[1] += sdd;
            acc[2] = fma(md, md, acc[2]);
            acc[3] = fma(md, sdd, acc[3]);
        }
    }
    block_sum_all<4>(acc, red);
    if (threadIdx.x == 0) {
        double* o = slots + (((size_t)b * C + c) * (size_t)(ntx * nty) + tl) * 4;
        o[0] = acc[0];  o[1] = acc[1];  o[2] = acc[2];  o[3] = acc[3];
    }
}

// One workgroup per (image, channel): its tiles' sums thread-strided, then in block_sum_all's tree; the closed-form line.
__global__ __launch_bounds__(256) void patch_fit_kernel(const double* __restrict__ slots, int ntile, double N, double* __restrict__ fit) {
    __shared__ double red[4][4];
    const int bc = blockIdx.x;
    const double* s = slots + (size_t)bc * ntile * 4;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < ntile; i += 256) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += s[4 * (size_t)i + k];
    }
    block_sum_all<4>(a, red);
    if (threadIdx.x == 0) {
        const double sm = a[0], ss = a[1], smm = a[2], sms = a[3];
        const double den = N * smm - sm * sm;
        const double nan = __builtin_nan("");
        const double slope = den == 0.0 ? nan : (N * sms - sm * ss) / den;
        double* o = fit + (size_t)bc * 7;
        o[0] = N;  o[1] = sm;  o[2] = ss;  o[3] = smm;  o[4] = sms;
        o[5] = slope;
        o[6] = (ss - slope * sm) / N;
    }
}

bool ps_sizes_ok(int B, int C, int H, int W) { return B > 0 && C > 0 && H > 0 && W > 0 && B <= 65535 && C <= 65535 && (int64_t)B * C < (1ll << 31); }

}  // namespace

extern "C" int nd_histogram_chunk_elements(void) { return HIST_CHUNK; }

extern "C" int64_t nd_histogram_workspace_bytes(int S, int64_t n, int n_bins) {
    ND_REQUIRE(hist_sizes_ok(S, n), ND_E_BADARG, "nd_histogram_workspace_bytes: S (<= 65535) and n (<= 2^40) must be positive");
    ND_REQUIRE(n_bins >= 1 && n_bins <= HIST_MAX_BINS, ND_E_SHAPE, "nd_histogram_workspace_bytes: n_bins=%d must be in [1, %d]", n_bins, HIST_MAX_BINS);
    return (int64_t)S * hist_blocks(n) * n_bins * (int64_t)sizeof(uint32_t);
}

extern "C" int nd_histogram_f32(const float* x, int S, int64_t n, const double* edges, int n_edges, int64_t* counts, void* workspace, void* stream) {
    ND_REQUIRE(x && edges && counts && workspace, ND_E_BADARG, "nd_histogram_f32: null pointer");
    ND_REQUIRE(hist_sizes_ok(S, n), ND_E_BADARG, "nd_histogram_f32: S (<= 65535) and n (<= 2^40) must be positive");
    const int n_bins = n_edges - 1;
    ND_REQUIRE(n_bins >= 1 && n_bins <= HIST_MAX_BINS, ND_E_SHAPE, "nd_histogram_f32: n_bins=%d (n_edges - 1) must be in [1, %d]", n_bins, HIST_MAX_BINS);
    ND_REQUIRE(((uintptr_t)edges & 7u) == 0 && ((uintptr_t)counts & 7u) == 0, ND_E_BADARG, "nd_histogram_f32: edges and counts must be 8-byte aligned");
    ND_REQUIRE(((uintptr_t)x & 3u) == 0 && ((uintptr_t)workspace & 3u) == 0, ND_E_BADARG, "nd_histogram_f32: x and workspace must be 4-byte aligned");
    const int nblk = hist_blocks(n);
    uint32_t* part = (uint32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk, (unsigned)S);
    constexpr int copies = ND_HIST_VARIANT == 1 ? 4 : 1;
    const bool waves = copies > 1 && n_bins <= HIST_WAVE_BINS;
    const size_t lds = (size_t)(n_bins + 1) * 8 + (size_t)(waves ? copies : 1) * n_bins * 4;          // 48.01 KB at most: under the 64 KB a launch may ask for
    if (waves) hipLaunchKernelGGL((histogram_partial_kernel<copies, false>), grid, dim3(HIST_THREADS), lds, st, x, n, edges, n_bins, part);
    else hipLaunchKernelGGL((histogram_partial_kernel<1, ND_HIST_VARIANT == 2>), grid, dim3(HIST_THREADS), lds, st, x, n, edges, n_bins, part);
    int e = nd_launch_status("nd_histogram_f32 (partials)");
    if (e) return e;
    hipLaunchKernelGGL(histogram_finalize_kernel, dim3((unsigned)nd_cdiv(n_bins, HIST_FIN_BINS), (unsigned)S), dim3(HIST_THREADS), 0, st, part, nblk,
                       n_bins, counts);
    return nd_launch_status("nd_histogram_f32 (finalize)");
}

static int kl_check(const char* who, const void* p, const void* q, int n_bins, int S, int q_sets, const double* out) {
    ND_REQUIRE(p && q && out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE(S > 0 && n_bins >= 1, ND_E_BADARG, "%s: S=%d and n_bins=%d must be positive", who, S, n_bins);
    ND_REQUIRE(q_sets == 1 || q_sets == S, ND_E_BADARG, "%s: q_sets=%d must be 1 or S=%d", who, q_sets, S);
    ND_REQUIRE(((uintptr_t)p & 7u) == 0 && ((uintptr_t)q & 7u) == 0 && ((uintptr_t)out & 7u) == 0, ND_E_BADARG, "%s: pointers must be 8-byte aligned", who);
    return 0;
}

extern "C" int nd_kl_div_f64(const int64_t* p_counts, const int64_t* q_counts, int64_t n_p, int64_t n_q, int n_bins, int S, int q_sets, double* out,
                             void* stream) {
    int e = kl_check("nd_kl_div_f64", p_counts, q_counts, n_bins, S, q_sets, out);
    if (e) return e;
    ND_REQUIRE(n_p > 0 && n_q > 0, ND_E_BADARG, "nd_kl_div_f64: n_p and n_q must be positive");
    hipLaunchKernelGGL(kl_div_kernel<true>, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, (const void*)p_counts, (const void*)q_counts,
                       (double)n_p, (double)n_q, n_bins, q_sets, out);
    return nd_launch_status("nd_kl_div_f64");
}

extern "C" int nd_kl_div_hist_f64(const double* p, const double* q, int n_bins, int S, int q_sets, double* out, void* stream) {
    int e = kl_check("nd_kl_div_hist_f64", p, q, n_bins, S, q_sets, out);
    if (e) return e;
    hipLaunchKernelGGL(kl_div_kernel<false>, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, (const void*)p, (const void*)q, 1.0, 1.0, n_bins,
                       q_sets, out);
    return nd_launch_status("nd_kl_div_hist_f64");
}

extern "C" int64_t nd_patch_std_mean_workspace_bytes(int B, int C, int H, int W) {
    ND_REQUIRE(ps_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_patch_std_mean_workspace_bytes: sizes must be positive (B, C <= 65535)");
    return (int64_t)B * C * nd_cdiv(H, PS_H) * nd_cdiv(W, PS_W) * 4 * (int64_t)sizeof(double);
}

extern "C" int nd_patch_std_mean_f32(const float* x, float* std, float* mean, double* fit, void* workspace, int B, int C, int H, int W, void* stream) {
    ND_REQUIRE(x && fit && workspace, ND_E_BADARG, "nd_patch_std_mean_f32: null pointer (only std and mean may be NULL)");
    ND_REQUIRE(ps_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_patch_std_mean_f32: sizes must be positive (B, C <= 65535)");
    ND_REQUIRE(((uintptr_t)fit & 7u) == 0 && ((uintptr_t)workspace & 7u) == 0, ND_E_BADARG, "nd_patch_std_mean_f32: fit and workspace must be 8-byte aligned");
    const int ntx = nd_cdiv(W, PS_W), nty = nd_cdiv(H, PS_H);
    ND_REQUIRE((int64_t)ntx * nty < (1ll << 31), ND_E_SHAPE, "nd_patch_std_mean_f32: image too large");
    hipStream_t st = (hipStream_t)stream;
    double* slots = (double*)workspace;
    hipLaunchKernelGGL(patch_std_mean_kernel, dim3((unsigned)(ntx * nty), (unsigned)C, (unsigned)B), dim3(256), 0, st, x, std, mean, slots, C, H, W, ntx,
                       nty);
    int e = nd_launch_status("nd_patch_std_mean_f32 (tiles)");
    if (e) return e;
    hipLaunchKernelGGL(patch_fit_kernel, dim3((unsigned)(B * C)), dim3(256), 0, st, slots, ntx * nty, (double)H * (double)W, fit);
    return nd_launch_status("nd_patch_std_mean_f32 (finalize)");
}
