// calibrate.hip -- the physics-based noise model's parameters from dark frames: what ELD / PMN get on the host from row means,
// scipy.stats.ppcc_max and scipy.stats.probplot, on uint16 frames that stay on the device.  The contract is in include/noisediff_hip.h.
//
//   stack      T[y][x] = sum over frames of the code: int32, exact
//   rows       t = D code - P per pixel (an integer); R[n][c][Y] = sum_X t: int64, exact.  One wave per (frame, packed row)
//   residual   x = (double)(t w - R) / (double)(w D): one correctly rounded division per pixel
//   row stats  the ddof-0 variance of the 4 h row means about their channel's mean, exactly in 128 bits, one conversion
//   ppcc       for sorted x: the sums that give Pearson's r, the slope and the intercept of x on the theoretical quantiles of the
//              order-statistic medians; a partial per workgroup in its workspace slot, the slots summed in slot order (the pattern of
//              noise_level.hip's Theil-Sen fit), and Brent's bounded minimisation of 1 - r(lam) stepped by one thread per frame
//
// No floating-point atomics, no cooperative launch, no kernel that waits for another workgroup, no host read.  The frame is a grid
// dimension and the grid per frame is a constant: a frame's bits do not depend on the stack around it.
#include "nd_common.h"
#include "block_sum.h"
#include "u128.h"
#include <math.h>

// Every fp64 operation is one IEEE operation in the written order, so that numpy repeats the exact quantities bit for bit.
#pragma clang fp contract(off)

#include "raw_codes.h"

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int CA_THREADS = 256;
constexpr int CA_MAX_SIDE = 32768;                         // packed rows and columns: within it h sum R^2 fits 128 bits and t w - R 53
constexpr int CA_MAX_FRAMES = 32767;                       // 32767 * 65535 < 2^31

struct CalArgs {
    const uint16_t* frames;
    const int32_t* T;                   // the stack's sums, or null
    const int64_t* R_in;
    int64_t* R;
    double* x;
    int N, h, w;
    int D, P;                           // t = D code - P; P is read from T where there is one
};

// t of the four channels of V packed columns from X on, row Y of frame n
template <int V, bool MEAN>
__device__ __forceinline__ void ca_values(const CalArgs& A, int n, int Y, int X, int64_t (&t)[4][V]) {
    const size_t W2 = 2 * (size_t)A.w;
    const size_t cell = (2 * (size_t)Y) * W2 + 2 * (size_t)X;                  // the cell's top-left code within a frame
    const uint16_t* src = A.frames + (size_t)n * (2 * (size_t)A.h) * W2 + cell;
    uint32_t top[V], bottom[V];
    rw_load_pairs<V>(src, top);
    rw_load_pairs<V>(src + W2, bottom);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int64_t p0 = A.P, p1 = A.P, p2 = A.P, p3 = A.P;
        if constexpr (MEAN) {
            const int2 pt = *reinterpret_cast<const int2*>(A.T + cell + 2 * i);
            const int2 pb = *reinterpret_cast<const int2*>(A.T + cell + W2 + 2 * i);
            p0 = pt.x;  p1 = pt.y;  p2 = pb.y;  p3 = pb.x;
        }
        const int64_t D = A.D;
        t[0][i] = D * (int64_t)(top[i] & 0xFFFFu) - p0;                        // the channel order of rw_code
        t[1][i] = D * (int64_t)(top[i] >> 16) - p1;
        t[2][i] = D * (int64_t)(bottom[i] >> 16) - p2;
        t[3][i] = D * (int64_t)(bottom[i] & 0xFFFFu) - p3;
    }
}

// One code pair per thread: both codes of a 4-byte word of every frame.
__global__ __launch_bounds__(CA_THREADS) void ca_stack_kernel(const uint16_t* __restrict__ frames, int N, int64_t pairs, int32_t* __restrict__ sums) {
    const int64_t p = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x;
    if (p >= pairs) return;
    int2 s = *reinterpret_cast<const int2*>(sums + 2 * p);
    for (int n = 0; n < N; ++n) {
        const uint32_t wd = *reinterpret_cast<const uint32_t*>(frames + 2 * ((int64_t)n * pairs + p));
        s.x += (int)(wd & 0xFFFFu);
        s.y += (int)(wd >> 16);
    }
    *reinterpret_cast<int2*>(sums + 2 * p) = s;
}

__global__ __launch_bounds__(CA_THREADS) void ca_mean_kernel(const int32_t* __restrict__ sums, int64_t count_px, int count, double* __restrict__ mean) {
    const int64_t i = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x;
    if (i < count_px) mean[i] = (double)sums[i] / (double)count;
}

// Wave k of workgroup b takes row unit u = 4 b + k = n h + Y: the four channels' sums over the row, lane-strided groups of V columns.
template <int V, bool MEAN>
__global__ __launch_bounds__(CA_THREADS) void ca_row_kernel(CalArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * (CA_THREADS / 64) + (threadIdx.x >> 6);
    if (u >= (int64_t)A.N * A.h) return;                                       // the whole wave leaves
    const int n = (int)(u / A.h), Y = (int)(u - (int64_t)n * A.h);
    long long s[4] = {0, 0, 0, 0};
    const int groups = A.w / V;
    for (int g = lane; g < groups; g += 64) {
        int64_t t[4][V];
        ca_values<V, MEAN>(A, n, Y, g * V, t);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < V; ++i) s[c] += t[c][i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += __shfl_xor(s[c], o);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) A.R[((int64_t)n * 4 + c) * A.h + Y] = s[c];
}

// Thread i of block row blockIdx.y = frame n takes packed columns V (i mod (w / V)) .. + V - 1 of row i / (w / V), all four channels.
template <int V, bool MEAN>
__global__ __launch_bounds__(CA_THREADS) void ca_residual_kernel(CalArgs A) {
    const int n = blockIdx.y;
    const int h = A.h, w = A.w, wv = w / V;
    const int64_t i = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x;
    if (i >= (int64_t)h * wv) return;
    const int Y = (int)(i / wv), X = (int)(i - (int64_t)Y * wv) * V;
    int64_t t[4][V];
    ca_values<V, MEAN>(A, n, Y, X, t);
    const int64_t wl = w;
    const double den = (double)(wl * A.D);                                     // below 2^30: exact
    const size_t plane = (size_t)h * w;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t Rc = A.R_in[((int64_t)n * 4 + c) * h + Y];
        double v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = (double)(t[c][k] * wl - Rc) / den;  // |t w - R| < 2^53: the conversion is exact
        double* dst = A.x + ((size_t)n * 4 + c) * plane + (size_t)Y * w + X;   // 8 V-byte aligned up to 16: w is a multiple of V
        if constexpr (V == 1) {
            dst[0] = v[0];
        } else {
#pragma unroll
            for (int k = 0; k < V; k += 2) *reinterpret_cast<double2*>(dst + k) = double2{v[k], v[k + 1]};
        }
    }
}

// One workgroup per frame.  Integer sums: their order does not matter.
__global__ __launch_bounds__(CA_THREADS) void ca_row_stats_kernel(const int64_t* __restrict__ R, int h, int w, int D, const double* __restrict__ var_x,
                                                                   int var_stride, double* __restrict__ out) {
    __shared__ long long lds_s[4][4];
    __shared__ u64 lds_q[4][4][2];
    const int n = blockIdx.x, t = threadIdx.x, wave = t >> 6;
    long long S[4];
    u64 lo[4], hi[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        long long s = 0;
        u128 q = 0;
        for (int Y = t; Y < h; Y += CA_THREADS) {
            const long long r = R[((int64_t)n * 4 + c) * h + Y];
            const u64 a = (u64)(r < 0 ? -r : r);
            s += r;
            q += (u128)a * a;
        }
        S[c] = s;
        lo[c] = (u64)q;
        hi[c] = (u64)(q >> 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            S[c] += __shfl_xor(S[c], o);
            const u64 olo = __shfl_xor(lo[c], o), ohi = __shfl_xor(hi[c], o);
            lo[c] += olo;
            hi[c] += ohi + (u64)(lo[c] < olo);
        }
    if ((t & 63) == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lds_s[c][wave] = S[c];
            lds_q[c][wave][0] = lo[c];
            lds_q[c][wave][1] = hi[c];
        }
    __syncthreads();
    if (t != 0) return;
    double* o = out + (size_t)n * 8;
    const double wd = (double)((int64_t)w * D);
    u128 total = 0;
    for (int c = 0; c < 4; ++c) {
        long long s = 0;
        u128 q = 0;
        for (int k = 0; k < 4; ++k) {
            s += lds_s[c][k];
            q += ((u128)lds_q[c][k][1] << 64) | (u128)lds_q[c][k][0];
        }
        const u64 a = (u64)(s < 0 ? -s : s);
        total += (u128)(u64)h * q - (u128)a * a;                               // >= 0 (Cauchy-Schwarz); the four of them below 2^124
        o[2 + c] = (double)s / (double)((int64_t)h * w * D);
    }
    const double v = nd_u128_to_double(total) / (double)(4ll * h * h) / wd / wd;
    const double vx = var_x[(size_t)n * var_stride];
    const double d = v - vx / (double)(w - 1);
    o[0] = sqrt(v);
    o[1] = sqrt(d < 0.0 ? 0.0 : d);                                            // a NaN passes
    o[6] = vx;
    o[7] = 0.0;
}

// ------------------------------------------------------------------ probability plots

constexpr int PP_THREADS = 256;
constexpr int PP_BLOCKS = 1024;                            // slots per frame, a constant: the order of every sum is a function of (xs, n, lam)
constexpr int PP_SUMS = 5;
constexpr int PP_MAX_EVAL = 64;
constexpr int PP_GAUSS = 0, PP_TUKEY = 1;

struct pp_state {                                          // one frame's search: scipy's _minimize_scalar_bounded, its names
    double a, b, fulc, nfc, xf, rat, e, x, fx, ffulc, fnfc, xatol;
    int num, done, max_eval, reserved;
};
constexpr int PP_STATE_DOUBLES = sizeof(pp_state) / sizeof(double);
static_assert(sizeof(pp_state) % sizeof(double) == 0, "the slots follow the states as doubles");

__device__ __forceinline__ double pp_tukey(double u, double lam) {             // physics_noise.hip's pn_tukey
    const double a = log(u);
    const double b = log1p(-u);
    if (lam == 0.0) return a - b;
    const double p = lam * a;
    const double q = lam * b;
    const double ep = expm1(p);
    const double eq = expm1(q);
    const double d = ep - eq;
    return d / lam;
}

__device__ __forceinline__ double pp_median(int64_t i, int64_t n, double m_last, double den) {
    if (i == n - 1) return m_last;
    if (i == 0) return 1.0 - m_last;
    return ((double)(i + 1) - 0.3175) / den;
}

template <int KIND>
__device__ __forceinline__ double pp_quantile(double m, double lam) {
    return KIND == PP_TUKEY ? pp_tukey(m, lam) : normcdfinv(m);
}

template <int KIND>
__global__ __launch_bounds__(PP_THREADS) void pp_quantile_kernel(int64_t n, double m_last, double lam, double* __restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (i < n) q[i] = pp_quantile<KIND>(pp_median(i, n, m_last, (double)n + 0.365), lam);
}

// Workgroup (b, f): elements b 256 + t, + 262144, ... of frame f.  lam and done are read at a stride: the search keeps them in its states.
template <int KIND>
__global__ __launch_bounds__(PP_THREADS) void pp_partial_kernel(const double* __restrict__ xs, int64_t n, double m_last, const double* __restrict__ lam,
                                                                int lam_stride, const int* __restrict__ done, int done_stride,
                                                                double* __restrict__ slots) {
    const int f = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    if (done && done[(size_t)f * done_stride]) return;
    __shared__ double red[PP_SUMS][4];
    const double* x = xs + (size_t)f * n;
    const double centre = x[n / 2];
    const double l = KIND == PP_TUKEY ? lam[(size_t)f * lam_stride] : 0.0;
    const double den = (double)n + 0.365;
    double acc[PP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)b * PP_THREADS + t; i < n; i += (int64_t)PP_BLOCKS * PP_THREADS) {
        const double q = pp_quantile<KIND>(pp_median(i, n, m_last, den), l);
        const double xc = x[i] - centre;
        acc[0] += xc;
        acc[1] += q;
        acc[2] += xc * xc;
        acc[3] += q * q;
        acc[4] += xc * q;
    }
    block_sum_all<PP_SUMS>(acc, red);
    if (t == 0) {
        double* s = slots + ((size_t)f * PP_BLOCKS + b) * PP_SUMS;
#pragma unroll
        for (int k = 0; k < PP_SUMS; ++k) s[k] = acc[k];
    }
}

struct pp_fit {
    double slope, icpt, r, mean, var;
};

// The slots of frame f in slot order (thread t takes t, t + 256, ..., then the tree); every thread gets the fit.
__device__ __forceinline__ pp_fit pp_finalize(const double* __restrict__ slots, int f, const double* __restrict__ xs, int64_t n, double (*red)[4]) {
    double S[PP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < PP_BLOCKS; b += PP_THREADS) {
        const double* s = slots + ((size_t)f * PP_BLOCKS + b) * PP_SUMS;
#pragma unroll
        for (int k = 0; k < PP_SUMS; ++k) S[k] += s[k];
    }
    block_sum_all<PP_SUMS>(S, red);
    const double nn = (double)n;
    const double cxx = S[2] - S[0] * S[0] / nn, cqq = S[3] - S[1] * S[1] / nn, cxq = S[4] - S[0] * S[1] / nn;
    pp_fit fit;
    fit.slope = cxq / cqq;
    fit.mean = xs[(size_t)f * n + n / 2] + S[0] / nn;
    fit.icpt = fit.mean - fit.slope * (S[1] / nn);
    const double r = cxq / (sqrt(cxx) * sqrt(cqq));
    fit.r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                             // a NaN passes
    fit.var = cxx / nn;
    return fit;
}

__global__ __launch_bounds__(PP_THREADS) void pp_plot_kernel(const double* __restrict__ xs, int64_t n, const double* __restrict__ slots,
                                                             double* __restrict__ out) {
    __shared__ double red[PP_SUMS][4];
    const int f = blockIdx.x;
    const pp_fit fit = pp_finalize(slots, f, xs, n, red);
    if (threadIdx.x != 0) return;
    double* o = out + (size_t)f * 6;
    o[0] = fit.slope;
    o[1] = fit.icpt;
    o[2] = fit.r;
    o[3] = fit.mean;
    o[4] = fit.var;
    o[5] = 0.0;
}

__global__ __launch_bounds__(PP_THREADS) void pp_init_kernel(pp_state* __restrict__ st, int N, double lo, double hi, double xatol, int max_eval) {
    const int f = blockIdx.x * PP_THREADS + threadIdx.x;
    if (f >= N) return;
    const double golden_mean = 0.5 * (3.0 - sqrt(5.0));
    pp_state s;
    s.a = lo;
    s.b = hi;
    s.fulc = s.a + golden_mean * (s.b - s.a);
    s.nfc = s.xf = s.x = s.fulc;
    s.rat = s.e = 0.0;
    s.fx = s.ffulc = s.fnfc = 0.0;
    s.xatol = xatol;
    s.num = 0;
    s.done = 0;
    s.max_eval = max_eval;
    s.reserved = 0;
    st[f] = s;
}

// One workgroup per frame: the objective at the state's x from the slots, then thread 0 runs the body of scipy's loop from the evaluation on
// and its head up to the next evaluation.
__global__ __launch_bounds__(PP_THREADS) void pp_step_kernel(const double* __restrict__ xs, int64_t n, pp_state* __restrict__ states,
                                                             const double* __restrict__ slots, double* __restrict__ out) {
    __shared__ double red[PP_SUMS][4];
    const int f = blockIdx.x;
    if (states[f].done) return;
    const pp_fit fit = pp_finalize(slots, f, xs, n, red);
    if (threadIdx.x != 0) return;
    pp_state s = states[f];
    double* o = out + (size_t)f * 3;
    const double fu = 1.0 - fit.r;
    const double x = s.x;
    s.num += 1;
    o[2] = (double)s.num;
    if (!(fu == fu)) {                                                         // a constant frame: no correlation to maximise
        s.done = 1;
        o[0] = o[1] = __builtin_nan("");
        states[f] = s;
        return;
    }
    if (s.num == 1) {
        s.fx = s.ffulc = s.fnfc = fu;
    } else if (fu <= s.fx) {
        if (x >= s.xf) s.a = s.xf;
        else s.b = s.xf;
        s.fulc = s.nfc;  s.ffulc = s.fnfc;
        s.nfc = s.xf;  s.fnfc = s.fx;
        s.xf = x;  s.fx = fu;
    } else {
        if (x < s.xf) s.a = x;
        else s.b = x;
        if (fu <= s.fnfc || s.nfc == s.xf) {
            s.fulc = s.nfc;  s.ffulc = s.fnfc;
            s.nfc = x;  s.fnfc = fu;
        } else if (fu <= s.ffulc || s.fulc == s.xf || s.fulc == s.nfc) {
            s.fulc = x;  s.ffulc = fu;
        }
    }
    const double sqrt_eps = sqrt(2.2e-16), golden_mean = 0.5 * (3.0 - sqrt(5.0));
    const double xm = 0.5 * (s.a + s.b);
    const double tol1 = sqrt_eps * fabs(s.xf) + s.xatol / 3.0;
    const double tol2 = 2.0 * tol1;
    o[0] = s.xf;
    o[1] = 1.0 - s.fx;
    if ((s.num > 1 && s.num >= s.max_eval) || !(fabs(s.xf - xm) > tol2 - 0.5 * (s.b - s.a))) {
        s.done = 1;
        states[f] = s;
        return;
    }
    bool golden = true;
    if (fabs(s.e) > tol1) {                                                    // a parabola through xf, nfc, fulc
        golden = false;
        double r = (s.xf - s.nfc) * (s.fx - s.ffulc);
        double q = (s.xf - s.fulc) * (s.fx - s.fnfc);
        double p = (s.xf - s.fulc) * q - (s.xf - s.nfc) * r;
        q = 2.0 * (q - r);
        if (q > 0.0) p = -p;
        q = fabs(q);
        r = s.e;
        s.e = s.rat;
        if (fabs(p) < fabs(0.5 * q * r) && p > q * (s.a - s.xf) && p < q * (s.b - s.xf)) {
            s.rat = (p + 0.0) / q;
            const double xn = s.xf + s.rat;
            if ((xn - s.a) < tol2 || (s.b - xn) < tol2) {
                const double d = xm - s.xf;
                s.rat = tol1 * (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 1.0));
            }
        } else {
            golden = true;
        }
    }
    if (golden) {
        s.e = s.xf >= xm ? s.a - s.xf : s.b - s.xf;
        s.rat = golden_mean * s.e;
    }
    const double si = s.rat > 0.0 ? 1.0 : (s.rat < 0.0 ? -1.0 : 1.0);
    s.x = s.xf + si * fmax(fabs(s.rat), tol1);
    states[f] = s;
}

bool ca_shape_ok(int N, int H2, int W2) {
    return N >= 1 && N <= CA_MAX_FRAMES && H2 >= 4 && W2 >= 4 && H2 % 2 == 0 && W2 % 2 == 0 && H2 / 2 <= CA_MAX_SIDE && W2 / 2 <= CA_MAX_SIDE;
}

double pp_m_last(int64_t n) { return pow(0.5, 1.0 / (double)n); }

template <int KIND>
void pp_launch_partial(hipStream_t st, const double* xs, int N, int64_t n, const double* lam, int lam_stride, const int* done, int done_stride,
                       double* slots) {
    hipLaunchKernelGGL(pp_partial_kernel<KIND>, dim3(PP_BLOCKS, (unsigned)N), dim3(PP_THREADS), 0, st, xs, n, pp_m_last(n), lam, lam_stride, done,
                       done_stride, slots);
}

int ca_frame_pass(const char* who, bool residual, const uint16_t* frames, int N, int H2, int W2, const int32_t* T, int black, const int64_t* R_in,
                  int64_t* R, double* x, void* stream) {
    ND_REQUIRE(frames && (residual ? (R_in && x) : R != nullptr), ND_E_BADARG, "%s: null pointer (only T may be NULL)", who);
    ND_REQUIRE(ca_shape_ok(N, H2, W2), ND_E_BADARG,
               "%s: need 1 <= N <= %d frames with even sides and 2 <= H2 / 2, W2 / 2 <= %d; got %d x %d x %d", who, CA_MAX_FRAMES, CA_MAX_SIDE, N, H2, W2);
    ND_REQUIRE(black >= 0 && black <= 65535, ND_E_BADARG, "%s: black=%d must be in [0, 65535]", who, black);
    ND_REQUIRE(((uintptr_t)frames & 3u) == 0 && ((uintptr_t)T & 7u) == 0 && (((uintptr_t)R | (uintptr_t)R_in) & 7u) == 0 && ((uintptr_t)x & 15u) == 0,
               ND_E_BADARG, "%s: frames must be 4-byte aligned, T and R 8-byte aligned, x 16-byte aligned", who);
    CalArgs A;
    A.frames = frames;  A.T = T;  A.R_in = R_in;  A.R = R;  A.x = x;
    A.N = N;  A.h = H2 / 2;  A.w = W2 / 2;
    A.D = T ? N : 1;  A.P = black;
    const int V = rw_width(A.w, 0);
    const bool mean = T != nullptr;
    hipStream_t st = (hipStream_t)stream;
    rw_dispatch(V, [&](auto v) {
        constexpr int VV = decltype(v)::value;
        if (residual) {
            const dim3 grid((unsigned)(((int64_t)A.h * (A.w / VV) + CA_THREADS - 1) / CA_THREADS), (unsigned)N);
            if (mean) hipLaunchKernelGGL((ca_residual_kernel<VV, true>), grid, dim3(CA_THREADS), 0, st, A);
            else hipLaunchKernelGGL((ca_residual_kernel<VV, false>), grid, dim3(CA_THREADS), 0, st, A);
        } else {
            const dim3 grid((unsigned)(((int64_t)N * A.h + CA_THREADS / 64 - 1) / (CA_THREADS / 64)));
            if (mean) hipLaunchKernelGGL((ca_row_kernel<VV, true>), grid, dim3(CA_THREADS), 0, st, A);
            else hipLaunchKernelGGL((ca_row_kernel<VV, false>), grid, dim3(CA_THREADS), 0, st, A);
        }
    });
    return nd_launch_status(who);
}

bool pp_shape_ok(int N, int64_t n) { return N >= 1 && N <= CA_MAX_FRAMES && n >= 3 && n <= (1ll << 40); }

}  // namespace

extern "C" int nd_dark_stack_add_u16(const uint16_t* frames, int N, int H2, int W2, int32_t* sums, void* stream) {
    ND_REQUIRE(frames && sums, ND_E_BADARG, "nd_dark_stack_add_u16: null pointer");
    ND_REQUIRE(ca_shape_ok(N, H2, W2), ND_E_BADARG,
               "nd_dark_stack_add_u16: need 1 <= N <= %d frames with even sides and 2 <= H2 / 2, W2 / 2 <= %d; got %d x %d x %d", CA_MAX_FRAMES,
               CA_MAX_SIDE, N, H2, W2);
    ND_REQUIRE(((uintptr_t)frames & 3u) == 0 && ((uintptr_t)sums & 7u) == 0, ND_E_BADARG,
               "nd_dark_stack_add_u16: frames must be 4-byte aligned and sums 8-byte aligned");
    const int64_t pairs = (int64_t)H2 * W2 / 2;
    hipLaunchKernelGGL(ca_stack_kernel, dim3((unsigned)((pairs + CA_THREADS - 1) / CA_THREADS)), dim3(CA_THREADS), 0, (hipStream_t)stream, frames, N, pairs,
                       sums);
    return nd_launch_status("nd_dark_stack_add_u16");
}

extern "C" int nd_dark_stack_mean_f64(const int32_t* sums, int H2, int W2, int count, double* mean, void* stream) {
    ND_REQUIRE(sums && mean, ND_E_BADARG, "nd_dark_stack_mean_f64: null pointer");
    ND_REQUIRE(ca_shape_ok(1, H2, W2) && count >= 1 && count <= CA_MAX_FRAMES, ND_E_BADARG,
               "nd_dark_stack_mean_f64: need even sides with 2 <= H2 / 2, W2 / 2 <= %d and 1 <= count <= %d; got %d x %d, count %d", CA_MAX_SIDE,
               CA_MAX_FRAMES, H2, W2, count);
    ND_REQUIRE(((uintptr_t)sums & 3u) == 0 && ((uintptr_t)mean & 7u) == 0, ND_E_BADARG,
               "nd_dark_stack_mean_f64: sums must be 4-byte aligned and mean 8-byte aligned");
    const int64_t px = (int64_t)H2 * W2;
    hipLaunchKernelGGL(ca_mean_kernel, dim3((unsigned)((px + CA_THREADS - 1) / CA_THREADS)), dim3(CA_THREADS), 0, (hipStream_t)stream, sums, px, count, mean);
    return nd_launch_status("nd_dark_stack_mean_f64");
}

extern "C" int nd_calib_row_sums_i64(const uint16_t* frames, int N, int H2, int W2, const int32_t* T, int black, int64_t* R, void* stream) {
    return ca_frame_pass("nd_calib_row_sums_i64", false, frames, N, H2, W2, T, black, nullptr, R, nullptr, stream);
}

extern "C" int nd_calib_residual_f64(const uint16_t* frames, int N, int H2, int W2, const int32_t* T, int black, const int64_t* R, double* x,
                                     void* stream) {
    return ca_frame_pass("nd_calib_residual_f64", true, frames, N, H2, W2, T, black, R, nullptr, x, stream);
}

extern "C" int nd_calib_row_stats_f64(const int64_t* R, int N, int h, int w, int D, const double* var_x, int var_stride, double* out, void* stream) {
    ND_REQUIRE(R && var_x && out, ND_E_BADARG, "nd_calib_row_stats_f64: null pointer");
    ND_REQUIRE(N >= 1 && N <= CA_MAX_FRAMES && h >= 2 && h <= CA_MAX_SIDE && w >= 2 && w <= CA_MAX_SIDE && D >= 1 && D <= CA_MAX_FRAMES && var_stride >= 1,
               ND_E_BADARG, "nd_calib_row_stats_f64: need 1 <= N, D <= %d, 2 <= h, w <= %d and var_stride >= 1; got N=%d h=%d w=%d D=%d var_stride=%d",
               CA_MAX_FRAMES, CA_MAX_SIDE, N, h, w, D, var_stride);
    ND_REQUIRE((((uintptr_t)R | (uintptr_t)var_x | (uintptr_t)out) & 7u) == 0, ND_E_BADARG, "nd_calib_row_stats_f64: pointers must be 8-byte aligned");
    hipLaunchKernelGGL(ca_row_stats_kernel, dim3((unsigned)N), dim3(CA_THREADS), 0, (hipStream_t)stream, R, h, w, D, var_x, var_stride, out);
    return nd_launch_status("nd_calib_row_stats_f64");
}

extern "C" int nd_calib_quantiles_f64(int64_t n, int kind, double lam, double* q, void* stream) {
    ND_REQUIRE(q && ((uintptr_t)q & 7u) == 0, ND_E_BADARG, "nd_calib_quantiles_f64: q must be given and 8-byte aligned");
    ND_REQUIRE(pp_shape_ok(1, n) && n < (1ll << 39), ND_E_BADARG, "nd_calib_quantiles_f64: n must be in [3, 2^39)");
    ND_REQUIRE(kind == PP_GAUSS || kind == PP_TUKEY, ND_E_BADARG, "nd_calib_quantiles_f64: kind=%d must be 0 (normal) or 1 (Tukey-lambda)", kind);
    const dim3 grid((unsigned)((n + PP_THREADS - 1) / PP_THREADS));
    if (kind == PP_TUKEY) hipLaunchKernelGGL(pp_quantile_kernel<PP_TUKEY>, grid, dim3(PP_THREADS), 0, (hipStream_t)stream, n, pp_m_last(n), lam, q);
    else hipLaunchKernelGGL(pp_quantile_kernel<PP_GAUSS>, grid, dim3(PP_THREADS), 0, (hipStream_t)stream, n, pp_m_last(n), lam, q);
    return nd_launch_status("nd_calib_quantiles_f64");
}

extern "C" int64_t nd_ppcc_workspace_bytes(int N) {
    ND_REQUIRE(N >= 1 && N <= CA_MAX_FRAMES, ND_E_BADARG, "nd_ppcc_workspace_bytes: N=%d must be in [1, %d]", N, CA_MAX_FRAMES);
    return (int64_t)N * (PP_STATE_DOUBLES + PP_BLOCKS * PP_SUMS) * (int64_t)sizeof(double);
}

extern "C" int nd_probplot_f64(const double* xs, int N, int64_t n, int kind, const double* lam, double* out, void* workspace, void* stream) {
    ND_REQUIRE(xs && out && workspace, ND_E_BADARG, "nd_probplot_f64: null pointer");
    ND_REQUIRE(pp_shape_ok(N, n), ND_E_BADARG, "nd_probplot_f64: need 1 <= N <= %d frames of 3 <= n <= 2^40 values", CA_MAX_FRAMES);
    ND_REQUIRE(kind == PP_TUKEY ? lam != nullptr : (kind == PP_GAUSS && lam == nullptr), ND_E_BADARG,
               "nd_probplot_f64: kind 1 (Tukey-lambda) takes lam, kind 0 (normal) takes NULL; got kind %d", kind);
    ND_REQUIRE((((uintptr_t)xs | (uintptr_t)lam | (uintptr_t)out | (uintptr_t)workspace) & 7u) == 0, ND_E_BADARG, "nd_probplot_f64: pointers must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* slots = (double*)workspace + (size_t)N * PP_STATE_DOUBLES;
    if (kind == PP_TUKEY) pp_launch_partial<PP_TUKEY>(st, xs, N, n, lam, 1, nullptr, 0, slots);
    else pp_launch_partial<PP_GAUSS>(st, xs, N, n, nullptr, 0, nullptr, 0, slots);
    hipLaunchKernelGGL(pp_plot_kernel, dim3((unsigned)N), dim3(PP_THREADS), 0, st, xs, n, (const double*)slots, out);
    return nd_launch_status("nd_probplot_f64");
}

extern "C" int nd_ppcc_max_f64(const double* xs, int N, int64_t n, double lo, double hi, double xtol, int max_eval, double* out, void* workspace,
                               void* stream) {
    ND_REQUIRE(xs && out && workspace, ND_E_BADARG, "nd_ppcc_max_f64: null pointer");
    ND_REQUIRE(pp_shape_ok(N, n), ND_E_BADARG, "nd_ppcc_max_f64: need 1 <= N <= %d frames of 3 <= n <= 2^40 values", CA_MAX_FRAMES);
    ND_REQUIRE(lo > -0.5 && lo < hi && hi < 1e6, ND_E_BADARG, "nd_ppcc_max_f64: need -0.5 < lo < hi (the unit variance is infinite at -0.5); got %g, %g", lo, hi);
    ND_REQUIRE(xtol > 0.0 && xtol < 1e6, ND_E_BADARG, "nd_ppcc_max_f64: xtol=%g must be positive", xtol);
    ND_REQUIRE(max_eval >= 3 && max_eval <= PP_MAX_EVAL, ND_E_BADARG, "nd_ppcc_max_f64: max_eval=%d must be in [3, %d]", max_eval, PP_MAX_EVAL);
    ND_REQUIRE((((uintptr_t)xs | (uintptr_t)out | (uintptr_t)workspace) & 7u) == 0, ND_E_BADARG, "nd_ppcc_max_f64: pointers must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    pp_state* states = (pp_state*)workspace;
    double* slots = (double*)workspace + (size_t)N * PP_STATE_DOUBLES;
    hipLaunchKernelGGL(pp_init_kernel, dim3((unsigned)nd_cdiv(N, PP_THREADS)), dim3(PP_THREADS), 0, st, states, N, lo, hi, xtol, max_eval);
    int e = nd_launch_status("nd_ppcc_max_f64 (start)");
    if (e) return e;
    const int stride_d = PP_STATE_DOUBLES, stride_i = (int)(sizeof(pp_state) / sizeof(int));
    for (int it = 0; it < max_eval; ++it) {
        pp_launch_partial<PP_TUKEY>(st, xs, N, n, &states[0].x, stride_d, &states[0].done, stride_i, slots);
        hipLaunchKernelGGL(pp_step_kernel, dim3((unsigned)N), dim3(PP_THREADS), 0, st, xs, n, states, (const double*)slots, out);
    }
    return nd_launch_status("nd_ppcc_max_f64 (steps)");
}
