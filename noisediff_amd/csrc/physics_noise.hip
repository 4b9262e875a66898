// physics_noise.hip -- the calibrated physics-based noise model of ELD / PMN drawn on windows of resident uint16 Bayer frames, one launch:
// Poisson shot noise, Gaussian or Tukey-lambda read noise, row noise, quantisation noise and a bias.  It is the baseline a learned noise
// synthesizer is scored against; the reference ships the model's calibration (utils/raw_util.py get_camera_noisy_params_max :422-452) and uses
// nothing of it but Kmax.
//
// The contract (also in include/noisediff_hip.h).  Units are codes above black at the short exposure (DN);
// wb = white - black in fp32.  Contraction to fma is off for this file: every line below is one IEEE operation (a product and the sum that
// takes it are two), in this order, so numpy repeats it bit for bit from the same variates.
//
// Output element (c, y, x) of sample b, the h x w window at (x0, y0) of frame `frame`: packed row Y = y0 + (flip ? h-1-y : y), column X = x0 + x.
//   c0 = max((float)code - black, 0)                 fp32      (as nd_raw_poisson_gaussian_f32)
//   clean_out = c0 / wb                              fp32
//   latent = c0 / (float)ratio                       fp32
//   lamP = (double)latent / K                        fp64
//   n  ~ Poisson(lamP)                               philox_poisson, counter {e, first_sample + b, draw, blocks 0..31}, e = c h w + y w + x
//   r  = the unit read variate, rounded to fp32      block 32 of the same counter
//        read_kind 0: sqrt(-2 log u0) cos((2 pi) u1) on words 0 and 1 (nd_raw_poisson_gaussian_f32's normal exactly)
//        read_kind 1: the Tukey-lambda quantile of u2 (word 2): a = log u2; b = log1p(-u2);
//                     lam != 0: Q = (expm1(lam a) - expm1(lam b)) / lam;  lam == 0: Q = a - b (the logistic quantile)
//   g  = the unit row variate, rounded to fp32       the same Box-Muller on words 0 and 1 of counter {4 Y + c, row_stream, draw, block 33}:
//        one per (absolute row Y, channel c), keyed by the SOURCE row, so a flipped window carries the row noise with its rows
//   uq = (float)(u3 - 0.5)                           word 3 of block 32
//   t = K n;  t = t + s_read r;  t = t + s_row g;  t = t + qstep uq;  t = t + bias          fp64
//   t = clip(t, -black, wb)                          by comparisons, a NaN passes: the sensor's range at the short exposure
//   v = t ratio;  v = v / wb;                        with ND_PHYS_CLIP01: v = clip(v, 0, 1)
//   noisy = fl32(v);  noise_out = noisy - clean_out  fp32
// Uniforms are u = (word + 0.5) 2^-32 in fp64.  s_read is the SCALE of the unit Tukey-lambda variate (scipy.stats.tukeylambda's scale=, PMN's
// sigTL), not a standard deviation.  The expm1 form, not pow: the calibrated |lam| go down to 0.0026 and pow(u, lam) - 1 cancels there.
//
// Threads as in raw.hip's pack kernel: a thread takes V = 4, 2 or 1 packed columns of one output row for all four channels, reads the cell's
// codes with two loads and derives the four row variates of its row itself (4 Box-Mullers next to 4 V elements).  Grid (tiles, B): the sample is
// the grid's second dimension, so read_kind is uniform per workgroup.  No LDS.  The draws of the 4 V elements run in one rolled loop: the
// Poisson draw, the Box-Muller and the quantile are inlined once.
#include "nd_common.h"

#pragma clang fp contract(off)

#include "philox_poisson.h"
#include "raw_codes.h"

namespace {

constexpr int PN_THREADS = 256;
constexpr uint32_t PN_READ_BLOCK = 32u;            // PO_MAX_ATTEMPTS / 2: the first block the Poisson draw leaves; the block of P-G's normal
constexpr uint32_t PN_ROW_BLOCK = 33u;
static_assert(PN_READ_BLOCK == PO_MAX_ATTEMPTS / 2, "the read variate takes the first block the Poisson draw cannot reach");

struct PhysArgs {
    const uint16_t* frames;
    const nd_physics_sample* table;     // [B]
    const int64_t* rng;                 // {seed, first_sample, draw} or null
    const float* counts_in;  const float* reads_in;  const float* rows_in;  const float* quants_in;
    float* counts_out;  float* reads_out;  float* rows_out;  float* quants_out;
    float* noisy;  float* clean_out;  float* noise_out;
    uint64_t seed;  int64_t first_sample;  int32_t draw;
    int N, H, W, h, w;                  // H, W: the packed frame
    int flags;
    float black, white;
};

template <int V>
__device__ __forceinline__ void pn_store_nan(float* p) {
    float nanv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) nanv[i] = __builtin_nanf("");
    nd_store_v<V>(p, nanv);
}

__device__ __forceinline__ double pn_box_muller(double u0, double u1) {
    const double r = sqrt(-2.0 * log(u0));
    const double a = 6.283185307179586 * u1;
    return r * cos(a);
}

__device__ __forceinline__ double pn_tukey(double u, double lam) {
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

// Thread i of block row blockIdx.y = sample b takes packed columns V (i mod (w / V)) .. + V - 1 of output row i / (w / V), all four channels.
template <int V>
__global__ __launch_bounds__(PN_THREADS) void physics_noise_kernel(PhysArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w, wv = w / V;
    const size_t t = (size_t)blockIdx.x * PN_THREADS + threadIdx.x;
    if (t >= (size_t)h * wv) return;
    const int y = (int)(t / wv), x = (int)(t - (size_t)y * wv) * V;
    const nd_physics_sample s = A.table[b];
    const size_t plane = (size_t)h * w;
    const size_t px = (size_t)y * w + x;
    const size_t o = (size_t)b * 4 * plane + px;
    const size_t orow = (size_t)b * 4 * h + y;                                  // rows_*[b][c][y] is orow + c h; written by the thread of x == 0

    // a table row that points outside the frame is refused here as well as on the host: NaN out, nothing read
    if (!(s.frame >= 0 && s.frame < A.N && s.x0 >= 0 && s.y0 >= 0 && s.x0 <= A.W - w && s.y0 <= A.H - h)) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            pn_store_nan<V>(A.noisy + o + c * plane);
            pn_store_nan<V>(A.clean_out + o + c * plane);
            if (A.noise_out) pn_store_nan<V>(A.noise_out + o + c * plane);
            if (A.counts_out) pn_store_nan<V>(A.counts_out + o + c * plane);
            if (A.reads_out) pn_store_nan<V>(A.reads_out + o + c * plane);
            if (A.quants_out) pn_store_nan<V>(A.quants_out + o + c * plane);
            if (A.rows_out && x == 0) A.rows_out[orow + (size_t)c * h] = __builtin_nanf("");
        }
        return;
    }
    const int Y = s.y0 + (s.flip ? h - 1 - y : y), X = s.x0 + x;
    const size_t W2 = 2 * (size_t)A.W;
    const uint16_t* src = A.frames + ((size_t)s.frame * (2 * (size_t)A.H) + 2 * (size_t)Y) * W2 + 2 * (size_t)X;
    uint32_t top[V], bottom[V];
    rw_load_pairs<V>(src, top);
    rw_load_pairs<V>(src + W2, bottom);

    uint64_t seed = A.seed;
    int64_t first = A.first_sample;
    uint32_t draw = (uint32_t)A.draw;
    if (A.rng) { seed = (uint64_t)A.rng[0];  first = A.rng[1];  draw = (uint32_t)A.rng[2]; }
    const uint32_t sample = (uint32_t)(first + b);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float black = A.black, wb = A.white - black;
    const float ratio32 = (float)s.ratio;
    const double wbd = (double)wb, lo = -(double)black;
    const bool clip01 = (A.flags & ND_PHYS_CLIP01) != 0;

#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        float grow;
        if (A.rows_in) {
            grow = A.rows_in[orow + (size_t)c * h];
        } else {
            uint32_t ctr[4] = {4u * (uint32_t)Y + (uint32_t)c, s.row_stream, draw, PN_ROW_BLOCK};
            Philox::gen(ctr, k0, k1);
            grow = (float)pn_box_muller(po_uniform(ctr[0]), po_uniform(ctr[1]));
        }
        if (A.rows_out && x == 0) A.rows_out[orow + (size_t)c * h] = grow;

        const size_t oc = o + c * plane;
        const uint32_t e0 = (uint32_t)((size_t)c * plane + px);
        float cf[V], clean[V], cnt[V], rd[V], qu[V], noisy[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float g = rw_code(top[i], bottom[i], c) - black;
            cf[i] = g < 0.0f ? 0.0f : g;
            clean[i] = cf[i] / wb;
        }
        if (A.counts_in) nd_load_v<V>(A.counts_in + oc, cnt);
        if (A.reads_in) nd_load_v<V>(A.reads_in + oc, rd);
        if (A.quants_in) nd_load_v<V>(A.quants_in + oc, qu);
        if (!A.counts_in || !A.reads_in || !A.quants_in) {
#pragma unroll 1
            for (int i = 0; i < V; ++i) {
                if (!A.counts_in) {
                    const float latent = cf[i] / ratio32;
                    const double lamP = (double)latent / s.K;
                    cnt[i] = (float)philox_poisson(lamP, seed, e0 + (uint32_t)i, sample, draw);
                }
                if (!A.reads_in || !A.quants_in) {
                    uint32_t ctr[4] = {e0 + (uint32_t)i, sample, draw, PN_READ_BLOCK};
                    Philox::gen(ctr, k0, k1);
                    if (!A.reads_in) {
                        double r;
                        if (s.read_kind == 0) r = pn_box_muller(po_uniform(ctr[0]), po_uniform(ctr[1]));
                        else if (s.read_kind == 1) r = pn_tukey(po_uniform(ctr[2]), s.lam);
                        else r = __builtin_nan("");
                        rd[i] = (float)r;
                    }
                    if (!A.quants_in) qu[i] = (float)(po_uniform(ctr[3]) - 0.5);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            double v = s.K * (double)cnt[i];
            const double pr = s.s_read * (double)rd[i];
            v = v + pr;
            const double pg = s.s_row * (double)grow;
            v = v + pg;
            const double pq = s.qstep * (double)qu[i];
            v = v + pq;
            v = v + s.bias;
            v = nd_clip<double>(v, lo, wbd);
            v = v * s.ratio;
            v = v / wbd;
            if (clip01) v = nd_clip<double>(v, 0.0, 1.0);
            noisy[i] = (float)v;
        }
        nd_store_v<V>(A.noisy + oc, noisy);
        nd_store_v<V>(A.clean_out + oc, clean);
        if (A.noise_out) {
            float nz[V];
#pragma unroll
            for (int i = 0; i < V; ++i) nz[i] = noisy[i] - clean[i];
            nd_store_v<V>(A.noise_out + oc, nz);
        }
        if (A.counts_out) nd_store_v<V>(A.counts_out + oc, cnt);
        if (A.reads_out) nd_store_v<V>(A.reads_out + oc, rd);
        if (A.quants_out) nd_store_v<V>(A.quants_out + oc, qu);
    }
}

}  // namespace

extern "C" int nd_raw_physics_noise_f32(const uint16_t* frames, int N, int H2, int W2, const nd_physics_sample* table, const int64_t* rng,
                                        uint64_t seed, int64_t first_sample, int32_t draw, const float* counts_in, const float* reads_in,
                                        const float* rows_in, const float* quants_in, float* counts_out, float* reads_out, float* rows_out,
                                        float* quants_out, float black, float white, int flags, float* noisy, float* clean_out, float* noise_out,
                                        int B, int h, int w, void* stream) {
    const char* who = "nd_raw_physics_noise_f32";
    ND_REQUIRE(frames && table && noisy && clean_out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE((flags & ~ND_PHYS_CLIP01) == 0, ND_E_BADARG, "%s: unknown flags %d", who, flags);
    ND_REQUIRE(draw >= 0, ND_E_BADARG, "%s: draw index %d is negative", who, draw);
    ND_REQUIRE(white > black && black >= 0.0f && white <= 65535.0f, ND_E_BADARG, "%s: need 0 <= black < white <= 65535", who);
    ND_REQUIRE(N > 0 && H2 > 0 && W2 > 0 && h > 0 && w > 0 && B > 0 && B <= 65535, ND_E_BADARG, "%s: N, H2, W2, h, w and B (<= 65535) must be positive",
               who);
    ND_REQUIRE(H2 % 2 == 0 && W2 % 2 == 0, ND_E_BADARG, "%s: a Bayer frame has even sides; got %d x %d", who, H2, W2);
    ND_REQUIRE(h <= H2 / 2 && w <= W2 / 2, ND_E_BADARG, "%s: the window %d x %d does not fit the packed frame %d x %d", who, h, w, H2 / 2, W2 / 2);
    ND_REQUIRE((int64_t)4 * h * w < (1ll << 32), ND_E_BADARG, "%s: 4 * h * w must fit the 32-bit element counter", who);
    ND_REQUIRE(((uintptr_t)frames & 3u) == 0, ND_E_BADARG, "%s: frames must be 4-byte aligned", who);
    ND_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)rng & 7u) == 0, ND_E_BADARG, "%s: table and rng must be 8-byte aligned", who);
    const uintptr_t out_bits = (uintptr_t)noisy | (uintptr_t)clean_out | (uintptr_t)noise_out | (uintptr_t)counts_out | (uintptr_t)reads_out |
                               (uintptr_t)quants_out;
    const uintptr_t bits = out_bits | (uintptr_t)rows_out | (uintptr_t)counts_in | (uintptr_t)reads_in | (uintptr_t)rows_in | (uintptr_t)quants_in;
    ND_REQUIRE((bits & 3u) == 0, ND_E_BADARG, "%s: the outputs and the variate arrays must be 4-byte aligned", who);
    PhysArgs A;
    A.frames = frames;  A.table = table;  A.rng = rng;
    A.counts_in = counts_in;  A.reads_in = reads_in;  A.rows_in = rows_in;  A.quants_in = quants_in;
    A.counts_out = counts_out;  A.reads_out = reads_out;  A.rows_out = rows_out;  A.quants_out = quants_out;
    A.noisy = noisy;  A.clean_out = clean_out;  A.noise_out = noise_out;
    A.seed = seed;  A.first_sample = first_sample;  A.draw = draw;
    A.N = N;  A.H = H2 / 2;  A.W = W2 / 2;  A.h = h;  A.w = w;  A.flags = flags;  A.black = black;  A.white = white;
    const int V = rw_width(w, out_bits);
    const size_t threads = (size_t)h * (w / V);
    rw_dispatch(V, [&](auto v) {
        hipLaunchKernelGGL(physics_noise_kernel<v()>, dim3((unsigned)((threads + PN_THREADS - 1) / PN_THREADS), (unsigned)B), dim3(PN_THREADS), 0,
                           (hipStream_t)stream, A);
    });
    return nd_launch_status(who);
}
