// denoise_loss.hip -- the end of a denoiser training step (models/trainer_denoising.py:66-76, 225-235): loss = mse * lambda_mse + l1 * lambda_l1 of the
// network output against the clean image, where the reference spends about ten ATen kernels (subtract, abs / square, mean; expand, divide, sign, multiply,
// copy) and the project two layout passes to hand ATen its layout.
//
//   nd_denoise_loss_f32           TWO launches: per-slice partial sums of |d| and d^2, then one workgroup that forms the loss and its terms.
//   nd_denoise_loss_backward_f32  ONE launch: the loss gradient with respect to the network output, written in the output's own layout.
//
// `out` is NCHW (C from 1 to 16) or NHWC (C = 4: LSID's 1x1 head writes a pixel's four channels as one float4), `target` always NCHW (what the batch
// builders emit).  Arithmetic, every operation rounded on its own (no contraction):
//   d = fl(out - target) in fp32.  |d| and d * d are formed and summed in fp64 (a product of two fp32 values is exact there).
//   loss = (float)(lambda_mse * S2 / N + lambda_l1 * S1 / N), N = B * C * HW, S1 = sum |d|, S2 = sum d^2; terms = {loss, (float)(S1 / N), (float)(S2 / N)};
//   sample_terms[b] = {(float)(S1_b / (C HW)), (float)(S2_b / (C HW))}.
//   grad = (float)((g * lambda_l1 / N) * sign(d) + (g * 2 * lambda_mse / N) * d), in fp64, rounded once; sign(0) = 0.  With lambda >= 0 the two terms
//   have d's sign and never cancel.  With lambda_mse = 0 this is (float)(g / N) * sign(d) exactly: what ATen's l1_loss gives.
// The summation order is defined over pixels and channels, not over memory: a sample's HW pixels are cut into slices of LOSS_PIXELS pixels, one workgroup
// each; thread i of the workgroup takes the slice's pixels i, i + 256, ... in that order and, of each pixel, the channels 0 .. C - 1 in that order; the 256
// thread sums are folded by a fixed butterfly, the slices of a sample are added in slice order, the samples in a fixed tree.  So loss, terms and sample
// terms are the same bits whether `out` arrives NCHW or NHWC, and a sample's sums depend on neither B nor the sample's row in the batch.  No atomics
// anywhere; every store is a vector store.  Planes are read one float per lane (a plane's base is 16-byte aligned only when HW % 4 == 0); consecutive
// lanes read consecutive pixels, so every load and store is coalesced.
#include "nd_common.h"
#include "block_sum.h"

#pragma clang fp contract(off)

namespace {

constexpr int LOSS_PIXELS = 1024;         // pixels of one sample per workgroup: 256 threads x 4 pixels
constexpr int LOSS_MAX_C = 16;

__host__ __device__ inline int loss_slices(int HW) { return (HW + LOSS_PIXELS - 1) / LOSS_PIXELS; }

// The C values of pixel `pix` of sample b: one float4 in NHWC (C == 4), C planes HW apart in NCHW.
template <bool NHWC>
__device__ __forceinline__ void load_pixel(const float* __restrict__ x, int b, int C, int HW, int pix, float (&v)[LOSS_MAX_C]) {
    if constexpr (NHWC) {
        const f32x4 q = nd_ld4(x + ((size_t)b * HW + pix) * 4);
        v[0] = q.x;  v[1] = q.y;  v[2] = q.z;  v[3] = q.w;
    } else {
        const float* p = x + (size_t)b * C * HW + pix;
#pragma unroll
        for (int c = 0; c < LOSS_MAX_C; ++c)
            if (c < C) v[c] = p[(size_t)c * HW];
    }
}

// grid (ns, B): slice k of sample b -> part[b][k] = {sum |d|, sum d^2}
template <bool NHWC>
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ out, const float* __restrict__ tgt, double* __restrict__ part, int C, int HW) {
    __shared__ double red[4];
    const int k = blockIdx.x, b = blockIdx.y, ns = gridDim.x;
    const int lo = k * LOSS_PIXELS, hi = HW - lo < LOSS_PIXELS ? HW : lo + LOSS_PIXELS;
    double a1 = 0.0, a2 = 0.0;
    for (int pix = lo + (int)threadIdx.x; pix < hi; pix += 256) {
        float o[LOSS_MAX_C], t[LOSS_MAX_C];
        load_pixel<NHWC>(out, b, C, HW, pix, o);
        load_pixel<false>(tgt, b, C, HW, pix, t);
#pragma unroll
        for (int c = 0; c < LOSS_MAX_C; ++c) {
            if (c < C) {
                const double d = (double)(o[c] - t[c]);
                a1 += fabs(d);
                a2 += d * d;
            }
        }
    }
    const double s1 = block_sum(a1, red), s2 = block_sum(a2, red);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)b * ns + k) * 2;
        p[0] = s1;
        p[1] = s2;
    }
}

// one workgroup: a sample's slices in slice order, the samples in a fixed tree
__global__ __launch_bounds__(256) void loss_final_kernel(const double* __restrict__ part, int B, int C, int HW, int ns, double lambda_l1, double lambda_mse,
                                                         float* __restrict__ terms, float* __restrict__ sample_terms) {
    __shared__ double red[4];
    const double n = (double)C * (double)HW;
    double p1 = 0.0, p2 = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < ns; ++k) {
            s1 += part[((size_t)b * ns + k) * 2];
            s2 += part[((size_t)b * ns + k) * 2 + 1];
        }
        if (sample_terms) {
            sample_terms[2 * b] = (float)(s1 / n);
            sample_terms[2 * b + 1] = (float)(s2 / n);
        }
        p1 += s1;
        p2 += s2;
    }
    const double N = (double)B * n;
    const double l1 = block_sum(p1, red) / N, mse = block_sum(p2, red) / N;
    if (threadIdx.x == 0) {
        terms[0] = (float)(lambda_mse * mse + lambda_l1 * l1);
        terms[1] = (float)l1;
        terms[2] = (float)mse;
    }
}

// grid (ns, B): grad = (float)(a sign(d) + m d), a = g lambda_l1 / N, m = g 2 lambda_mse / N, in out's layout
template <bool NHWC>
__global__ __launch_bounds__(256) void loss_backward_kernel(const float* __restrict__ out, const float* __restrict__ tgt, const float* __restrict__ g,
                                                            float* __restrict__ grad, int B, int C, int HW, double lambda_l1, double lambda_mse) {
    const int k = blockIdx.x, b = blockIdx.y;
    const int lo = k * LOSS_PIXELS, hi = HW - lo < LOSS_PIXELS ? HW : lo + LOSS_PIXELS;
    const double gd = (double)*g, N = (double)B * ((double)C * (double)HW);
    const double a = gd * lambda_l1 / N, m = gd * 2.0 * lambda_mse / N;
    for (int pix = lo + (int)threadIdx.x; pix < hi; pix += 256) {
        float o[LOSS_MAX_C], t[LOSS_MAX_C], r[LOSS_MAX_C];
        load_pixel<NHWC>(out, b, C, HW, pix, o);
        load_pixel<false>(tgt, b, C, HW, pix, t);
#pragma unroll
        for (int c = 0; c < LOSS_MAX_C; ++c) {
            if (c < C) {
                const double d = (double)(o[c] - t[c]);
                const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                r[c] = (float)(a * sg + m * d);
            }
        }
        if constexpr (NHWC) nd_st4(grad + ((size_t)b * HW + pix) * 4, f32x4{r[0], r[1], r[2], r[3]});
        else {
            float* p = grad + (size_t)b * C * HW + pix;
#pragma unroll
            for (int c = 0; c < LOSS_MAX_C; ++c)
                if (c < C) p[(size_t)c * HW] = r[c];
        }
    }
}

int check_shape(int layout, int B, int C, int HW, const char* who) {
    ND_REQUIRE(B > 0 && C > 0 && HW > 0, ND_E_BADARG, "%s: B=%d, C=%d, HW=%d must be positive", who, B, C, HW);
    ND_REQUIRE(layout == ND_LAYOUT_NCHW || layout == ND_LAYOUT_NHWC, ND_E_BADARG, "%s: out_layout %d is neither ND_LAYOUT_NCHW nor ND_LAYOUT_NHWC", who, layout);
    ND_REQUIRE(C <= LOSS_MAX_C, ND_E_SHAPE, "%s: C=%d: at most %d channels", who, C, LOSS_MAX_C);
    ND_REQUIRE(layout == ND_LAYOUT_NCHW || C == 4, ND_E_SHAPE, "%s: an NHWC output has C = 4 (a pixel is one float4), got C=%d", who, C);
    ND_REQUIRE(B <= 65535, ND_E_SHAPE, "%s: B=%d (<= 65535)", who, B);
    return 0;
}

int check_lambdas(double lambda_l1, double lambda_mse, const char* who) {
    ND_REQUIRE(lambda_l1 >= 0.0 && lambda_mse >= 0.0 && lambda_l1 <= 1.0e300 && lambda_mse <= 1.0e300, ND_E_BADARG,
               "%s: lambda_l1=%g and lambda_mse=%g must be finite and not negative", who, lambda_l1, lambda_mse);
    ND_REQUIRE(lambda_l1 > 0.0 || lambda_mse > 0.0, ND_E_BADARG, "%s: lambda_l1 and lambda_mse are both zero: there is no loss", who);
    return 0;
}

}  // namespace

extern "C" int nd_denoise_loss_slice_pixels(void) { return LOSS_PIXELS; }

extern "C" int64_t nd_denoise_loss_workspace_bytes(int B, int C, int HW) {
    if (int e = check_shape(ND_LAYOUT_NCHW, B, C, HW, "nd_denoise_loss_workspace_bytes")) return e;
    return 16 * (int64_t)B * loss_slices(HW);
}

extern "C" int nd_denoise_loss_f32(const float* out, int out_layout, const float* target, int B, int C, int HW, double lambda_l1, double lambda_mse,
                                   void* workspace, float* terms, float* sample_terms, void* stream) {
    const char* who = "nd_denoise_loss_f32";
    ND_REQUIRE(out && target && workspace && terms, ND_E_BADARG, "%s: null pointer", who);
    if (int e = check_shape(out_layout, B, C, HW, who)) return e;
    if (int e = check_lambdas(lambda_l1, lambda_mse, who)) return e;
    ND_REQUIRE(nd_aligned16(out) && nd_aligned16(target) && nd_aligned16(workspace), ND_E_ALIGN, "%s: out, target and workspace must be 16-byte aligned", who);
    ND_REQUIRE((((uintptr_t)terms | (uintptr_t)sample_terms) & 3u) == 0, ND_E_ALIGN, "%s: terms and sample_terms must be 4-byte aligned", who);
    const int ns = loss_slices(HW);
    double* part = (double*)workspace;
    if (out_layout == ND_LAYOUT_NHWC) hipLaunchKernelGGL(loss_partial_kernel<true>, dim3(ns, B), dim3(256), 0, (hipStream_t)stream, out, target, part, C, HW);
    else hipLaunchKernelGGL(loss_partial_kernel<false>, dim3(ns, B), dim3(256), 0, (hipStream_t)stream, out, target, part, C, HW);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, B, C, HW, ns, lambda_l1, lambda_mse, terms, sample_terms);
    return nd_launch_status(who);
}

extern "C" int nd_denoise_loss_backward_f32(const float* out, int out_layout, const float* target, const float* g, float* grad, int B, int C, int HW,
                                            double lambda_l1, double lambda_mse, void* stream) {
    const char* who = "nd_denoise_loss_backward_f32";
    ND_REQUIRE(out && target && g && grad, ND_E_BADARG, "%s: null pointer", who);
    if (int e = check_shape(out_layout, B, C, HW, who)) return e;
    if (int e = check_lambdas(lambda_l1, lambda_mse, who)) return e;
    ND_REQUIRE(nd_aligned16(out) && nd_aligned16(target) && nd_aligned16(grad), ND_E_ALIGN, "%s: out, target and grad must be 16-byte aligned", who);
    ND_REQUIRE((((uintptr_t)g) & 3u) == 0, ND_E_ALIGN, "%s: g must be 4-byte aligned", who);
    const int ns = loss_slices(HW);
    if (out_layout == ND_LAYOUT_NHWC)
        hipLaunchKernelGGL(loss_backward_kernel<true>, dim3(ns, B), dim3(256), 0, (hipStream_t)stream, out, target, g, grad, B, C, HW, lambda_l1, lambda_mse);
    else
        hipLaunchKernelGGL(loss_backward_kernel<false>, dim3(ns, B), dim3(256), 0, (hipStream_t)stream, out, target, g, grad, B, C, HW, lambda_l1, lambda_mse);
    return nd_launch_status(who);
}
