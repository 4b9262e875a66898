// lsid_train.hip -- the gradient join at every LeakyReLU of LSID (models/archs/SID_arch.py:105-175) under loss.backward().
//
// Every convolution of the training forward stores its RAW output z; the consumers apply LeakyReLU(0.2) in their prologue and the
// ceil-mode 2x2 max-pools run on z (max commutes with a strictly increasing activation).  The backward therefore meets, at each z,
//
//   dz = (d_direct + pool_scatter(d_pool)) * (z > 0 ? 1 : 0.2)
//
//   d_direct  the gradient of LeakyReLU(z) through its direct consumers (the next convolution, the ConvTranspose, or the skip half of the
//             concat convolution's data gradient -- a channel slice of a wider tensor, hence its own pixel stride); may be NULL;
//   d_pool    the gradient of maxpool(LeakyReLU(z)) = the data gradient of the next stage's first convolution; may be NULL.  It goes to the
//             argmax of each 2x2 window -- the FIRST maximum in row-major order, windows hanging over the border use the in-bounds
//             elements only: what max_pool2d(ceil_mode=True)'s backward does (max_pool2d_with_indices: `val > maxval || isnan(val)`).
//             The argmax of z equals the argmax of LeakyReLU(z), ties included, since LeakyReLU is strictly increasing.
//
// The slope at z == 0 is 0.2: leaky_relu_backward's `> 0` test on the in-place activation's result.  One streaming pass: thread =
// (sample, pooled pixel, channel quad) -- it reads the 2x2 window of z once and writes the four gradients of the window.
#include "nd_common.h"

namespace {

__device__ __forceinline__ float lk_slope(float z) { return z > 0.0f ? 1.0f : 0.2f; }

__global__ __launch_bounds__(256) void leaky_grad_join_kernel(const float* __restrict__ z, float* dz, const float* dd, int ldd,
                                                              const float* __restrict__ dp, int B, int H, int W, int C) {
    const int Ho = (H + 1) >> 1, Wo = (W + 1) >> 1, cq = C >> 2;
    const size_t total = (size_t)B * Ho * Wo * cq;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cq) * 4;
        size_t r = i / cq;
        const int x = (int)(r % Wo); r /= Wo;
        const int y = (int)(r % Ho);
        const int b = (int)(r / Ho);
        const int ny = min(2, H - 2 * y), nx = min(2, W - 2 * x);          // the in-bounds part of the window
        size_t pix[4];
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = 2 * y + min(k >> 1, ny - 1), xx = 2 * x + min(k & 1, nx - 1);    // clamped: out-of-window slots repeat an in-bounds element
            pix[k] = ((size_t)b * H + yy) * W + xx;
            v[k] = nd_ld4(z + pix[k] * C + c);
        }
        f32x4 g = {0, 0, 0, 0};
        int am[4] = {0, 0, 0, 0};                                           // window slot of the argmax, per channel
        if (dp) {
            g = nd_ld4(dp + i * 4);
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                float m = v[0][ch];
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    const bool in = (k >> 1) < ny && (k & 1) < nx;
                    const float e = v[k][ch];
                    if (in && (e > m || e != e)) { m = e;  am[ch] = k; }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((k >> 1) >= ny || (k & 1) >= nx) continue;
            f32x4 d = {0, 0, 0, 0};
            if (dd) d = nd_ld4(dd + pix[k] * ldd + c);
            f32x4 o;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const float s = d[ch] + (am[ch] == k ? g[ch] : 0.0f);
                o[ch] = s * lk_slope(v[k][ch]);
            }
            nd_st4(dz + pix[k] * C + c, o);
        }
    }
}

}  // namespace

extern "C" int nd_leaky_grad_join_f32(const float* z, float* dz, const float* d_direct, int ld_direct, const float* d_pool, int B, int H, int W, int C,
                                      void* stream) {
    ND_REQUIRE(z && dz && (d_direct || d_pool), ND_E_BADARG, "nd_leaky_grad_join: null pointer (z, dz and at least one of d_direct / d_pool)");
    ND_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, ND_E_BADARG, "nd_leaky_grad_join: non-positive size");
    ND_REQUIRE(C % 4 == 0 && (!d_direct || (ld_direct >= C && ld_direct % 4 == 0)), ND_E_SHAPE,
               "nd_leaky_grad_join: C=%d and the d_direct pixel stride (%d) must be multiples of 4, stride >= C", C, ld_direct);
    ND_REQUIRE(nd_aligned16(z) && nd_aligned16(dz) && nd_aligned16(d_direct) && nd_aligned16(d_pool), ND_E_ALIGN, "nd_leaky_grad_join: pointers must be 16-byte aligned");
    ND_REQUIRE(dz != z && (const float*)dz != d_pool && ((const float*)dz != d_direct || ld_direct == C), ND_E_BADARG,
               "nd_leaky_grad_join: dz may alias d_direct only, and only when d_direct is dense (ld_direct == C)");
    const size_t total = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(leaky_grad_join_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream,
                       z, dz, d_direct, ld_direct, d_pool, B, H, W, C);
    return nd_launch_status("nd_leaky_grad_join_f32");
}
