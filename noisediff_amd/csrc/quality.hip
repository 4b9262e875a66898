// quality.hip -- scoring of denoised frames (test_denoising.py:220-263,318-343): illumination correction, PSNR and SSIM.
//
//   IlluminanceCorrect  p = clamp(pred, 0, 1), m = (source != 1), k = sum(m p s) / sum(m p p), out = fl32(k) * p       (:232-263)
//   PSNR                10 log10(R^2 / mse), mse = mean over all C*H*W of fl32(fl32(x - y)^2), accumulated in fp64   (skimage >= 0.19)
//   SSIM                structural_similarity(channel_axis=2, data_range=R) with its defaults: 7 x 7 uniform window, cov_norm 49/48,
//                       K1 0.01, K2 0.03, S averaged over the interior [3, H-3) x [3, W-3) of each channel, then over channels
//
// Inputs are clipped to [0, R] first, as both tensor2im helpers do; the clip keeps NaN (comparisons, not fminf / fmaxf).  The window sums
// and S are fp64: a product of two fp32 values is exact in fp64, so the fma in the horizontal sums rounds exactly as mul + add would.
//
// Determinism: no atomics.  The quality kernel writes one fp64 pair (sum S, sum d^2) per (image, channel, tile) slot, the illumination
// partial kernel one pair (num, den) per (image, chunk); the slot layout of an image depends on (C, H, W) only.  The finalize kernels sum
// an image's slots in a fixed order (thread-strided, then a fixed tree), so a repeated call gives the same bits and an image's results
// in a batch of any size equal its results alone.
#include "nd_common.h"
#include "block_sum.h"

namespace {

constexpr int QT_W = 256;                 // output columns per tile = threads per workgroup, one column per lane
constexpr int QT_H = 32;                  // output rows per tile; the walk covers QT_H + 6 input rows
constexpr int Q_R = 3;                    // window radius (7 x 7)
constexpr int Q_LDS = QT_W + 8;           // one staged row: columns x0-4 .. x0+QT_W+3 (starts 16-byte aligned when W % 4 == 0)
constexpr int Q_VEC_LANES = Q_LDS / 4;    // float4 loads per tensor and row
constexpr int IL_THREADS = 256;
constexpr int IL_CHUNK = IL_THREADS * 4 * 16;     // elements per illumination partial: 16 float4 per thread

// One (image, channel, QT_H x QT_W tile) per workgroup.  The block walks the tile's input rows y0-3 .. y1+2 top to bottom: every row is
// staged in LDS (clipped, and illumination-corrected when `scale` is given), each lane forms the five horizontal 7-sums of its column
// (x, y, xx, yy, xy) in fp64 and keeps the last seven rows of them in a register ring; once seven rows are in, the ring's vertical sums
// give the window means of the output row three above.  No running sums: each window is summed afresh from its 49 products.
// VEC: W % 4 == 0 and both planes 16-byte aligned -- a staged row is 66 float4 per tensor; else one float per lane (and 8 more).
template <bool VEC>
__global__ __launch_bounds__(QT_W) void quality_tile_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                            const float* __restrict__ scale, float R, double C1, double C2,
                                                            double* __restrict__ slots, int C, int H, int W, int ntx, int nty) {
    __shared__ __attribute__((aligned(16))) float xs[2][Q_LDS];
    __shared__ __attribute__((aligned(16))) float ys[2][Q_LDS];
    __shared__ double red[2][4];
    const int tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tx = tile % ntx, ty = tile / ntx;
    const int x0 = tx * QT_W, y0 = ty * QT_H, y1 = min(H, y0 + QT_H);
    const size_t plane = ((size_t)b * C + c) * (size_t)H * W;
    const float* ep = est + plane;
    const float* tp = tgt + plane;
    const bool corr = scale != nullptr;
    const float k = corr ? scale[b] : 1.0f;
    const int t = threadIdx.x, x = x0 + t;
    const bool in_x = x < W, s_x = x >= Q_R && x < W - Q_R;
    const int rb = y0 - Q_R, re = y1 + Q_R;

    auto fx = [&](float v) { return corr ? nd_clip(k * nd_clip(v, 0.0f, 1.0f), 0.0f, R) : nd_clip(v, 0.0f, R); };

    // ---- the row loader: global -> registers (issued a row ahead), registers -> LDS
    f32x4 v4 = {0.0f, 0.0f, 0.0f, 0.0f};           // VEC: threads 0..65 hold est, 66..131 target
    float e0 = 0.0f, g0 = 0.0f, e1 = 0.0f, g1 = 0.0f;      // scalar: column t and, for t < 8, column QT_W + t of the staged row
    auto load = [&](int r) {
        const bool row_in = r >= 0 && r < H;
        if (VEC) {
            v4 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (row_in && t < 2 * Q_VEC_LANES) {
                const bool is_t = t >= Q_VEC_LANES;
                const int col = x0 - 4 + 4 * (is_t ? t - Q_VEC_LANES : t);
                if (col >= 0 && col < W) v4 = nd_ld4((is_t ? tp : ep) + (size_t)r * W + col);      // W % 4 == 0: all four in range
            }
        } else {
            e0 = g0 = e1 = g1 = 0.0f;
            if (row_in) {
                const int c0 = x0 - 4 + t, c1 = x0 - 4 + QT_W + t;
                if (c0 >= 0 && c0 < W) { e0 = ep[(size_t)r * W + c0];  g0 = tp[(size_t)r * W + c0]; }
                if (t < Q_LDS - QT_W && c1 < W) { e1 = ep[(size_t)r * W + c1];  g1 = tp[(size_t)r * W + c1]; }
            }
        }
    };
    auto store = [&](int buf) {
        if (VEC) {
            if (t < Q_VEC_LANES) nd_st4(&xs[buf][4 * t], f32x4{fx(v4[0]), fx(v4[1]), fx(v4[2]), fx(v4[3])});
            else if (t < 2 * Q_VEC_LANES)
                nd_st4(&ys[buf][4 * (t - Q_VEC_LANES)], f32x4{nd_clip(v4[0], 0.0f, R), nd_clip(v4[1], 0.0f, R), nd_clip(v4[2], 0.0f, R), nd_clip(v4[3], 0.0f, R)});
        } else {
            xs[buf][t] = fx(e0);
            ys[buf][t] = nd_clip(g0, 0.0f, R);
            if (t < Q_LDS - QT_W) { xs[buf][QT_W + t] = fx(e1);  ys[buf][QT_W + t] = nd_clip(g1, 0.0f, R); }
        }
    };

    double ring[7][5];
#pragma unroll
    for (int s = 0; s < 7; ++s)
#pragma unroll
        for (int q = 0; q < 5; ++q) ring[s][q] = 0.0;
    double accS = 0.0, accD = 0.0;
    constexpr double inv49 = 1.0 / 49.0, cov_norm = 49.0 / 48.0;

    load(rb);
    for (int r0 = rb; r0 < re; r0 += 7) {
#pragma unroll
        for (int s = 0; s < 7; ++s) {             // ring slot s holds row r with (r - rb) % 7 == s: compile-time register indices
            const int r = r0 + s;
            if (r >= re) break;                   // block-uniform
            const int buf = (r - rb) & 1;         // two LDS rows: the one written here was last read two rows ago, before the barrier of the previous row
            store(buf);
            __syncthreads();
            if (r + 1 < re) load(r + 1);
            const float* xr = &xs[buf][t + 1];    // columns x-3 .. x+3
            const float* yr = &ys[buf][t + 1];
            double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const double a = xr[d], g = yr[d];
                hx += a;
                hy += g;
                hxx = fma(a, a, hxx);
                hyy = fma(g, g, hyy);
                hxy = fma(a, g, hxy);
            }
            ring[s][0] = hx;  ring[s][1] = hy;  ring[s][2] = hxx;  ring[s][3] = hyy;  ring[s][4] = hxy;
            if (r >= y0 && r < y1 && in_x) {
                const float d = xr[3] - yr[3];
                accD += (double)(d * d);
            }
            const int yo = r - Q_R;               // the output row whose window the ring now covers
            if (r - rb >= 6 && yo >= Q_R && yo < H - Q_R && s_x) {
                double u[5];
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    u[q] = ((ring[0][q] + ring[1][q]) + (ring[2][q] + ring[3][q])) + ((ring[4][q] + ring[5][q]) + ring[6][q]);
                const double ux = u[0] * inv49, uy = u[1] * inv49, uxx = u[2] * inv49, uyy = u[3] * inv49, uxy = u[4] * inv49;
                const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
                const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
                accS += (A1 * A2) / (B1 * B2);
            }
        }
    }
    block_sum_all(accS, accD, red);
    if (t == 0) {
        double* o = slots + ((size_t)b * C * nty * ntx + ((size_t)c * nty + ty) * ntx + tx) * 2;
        o[0] = accS;
        o[1] = accD;
    }
}

// One block per image: that image's `nslot` pairs summed thread-strided, then in block_sum_all's tree.
__global__ __launch_bounds__(256) void quality_finalize_kernel(const double* __restrict__ slots, int nslot, double R2, double n_all,
                                                               double n_int, double* psnr, double* ssim, double* mse) {
    __shared__ double red[2][4];
    const int b = blockIdx.x;
    const double* s = slots + (size_t)b * nslot * 2;
    double aS = 0.0, aD = 0.0;
    for (int i = threadIdx.x; i < nslot; i += 256) {
        aS += s[2 * i];
        aD += s[2 * i + 1];
    }
    block_sum_all(aS, aD, red);
    if (threadIdx.x == 0) {
        const double m = aD / n_all;
        mse[b] = m;
        psnr[b] = 10.0 * log10(R2 / m);           // mse 0: +inf, as skimage
        ssim[b] = aS / n_int;
    }
}

// num / den partials of one (chunk, image).  Thread t takes elements start + 4 t + 1024 i + e in that order on both paths, so the sums do
// not depend on which path runs.
template <bool VEC>
__global__ __launch_bounds__(IL_THREADS) void illum_partial_kernel(const float* __restrict__ pred, const float* __restrict__ src, int src_batch,
                                                                   double* __restrict__ part, size_t n, int nchunk) {
    __shared__ double red[2][4];
    const int chunk = blockIdx.x, b = blockIdx.y;
    const float* p = pred + (size_t)b * n;
    const float* s = src + (src_batch == 1 ? (size_t)0 : (size_t)b * n);
    const size_t start = (size_t)chunk * IL_CHUNK, end = min(n, start + IL_CHUNK);
    double num = 0.0, den = 0.0;
    for (size_t i = start + 4 * threadIdx.x; i < end; i += 4 * IL_THREADS) {
        f32x4 pv, sv;
        if (VEC) {
            pv = nd_ld4(p + i);
            sv = nd_ld4(s + i);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pv[e] = i + e < end ? p[i + e] : 0.0f;
                sv[e] = i + e < end ? s[i + e] : 1.0f;      // masked out
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double pc = nd_clip(pv[e], 0.0f, 1.0f);
            if (sv[e] != 1.0f) {
                num = fma(pc, (double)sv[e], num);
                den = fma(pc, pc, den);
            }
        }
    }
    block_sum_all(num, den, red);
    if (threadIdx.x == 0) {
        part[((size_t)b * nchunk + chunk) * 2] = num;
        part[((size_t)b * nchunk + chunk) * 2 + 1] = den;
    }
}

__global__ __launch_bounds__(IL_THREADS) void illum_finalize_kernel(const double* __restrict__ part, int nchunk, float* k32, double* k64) {
    __shared__ double red[2][4];
    const int b = blockIdx.x;
    const double* q = part + (size_t)b * nchunk * 2;
    double num = 0.0, den = 0.0;
    for (int i = threadIdx.x; i < nchunk; i += IL_THREADS) {
        num += q[2 * i];
        den += q[2 * i + 1];
    }
    block_sum_all(num, den, red);
    if (threadIdx.x == 0) {
        const double kk = num / den;              // den 0: NaN or inf, as the reference
        k64[b] = kk;
        k32[b] = (float)kk;
    }
}

template <bool VEC>
__global__ __launch_bounds__(IL_THREADS) void illum_apply_kernel(const float* pred, const float* __restrict__ k32, float* out, size_t n) {     // out may alias pred
    const int b = blockIdx.y;
    const float k = k32[b];
    const float* p = pred + (size_t)b * n;
    float* o = out + (size_t)b * n;
    const size_t start = (size_t)blockIdx.x * IL_CHUNK, end = min(n, start + IL_CHUNK);
    for (size_t i = start + 4 * threadIdx.x; i < end; i += 4 * IL_THREADS) {
        if (VEC) {
            const f32x4 v = nd_ld4(p + i);
            nd_st4(o + i, f32x4{k * nd_clip(v[0], 0.0f, 1.0f), k * nd_clip(v[1], 0.0f, 1.0f), k * nd_clip(v[2], 0.0f, 1.0f), k * nd_clip(v[3], 0.0f, 1.0f)});
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < end) o[i + e] = k * nd_clip(p[i + e], 0.0f, 1.0f);
        }
    }
}

bool q_sizes_ok(int B, int C, int H, int W) {
    return B > 0 && C > 0 && H > 0 && W > 0 && B <= 65535 && C <= 65535;
}
int q_ntx(int W) { return nd_cdiv(W, QT_W); }
int q_nty(int H) { return nd_cdiv(H, QT_H); }
int64_t q_chunks(int C, int H, int W) { return ((int64_t)C * H * W + IL_CHUNK - 1) / IL_CHUNK; }

}  // namespace

extern "C" int64_t nd_image_quality_workspace_bytes(int B, int C, int H, int W) {
    ND_REQUIRE(q_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_image_quality_workspace_bytes: sizes must be positive (B, C <= 65535)");
    ND_REQUIRE(H >= 7 && W >= 7, ND_E_SHAPE, "nd_image_quality_workspace_bytes: H=%d and W=%d must be at least 7 (the SSIM window)", H, W);
    return (int64_t)B * C * q_nty(H) * q_ntx(W) * 2 * (int64_t)sizeof(double);
}

extern "C" int nd_image_quality_f32(const float* est, const float* target, const float* scale, double data_range, double* psnr, double* ssim,
                                    double* mse, void* workspace, int B, int C, int H, int W, void* stream) {
    ND_REQUIRE(est && target && psnr && ssim && mse && workspace, ND_E_BADARG, "nd_image_quality_f32: null pointer");
    ND_REQUIRE(q_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_image_quality_f32: sizes must be positive (B, C <= 65535)");
    ND_REQUIRE(data_range > 0.0 && data_range < 3.0e38, ND_E_BADARG, "nd_image_quality_f32: data_range must be positive and finite");
    ND_REQUIRE(H >= 7 && W >= 7, ND_E_SHAPE, "nd_image_quality_f32: H=%d and W=%d must be at least 7 (the SSIM window)", H, W);
    ND_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)psnr & 7u) == 0 && ((uintptr_t)ssim & 7u) == 0 && ((uintptr_t)mse & 7u) == 0,
               ND_E_ALIGN, "nd_image_quality_f32: workspace and outputs must be 8-byte aligned");
    const int ntx = q_ntx(W), nty = q_nty(H);
    ND_REQUIRE((int64_t)ntx * nty < (1ll << 31), ND_E_SHAPE, "nd_image_quality_f32: image too large");
    const double R = data_range, K1 = 0.01, K2 = 0.03;
    const double C1 = (K1 * R) * (K1 * R), C2 = (K2 * R) * (K2 * R);
    const bool vec = W % 4 == 0 && nd_aligned16(est) && nd_aligned16(target);
    const dim3 grid((unsigned)(ntx * nty), (unsigned)C, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    double* slots = (double*)workspace;
    if (vec)
        hipLaunchKernelGGL(quality_tile_kernel<true>, grid, dim3(QT_W), 0, st, est, target, scale, (float)R, C1, C2, slots, C, H, W, ntx, nty);
    else
        hipLaunchKernelGGL(quality_tile_kernel<false>, grid, dim3(QT_W), 0, st, est, target, scale, (float)R, C1, C2, slots, C, H, W, ntx, nty);
    int e = nd_launch_status("nd_image_quality_f32 (tiles)");
    if (e) return e;
    const double n_all = (double)C * H * W, n_int = (double)C * (H - 2 * Q_R) * (W - 2 * Q_R);
    hipLaunchKernelGGL(quality_finalize_kernel, dim3(B), dim3(256), 0, st, slots, C * nty * ntx, R * R, n_all, n_int, psnr, ssim, mse);
    return nd_launch_status("nd_image_quality_f32 (finalize)");
}

extern "C" int64_t nd_illum_scale_workspace_bytes(int B, int C, int H, int W) {
    ND_REQUIRE(q_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_illum_scale_workspace_bytes: sizes must be positive (B, C <= 65535)");
    return (int64_t)B * q_chunks(C, H, W) * 2 * (int64_t)sizeof(double);
}

extern "C" int nd_illum_scale_f32(const float* pred, const float* source, int source_batch, float* k32, double* k64, void* workspace,
                                  int B, int C, int H, int W, void* stream) {
    ND_REQUIRE(pred && source && k32 && k64 && workspace, ND_E_BADARG, "nd_illum_scale_f32: null pointer");
    ND_REQUIRE(q_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_illum_scale_f32: sizes must be positive (B, C <= 65535)");
    ND_REQUIRE(source_batch == 1 || source_batch == B, ND_E_BADARG, "nd_illum_scale_f32: source batch %d must be 1 or B=%d", source_batch, B);
    ND_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)k64 & 7u) == 0 && ((uintptr_t)k32 & 3u) == 0, ND_E_ALIGN,
               "nd_illum_scale_f32: workspace and k64 must be 8-byte aligned, k32 4-byte");
    const int64_t nchunk = q_chunks(C, H, W);
    ND_REQUIRE(nchunk < (1ll << 31), ND_E_SHAPE, "nd_illum_scale_f32: image too large");
    const size_t n = (size_t)C * H * W;
    const bool vec = n % 4 == 0 && nd_aligned16(pred) && nd_aligned16(source);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    if (vec) hipLaunchKernelGGL(illum_partial_kernel<true>, grid, dim3(IL_THREADS), 0, st, pred, source, source_batch, part, n, (int)nchunk);
    else hipLaunchKernelGGL(illum_partial_kernel<false>, grid, dim3(IL_THREADS), 0, st, pred, source, source_batch, part, n, (int)nchunk);
    int e = nd_launch_status("nd_illum_scale_f32 (partials)");
    if (e) return e;
    hipLaunchKernelGGL(illum_finalize_kernel, dim3(B), dim3(IL_THREADS), 0, st, part, (int)nchunk, k32, k64);
    return nd_launch_status("nd_illum_scale_f32 (finalize)");
}

extern "C" int nd_illum_apply_f32(const float* pred, const float* k32, float* out, int B, int C, int H, int W, void* stream) {
    ND_REQUIRE(pred && k32 && out, ND_E_BADARG, "nd_illum_apply_f32: null pointer");
    ND_REQUIRE(q_sizes_ok(B, C, H, W), ND_E_BADARG, "nd_illum_apply_f32: sizes must be positive (B, C <= 65535)");
    const int64_t nchunk = q_chunks(C, H, W);
    ND_REQUIRE(nchunk < (1ll << 31), ND_E_SHAPE, "nd_illum_apply_f32: image too large");
    const size_t n = (size_t)C * H * W;
    const bool vec = n % 4 == 0 && nd_aligned16(pred) && nd_aligned16(out);
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    if (vec) hipLaunchKernelGGL(illum_apply_kernel<true>, grid, dim3(IL_THREADS), 0, (hipStream_t)stream, pred, k32, out, n);
    else hipLaunchKernelGGL(illum_apply_kernel<false>, grid, dim3(IL_THREADS), 0, (hipStream_t)stream, pred, k32, out, n);
    return nd_launch_status("nd_illum_apply_f32");
}
