// block_sum.h -- the library's fixed-order fp64 sums over a 256-thread workgroup.  Every form is an xor butterfly in each wave, then the four wave
// sums r0..r3 from LDS; the "same bits on every call" contracts rest on the order of that last step, and there are TWO orders:
//
//   block_sum        ((r0 + r1) + r2) + r3, valid in thread 0 only.  The loss kernels: nd_diffusion_loss_f32 (diffusion_train.hip) and
//                    nd_denoise_loss_f32 (denoise_loss.hip).
//   block_sum_all    (r0 + r1) + (r2 + r3), K values at once, every thread gets the results.  The scoring and fitting kernels:
//                    nd_image_quality_f32, nd_illum_scale_f32 (quality.hip), nd_kl_div_f64, nd_kl_div_hist_f64, nd_patch_std_mean_f32
//                    (noise_stats.hip), nd_theil_sen_f64 (noise_level.hip).
//
// The two trees round differently: folding them into one changes the bits of the entry points on one side and the values their tests pin.
#pragma once
#include "nd_common.h"

__device__ __forceinline__ double wave_sum(double v) {             // all 64 lanes, fixed order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, ND_WAVE);
    return v;
}
// sum over the 256 threads of a workgroup, valid in thread 0; `lds`: 4 doubles
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    __syncthreads();                                               // (lds may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// K sums over the 256 threads of a workgroup, in place, valid in every thread; `red`: K x 4 doubles
template <int K>
__device__ __forceinline__ void block_sum_all(double (&a)[K], double (*red)[4]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += __shfl_xor(a[k], o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][w] = a[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}
__device__ __forceinline__ void block_sum_all(double& a, double& b, double (*red)[4]) {
    double v[2] = {a, b};
    block_sum_all<2>(v, red);
    a = v[0];  b = v[1];
}
