// fp64 sums over a 256-thread workgroup in a fixed order: what the loss kernels (diffusion_train.hip, denoise_loss.hip) fold their thread sums with.
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
