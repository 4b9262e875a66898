// philox_normal.h -- the library's counter-based normal draw, shared by sampler.hip (x_T and the per-step noise of the reverse chain) and
// diffusion_train.hip (the training step's element noise and offset noise).
//
// Philox4x32-10, key = the 64-bit seed, counter = {index, global sample index, draw index, block}; the four words of one block become four
// N(0,1) by two Box-Muller pairs on u = (word + 0.5) 2^-32 in fp32 (restated in fp64 by oracle/noisediff_oracle.py::philox_normal4).
//   block 0: the sampler.  index = quad q of the sample's elements in NHWC order, draw = 0 for x_T and i + 1 for the i-th step.
//   blocks 1-3: the training step, see diffusion_train.hip.
#pragma once
#include "nd_common.h"

namespace {

// four N(0,1) for quad `q` of sample `sample` at noise draw `step1` (0 = x_T, i+1 = i-th step)
__device__ __forceinline__ f32x4 philox_normal4(uint64_t seed, uint32_t sample, uint32_t step1, uint32_t q, uint32_t block = 0u) {
    uint32_t c[4] = {q, sample, step1, block};
    Philox::gen(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float k = 1.0f / 4294967296.0f;
    const float u0 = ((float)c[0] + 0.5f) * k, u1 = ((float)c[1] + 0.5f) * k;
    const float u2 = ((float)c[2] + 0.5f) * k, u3 = ((float)c[3] + 0.5f) * k;
    const float r0 = sqrtf(-2.0f * logf(fminf(u0, 1.0f))), r1 = sqrtf(-2.0f * logf(fminf(u2, 1.0f)));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0);
    sincosf(6.283185307179586f * u3, &s1, &c1);
    return (f32x4){r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

}  // namespace
