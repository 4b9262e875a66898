// philox_poisson.h -- the library's counter-based Poisson draw, shared by denoise_batch.hip (the shot-noise augmentation) and raw.hip (the
// Poisson-Gaussian training set).
//
// Philox4x32-10, key = the 64-bit seed, counter = {element index within the sample, global sample index, draw index, block j}; uniforms
// u = (word + 0.5) 2^-32 in fp64; every decision in fp64.
//   lam == 0: 0.   0 < lam < 10: inversion by sequential search on word 0 of block 0 (at most PO_INV_MAX steps).
//   lam >= 10: Hoermann's transformed rejection (PTRS, "The transformed rejection method for generating Poisson random variables", 1993);
//   attempt t takes words 2 (t mod 2), 2 (t mod 2) + 1 of block t / 2 (at most PO_MAX_ATTEMPTS; the chance to need more is below 1e-38).
//   lam negative, NaN or infinite: NaN.
// The draw stops at block PO_MAX_ATTEMPTS / 2 - 1 = 31: block 32 of the same counter is free for another variate of the same element.
#pragma once
#include "nd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PO_INV_MAX = 200;           // steps of the inversion search: P(k > 200 | lam < 10) = 0 in fp64; a bound for u above the rounded sum
constexpr int PO_MAX_ATTEMPTS = 64;       // rejection attempts: each accepts with probability > 0.75

__device__ __forceinline__ double po_uniform(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

// One Poisson(lam) count as a double.  elem / sample / draw are the counter words; see the head of the file.  Inlined: as a call it takes
// the calling convention's worst-case registers and spills to scratch.
__device__ __forceinline__ double philox_poisson(double lam, uint64_t seed, uint32_t elem, uint32_t sample, uint32_t draw) {
    if (!(lam > 0.0)) return lam == 0.0 ? 0.0 : __builtin_nan("");
    if (!(lam <= 1.7976931348623157e308)) return __builtin_nan("");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (lam < 10.0) {
        uint32_t c[4] = {elem, sample, draw, 0u};
        Philox::gen(c, k0, k1);
        const double u = po_uniform(c[0]);
        double p = exp(-lam), s = p, k = 0.0;
        while (u > s && k < (double)PO_INV_MAX) {
            k += 1.0;
            p *= lam / k;
            s += p;
        }
        return k;
    }
    const double sl = sqrt(lam), ll = log(lam);
    const double b = 0.931 + 2.53 * sl, a = -0.059 + 0.02483 * b;
    const double lia = log(1.1239 + 1.1328 / (b - 3.4)), vr = 0.9277 - 3.6224 / (b - 2.0);
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (int t = 0; t < PO_MAX_ATTEMPTS; ++t) {
        if ((t & 1) == 0) {
            c[0] = elem;  c[1] = sample;  c[2] = draw;  c[3] = (uint32_t)(t >> 1);
            Philox::gen(c, k0, k1);
        }
        const double U = po_uniform(c[2 * (t & 1)]) - 0.5, V = po_uniform(c[2 * (t & 1) + 1]);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        const double lhs = log(V) + lia - log(a / (us * us) + b);
        const double rhs = -lam + k * ll - lgamma(k + 1.0);
        if (lhs <= rhs) return k;
    }
    return __builtin_nan("");
}

}  // namespace
