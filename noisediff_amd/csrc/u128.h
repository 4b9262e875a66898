// u128.h -- what the exact integer variances of noise_level.hip (per level) and calibrate.hip (row means) end in: n sum q^2 - (sum q)^2 is formed
// in 128 bits and converted to fp64 ONCE.
#pragma once
#include "nd_common.h"

// Round to nearest even, once: the top 64 bits with everything below them folded into the last one, which lies under the rounding position.
__device__ __forceinline__ double nd_u128_to_double(unsigned __int128 v) {
    const unsigned long long hi = (unsigned long long)(v >> 64);
    if (hi == 0) return (double)(unsigned long long)v;
    const int sh = 64 - __builtin_clzll(hi);                                   // 1 .. 64
    unsigned long long top = (unsigned long long)(v >> sh);
    const unsigned __int128 below = sh == 64 ? (unsigned __int128)(unsigned long long)v : (v & (((unsigned __int128)1 << sh) - 1));
    top |= (unsigned long long)(below != 0);
    return ldexp((double)top, sh);
}
