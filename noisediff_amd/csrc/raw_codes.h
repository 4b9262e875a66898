// What raw.hip and develop.hip share: reading the codes of Bayer cells from a uint16 frame, and the code a packed fp32 value is written as.
#pragma once
#include "nd_common.h"

#pragma clang fp contract(off)      // file scope: holds for the rest of the including source as well, and both sources ask for it themselves

// 2 V codes from p (4-byte aligned at least) as V words: the even Bayer column in the low half, the odd one in the high half
template <int V>
__device__ __forceinline__ void rw_load_pairs(const uint16_t* p, uint32_t (&r)[V]) {
    static_assert(V == 1 || V == 2 || V == 4, "one, two or four packed columns per thread");
    const uintptr_t a = (uintptr_t)p;
    if constexpr (V == 4) {
        if ((a & 15u) == 0) {
            const uint4 t = *reinterpret_cast<const uint4*>(p);
            r[0] = t.x;  r[1] = t.y;  r[2] = t.z;  r[3] = t.w;
            return;
        }
    }
    if constexpr (V >= 2) {
        if ((a & 7u) == 0) {
#pragma unroll
            for (int i = 0; i < V; i += 2) {
                const uint2 t = *reinterpret_cast<const uint2*>(p + 2 * i);
                r[i] = t.x;  r[i + 1] = t.y;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = *reinterpret_cast<const uint32_t*>(p + 2 * i);
}

// nd_raw_to_bayer_u16's rule for one value: trunc((double)clip(x, 0, 1) * (white - bl) + bl), NaN -> 0
__device__ __forceinline__ uint32_t rw_to_code(float x, int bl, int white) {
    if (!(x == x)) return 0u;
    const float p = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    const double t = (double)p * (double)(white - bl) + (double)bl;
    return (uint32_t)t;
}
