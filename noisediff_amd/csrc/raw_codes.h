// What raw.hip, develop.hip and frame.hip share: reading and writing the codes of Bayer cells in a uint16 frame, the code a packed fp32 value is
// written as, and the choice of how many packed columns a thread takes.
#pragma once
#include "nd_common.h"
#include <type_traits>

#pragma clang fp contract(off)      // file scope: holds for the rest of the including source as well, and the sources ask for it themselves

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

template <int V>
__device__ __forceinline__ void rw_store_pairs(uint16_t* p, const uint32_t (&r)[V]) {      // p is 4 V-byte aligned: checked on the host
    if constexpr (V == 4) *reinterpret_cast<uint4*>(p) = uint4{r[0], r[1], r[2], r[3]};
    else if constexpr (V == 2) *reinterpret_cast<uint2*>(p) = uint2{r[0], r[1]};
    else *reinterpret_cast<uint32_t*>(p) = r[0];
}

// channel c of a Bayer cell given its two words (row 2Y, row 2Y+1)
__device__ __forceinline__ float rw_code(uint32_t top, uint32_t bottom, int c) {
    const uint32_t wd = c < 2 ? top : bottom;
    return (float)((c == 1 || c == 2) ? (wd >> 16) : (wd & 0xFFFFu));
}

// nd_raw_to_bayer_u16's rule for one value: trunc((double)clip(x, 0, 1) * (white - bl) + bl), NaN -> 0
__device__ __forceinline__ uint32_t rw_to_code(float x, int bl, int white) {
    if (!(x == x)) return 0u;
    const float p = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    const double t = (double)p * (double)(white - bl) + (double)bl;
    return (uint32_t)t;
}

// the widest V with w % V == 0 and every pointer of `bits` 4 V-byte aligned
static inline int rw_width(int w, uintptr_t bits) {
    if (w % 4 == 0 && (bits & 15u) == 0) return 4;
    if (w % 2 == 0 && (bits & 7u) == 0) return 2;
    return 1;
}

// launch(std::integral_constant<int, V>) for V = 4, 2 or 1: the one place a width chosen at run time becomes a kernel's template argument
template <class F>
static inline void rw_dispatch(int V, F launch) {
    if (V == 4) launch(std::integral_constant<int, 4>());
    else if (V == 2) launch(std::integral_constant<int, 2>());
    else launch(std::integral_constant<int, 1>());
}
