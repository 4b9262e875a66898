// wino2x2.h -- the transforms of Winograd F(2x2, 3x3) (Lavin & Gray) as constexpr tables, shared by conv3x3_wino.hip and conv3x3_wino2.hip
// (tests/conv3x3_ref.py restates them as its m = 2).  The F(4x4) kernels' transforms are written per kernel on purpose and are not here.
#pragma once
#include "nd_common.h"

// B^T rows as (index, sign) pairs: xi -> s1*d[r1] + s2*d[r2]
__device__ __forceinline__ constexpr int bt_r1(int xi) { return xi == 0 ? 0 : 1; }
__device__ __forceinline__ constexpr int bt_r2(int xi) { return xi == 3 ? 3 : 2; }
__device__ __forceinline__ constexpr float bt_s1(int xi) { return xi == 2 ? -1.0f : 1.0f; }
__device__ __forceinline__ constexpr float bt_s2(int xi) { return (xi == 0 || xi == 3) ? -1.0f : 1.0f; }
// A^T[a][xi]
__device__ __forceinline__ constexpr int at_coef(int a, int xi) {
    return a == 0 ? (xi <= 2 ? 1 : 0) : (xi == 0 ? 0 : (xi == 1 ? 1 : -1));
}
