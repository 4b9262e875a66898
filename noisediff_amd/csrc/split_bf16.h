// split_bf16.h -- the library's one three-term bf16 split: the arithmetic of every kernel that puts an fp32 product on the bf16 matrix pipe at the
// operands' FULL fp32 significand (pointwise.hip: the wide 1x1 layers; pwchain.hip: the fused per-pixel chains; small.hip: the 7x7 stem).
//
//   v = v1 + v2 + v3 exactly:  v1 = bf16(v), v2 = bf16(v - v1) (round-to-nearest-even, v_cvt_pk_bf16_f32), v3 = v - v1 - v2.  Both remainders are exact in
//   fp32 and the second has at most 8 significant bits, so the upper half of its fp32 pattern IS the third term.
//   Six of the nine term products of w . x are kept -- w1 x1, w1 x2, w2 x1, w2 x2, w1 x3, w3 x1 -- each one v_mfma_f32_32x32x16_bf16 (products of bf16 pairs
//   are exact in fp32; accumulation in fp32).  The dropped ones (w2 x3, w3 x2, w3 x3) are below 2^-25 of the product, under the rounding of an fp32 FMA.
//   16 channels of a 32 x 32 tile cost 6 x 32 matrix cycles against 8 x 64 on v_mfma_f32_32x32x2_f32 (2.67x), and -- unlike the fp32 instruction, which
//   issues on the VALU's own lanes -- the bf16 one leaves the vector ALU to the split, the prologues and the epilogues.
//
// Activations are split in the kernels (nd_split2_bf16, 11 VALU instructions per value pair), weights once at pack time (nd_split3_bf16): the "exact"
// claim holds because both are the SAME rule, stated here and nowhere else.  The units keep what is theirs: layouts, K-step slot maps, LDS plane geometry.
// Accuracy against fp64: profiles/r6_split_gemm_accuracy.txt (the r5 study of the same split on the F(4x4) kernel: rms error 0.94 of fp32's).
#pragma once
#include "nd_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));       // eight bf16 of one term: an MFMA operand
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// (x, y) -> one dword of each of the three bf16 terms (x in the low half): x == t1 + t2 + t3 exactly
__device__ __forceinline__ void nd_split2_bf16(float x, float y, unsigned& w1, unsigned& w2, unsigned& w3) {
    w1 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, y}, bf16x2));
    const float rx = x - __builtin_bit_cast(float, w1 << 16), ry = y - __builtin_bit_cast(float, w1 & 0xFFFF0000u);
    w2 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{rx, ry}, bf16x2));
    const float sx = rx - __builtin_bit_cast(float, w2 << 16), sy = ry - __builtin_bit_cast(float, w2 & 0xFFFF0000u);
    w3 = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, sy), __builtin_bit_cast(unsigned, sx), 0x07060302u);   // the upper halves ARE the third terms
}

// the same rule for one value, as the pack kernels store it: the 16-bit patterns of the three terms
struct bf16_terms { unsigned short t1, t2, t3; };
__device__ __forceinline__ bf16_terms nd_split3_bf16(float v) {
    const __bf16 t1 = (__bf16)v;
    const float r1 = v - (float)t1;                       // exact
    const __bf16 t2 = (__bf16)r1;
    const float r2 = r1 - (float)t2;                      // exact, at most 8 significant bits: its upper half is the third term
    return {__builtin_bit_cast(unsigned short, t1), __builtin_bit_cast(unsigned short, t2), (unsigned short)(__builtin_bit_cast(unsigned, r2) >> 16)};
}

// D(32x32) += A(32x16) * B(16x32) on bf16 terms; lane l gives eight consecutive K slots of row / column l & 31, K group l >> 5
__device__ __forceinline__ f32x16 nd_mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
