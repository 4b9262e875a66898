// attn_train.hip -- the backward passes of the attention modules (models/archs/Diffusion_arch.py:84-90, 198-266; models/attend.py:101-116):
// full attention, LinearAttention and RMSNorm, fp32, fixed summation order, no atomics.  The forwards are attention.hip (with the LSE output),
// linattn.hip and norm.hip.  Tensors are NHWC: qkv / dqkv [B][N][q | k | v thirds of heads * 32], out / dout [B][N][heads * 32].
//
// Full attention, flash-style: P = exp(S - lse) is recomputed per 32 x 32 tile on the exact-fp32 matrix pipe, no N x N tensor in memory.
//   delta_i = sum_d dO_i O_i                                                      (attn_delta_kernel, into the workspace)
//   dV = P^T dO,  dP = dO V^T,  dS = P (.) (dP - delta),  dK = scale dS^T Q        (attn_bwd_dkv_kernel: a wave owns 32 KEYS and walks the queries)
//   dQ = scale dS K                                                                (attn_bwd_dq_kernel:  a wave owns 32 QUERIES and walks the keys)
// In both passes the owned index sits on the lane column and the walked one on the accumulator rows, so S and dP leave the matrix pipe as the
// B operand of the products that follow (register r of lane half h is row (r&3)+8(r>>2)+4h: one k-step) and never move through LDS.  S is the
// forward's own instruction sequence (q pre-scaled, the same k-step order), so P sums to the forward's l bit for bit.
//
// LinearAttention: q~ = softmax_d(q), k^ = softmax_n(k), ctx = k^ v^T, out = s ctx^T q~ (s = dh^-1/2).  Two passes over N:
//   1. dctx[d][e] = s sum_n q~[d][n] dout[e][n]: per-chunk partials (la_dctx_kernel), then ctx, dctx and r[d] = sum_e dctx ctx reduced over the
//      chunks in chunk order (la_bwd_finalize_kernel);
//   2. per 32 pixels (la_bwd_kernel): dq = q~ (.) (t - sum_d q~ t), t = s ctx dout;  dv = dctx^T k^;  dk = k^ (.) (dctx v - r) -- the softmax over N
//      needs no pass of its own: sum_n k^ (dctx v) = sum_e dctx ctx.
//
// RMSNorm: y = x / max(|x|, 1e-12) * g * sqrt(C), the norm recomputed from x; dg in two stages (per-workgroup partials, then fp64 in fixed order).
#include "nd_common.h"

namespace {

constexpr int DH = 32, LDP = DH + 4, TILE = 64;

__device__ __forceinline__ void nd_st_acc(float* p, const f32x16& a, int half, float mul) {      // accumulator rows of this lane -> 4 quads of a 32-float row
#pragma unroll
    for (int g = 0; g < 4; ++g) nd_st4(p + 8 * g + 4 * half, f32x4{a[4 * g] * mul, a[4 * g + 1] * mul, a[4 * g + 2] * mul, a[4 * g + 3] * mul});
}

// ------------------------------------------------------------------------------------------------------------------ full attention
// delta[b][h][i] = sum_d dout[b][i][h][d] * out[b][i][h][d]; one thread per (token, head), head fastest
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ out, int ldo, const float* __restrict__ dout, int ldd,
                                                         float* __restrict__ delta, int N, int heads, size_t total) {
    const size_t idx = blockIdx.x * (size_t)256 + threadIdx.x;
    if (idx >= total) return;
    const int h = (int)(idx % heads);
    const size_t tok = idx / heads, b = tok / N, i = tok % N;
    const float* o = out + tok * ldo + h * DH;
    const float* d = dout + tok * ldd + h * DH;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4 a = nd_ld4(o + 4 * j), c = nd_ld4(d + 4 * j);
        s += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
    }
    delta[(b * heads + h) * N + i] = s;
}

// dK, dV: one workgroup = 4 waves = 128 keys of one (sample, head); each wave keeps dK^T and dV^T of its 32 keys in 32 accumulator registers
// while the workgroup walks the queries in staged tiles of 64 (Q pre-scaled, dO; lse and delta of the tile next to them).
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ dout, int ldd,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           float* __restrict__ dqkv, int ldg, int N, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Qs[TILE * LDP];
    __shared__ __attribute__((aligned(16))) float Ds[TILE * LDP];
    __shared__ float Ls[TILE], Dl[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int kt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int hid = heads * DH;
    const float* base = qkv + (size_t)b * N * ldq;
    const float* dbase = dout + (size_t)b * N * ldd;
    const float* lse_b = lse + ((size_t)b * heads + h) * N;
    const float* del_b = delta + ((size_t)b * heads + h) * N;
    const int key = kt * 128 + wave * 32 + col;          // this lane's key
    const bool kvalid = key < N;
    float kf[16], vf[16];                                // lane (key, half) holds k[16*half + s], v[16*half + s]
    {
        const float* kp = base + (size_t)(kvalid ? key : 0) * ldq + hid + h * DH + 16 * half;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 k4 = kvalid ? nd_ld4(kp + 4 * j) : (f32x4){0, 0, 0, 0};
            const f32x4 v4 = kvalid ? nd_ld4(kp + hid + 4 * j) : (f32x4){0, 0, 0, 0};
            kf[4 * j] = k4.x; kf[4 * j + 1] = k4.y; kf[4 * j + 2] = k4.z; kf[4 * j + 3] = k4.w;
            vf[4 * j] = v4.x; vf[4 * j + 1] = v4.y; vf[4 * j + 2] = v4.z; vf[4 * j + 3] = v4.w;
        }
    }
    f32x16 dk = nd_zero16(), dv = nd_zero16();

    for (int q0 = 0; q0 < N; q0 += TILE) {
        __syncthreads();
        // stage Q * scale and dO: 64 queries x 32 floats each = 512 quads per tensor, 256 threads x 2; rows past N: zeros, lse = +inf (P = 0)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * 256, qr = idx >> 3, q4 = (idx & 7) * 4;
            f32x4 qv = {0, 0, 0, 0}, gv = {0, 0, 0, 0};
            if (q0 + qr < N) {
                qv = nd_ld4(base + (size_t)(q0 + qr) * ldq + h * DH + q4) * scale;
                gv = nd_ld4(dbase + (size_t)(q0 + qr) * ldd + h * DH + q4);
            }
            nd_st4(&Qs[qr * LDP + q4], qv);
            nd_st4(&Ds[qr * LDP + q4], gv);
        }
        if (tid < TILE) {
            const bool ok = q0 + tid < N;
            Ls[tid] = ok ? lse_b[q0 + tid] : INFINITY;
            Dl[tid] = ok ? del_b[q0 + tid] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < TILE / 32; ++sub) {
            if (q0 + sub * 32 >= N) break;
            // S and dP tiles: rows = queries, cols = keys
            f32x16 s = nd_zero16(), dp = nd_zero16();
            const float* qp = &Qs[(sub * 32 + col) * LDP + 16 * half];
            const float* gp = &Ds[(sub * 32 + col) * LDP + 16 * half];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 q4 = nd_ld4(qp + 4 * j);
                s = nd_mfma(q4.x, kf[4 * j], s);
                s = nd_mfma(q4.y, kf[4 * j + 1], s);
                s = nd_mfma(q4.z, kf[4 * j + 2], s);
                s = nd_mfma(q4.w, kf[4 * j + 3], s);
                const f32x4 g4 = nd_ld4(gp + 4 * j);
                dp = nd_mfma(g4.x, vf[4 * j], dp);
                dp = nd_mfma(g4.y, vf[4 * j + 1], dp);
                dp = nd_mfma(g4.z, vf[4 * j + 2], dp);
                dp = nd_mfma(g4.w, vf[4 * j + 3], dp);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = sub * 32 + nd_acc_row(r, lane);
                s[r] = __expf(s[r] - Ls[qr]);                    // P
                dp[r] = s[r] * (dp[r] - Dl[qr]);                 // dS
            }
            // dV^T[dh][key] += dO^T[dh][query] P[query][key]; dK^T[dh][key] += (scale Q)^T[dh][query] dS[query][key]; k-step r pairs queries row(r,0), row(r,1)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = sub * 32 + nd_acc_row(r, lane);
                dv = nd_mfma(Ds[qr * LDP + col], s[r], dv);
                dk = nd_mfma(Qs[qr * LDP + col], dp[r], dk);
            }
        }
    }
    if (kvalid) {
        float* gp = dqkv + ((size_t)b * N + key) * ldg + hid + h * DH;
        nd_st_acc(gp, dk, half, 1.0f);
        nd_st_acc(gp + hid, dv, half, 1.0f);
    }
}

// dQ: one workgroup = 4 waves = 128 queries of one (sample, head), the forward's shape: each wave owns 32 queries and walks the keys in staged tiles of 64.
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ dout, int ldd,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ dqkv, int ldg, int N, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) float Ks[TILE * LDP];
    __shared__ __attribute__((aligned(16))) float Vs[TILE * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int hid = heads * DH;
    const float* base = qkv + (size_t)b * N * ldq;
    const int qi = qt * 128 + wave * 32 + col;          // this lane's query
    const bool qvalid = qi < N;
    float qf[16], gf[16];                               // lane (query, half) holds scale * q[16*half + s], dO[16*half + s]
    {
        const float* qp = base + (size_t)(qvalid ? qi : 0) * ldq + h * DH + 16 * half;
        const float* gp = dout + ((size_t)b * N + (qvalid ? qi : 0)) * ldd + h * DH + 16 * half;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 q4 = qvalid ? nd_ld4(qp + 4 * j) : (f32x4){0, 0, 0, 0};
            const f32x4 g4 = qvalid ? nd_ld4(gp + 4 * j) : (f32x4){0, 0, 0, 0};
            qf[4 * j] = q4.x * scale; qf[4 * j + 1] = q4.y * scale; qf[4 * j + 2] = q4.z * scale; qf[4 * j + 3] = q4.w * scale;
            gf[4 * j] = g4.x; gf[4 * j + 1] = g4.y; gf[4 * j + 2] = g4.z; gf[4 * j + 3] = g4.w;
        }
    }
    const float lse_i = qvalid ? lse[((size_t)b * heads + h) * N + qi] : 0.0f;
    const float del_i = qvalid ? delta[((size_t)b * heads + h) * N + qi] : 0.0f;
    f32x16 dq = nd_zero16();

    for (int k0 = 0; k0 < N; k0 += TILE) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * 256, kr = idx >> 3, q4 = (idx & 7) * 4;
            f32x4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
            if (k0 + kr < N) {
                const float* rp = base + (size_t)(k0 + kr) * ldq + h * DH + q4;
                kv = nd_ld4(rp + hid);
                vv = nd_ld4(rp + 2 * hid);
            }
            nd_st4(&Ks[kr * LDP + q4], kv);
            nd_st4(&Vs[kr * LDP + q4], vv);
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < TILE / 32; ++sub) {
            if (k0 + sub * 32 >= N) break;
            // S^T and dP^T tiles: rows = keys, cols = queries
            f32x16 st = nd_zero16(), dp = nd_zero16();
            const float* kp = &Ks[(sub * 32 + col) * LDP + 16 * half];
            const float* vp = &Vs[(sub * 32 + col) * LDP + 16 * half];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 k4 = nd_ld4(kp + 4 * j);
                st = nd_mfma(k4.x, qf[4 * j], st);
                st = nd_mfma(k4.y, qf[4 * j + 1], st);
                st = nd_mfma(k4.z, qf[4 * j + 2], st);
                st = nd_mfma(k4.w, qf[4 * j + 3], st);
                const f32x4 v4 = nd_ld4(vp + 4 * j);
                dp = nd_mfma(v4.x, gf[4 * j], dp);
                dp = nd_mfma(v4.y, gf[4 * j + 1], dp);
                dp = nd_mfma(v4.z, gf[4 * j + 2], dp);
                dp = nd_mfma(v4.w, gf[4 * j + 3], dp);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kr = k0 + sub * 32 + nd_acc_row(r, lane);
                const float p = kr < N ? __expf(st[r] - lse_i) : 0.0f;
                dp[r] = p * (dp[r] - del_i);                     // dS^T
            }
            // dQ^T[dh][query] += K^T[dh][key] dS^T[key][query]; k-step r pairs keys row(r,0), row(r,1)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq = nd_mfma(Ks[(sub * 32 + nd_acc_row(r, lane)) * LDP + col], dp[r], dq);
        }
    }
    if (qvalid) nd_st_acc(dqkv + ((size_t)b * N + qi) * ldg + h * DH, dq, half, scale);
}

// ------------------------------------------------------------------------------------------------------------------ LinearAttention
constexpr int CHUNK = ND_LA_CHUNK;                  // pixels per partial workgroup: the forward's chunks (linattn.hip), whose partials this file reads
constexpr int LA_FIN = 2 * DH * DH + DH;            // per (sample, head): ctx, dctx, r

// 1. dpart[b][h][chunk][d][e] = s sum_{n in chunk} softmax_d(q)[n][d] dout[n][e].  A wave softmaxes 32 pixels with the pixel on the lane, hands the
//    tile to the matrix pipe through its own LDS block (the product runs over the pixels), and the four waves meet in LDS in wave order.
__global__ __launch_bounds__(256) void la_dctx_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ dout, int ldd,
                                                      float* __restrict__ dpart, int N, int heads, int chunks, float scale) {
    __shared__ float qs[4][32 * 33];
    __shared__ float red[4][DH * DH];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int n_begin = c * CHUNK, n_end = min(N, n_begin + CHUNK);
    const float* gb = dout + (size_t)b * N * ldd + h * DH + col;
    f32x16 acc = nd_zero16();
    for (int g0 = n_begin; g0 < n_end; g0 += 128) {          // (the trip count is the workgroup's: the barriers are reached by every wave)
        const int nb = g0 + wave * 32, n = nb + col;
        const bool ok = n < n_end;
        const float* qp = qkv + ((size_t)b * N + (ok ? n : n_begin)) * ldq + h * DH + 16 * half;
        float q[16];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = nd_ld4(qp + 4 * j);
            q[4 * j] = v.x; q[4 * j + 1] = v.y; q[4 * j + 2] = v.z; q[4 * j + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) mx = fmaxf(mx, q[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) { q[j] = __expf(q[j] - mx); sum += q[j]; }
        sum += __shfl_xor(sum, 32);
        const float norm = ok ? scale / sum : 0.0f;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) qs[wave][col * 33 + 16 * half + j] = q[j] * norm;
        __syncthreads();
        if (nb < n_end) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {                   // k-step j pairs pixels nb + 2j (half 0) and nb + 2j + 1 (half 1)
                const int p = nb + 2 * j + half;
                const float gv = p < n_end ? gb[(size_t)p * ldd] : 0.0f;
                acc = nd_mfma(qs[wave][(2 * j + half) * 33 + col], gv, acc);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][nd_acc_row(r, lane) * DH + col] = acc[r];
    __syncthreads();
    float* o = dpart + (((size_t)b * heads + h) * chunks + c) * DH * DH;
    for (int i = tid; i < DH * DH; i += 256) o[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// fin[b][h] = {ctx[d][e], dctx[d][e], r[d] = sum_e dctx[d][e] ctx[d][e]}: the chunks in chunk order (ctx as the forward's output kernel sums it)
__global__ __launch_bounds__(256) void la_bwd_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ dpart, float* __restrict__ fin,
                                                              int heads, int chunks) {
    __shared__ float prod[DH * DH];
    const size_t bh = (size_t)blockIdx.y * heads + blockIdx.x;
    const int tid = threadIdx.x;
    const float* pa = partial + bh * chunks * DH * DH;
    const float* pd = dpart + bh * chunks * DH * DH;
    float* o = fin + bh * LA_FIN;
    for (int i = tid; i < DH * DH; i += 256) {
        float s = 0.0f, t = 0.0f;
        for (int c = 0; c < chunks; ++c) { s += pa[(size_t)c * DH * DH + i]; t += pd[(size_t)c * DH * DH + i]; }
        o[i] = s;
        o[DH * DH + i] = t;
        prod[i] = s * t;
    }
    __syncthreads();
    if (tid < DH) {
        float r = 0.0f;
        for (int e = 0; e < DH; ++e) r += prod[tid * DH + e];
        o[2 * DH * DH + tid] = r;
    }
}

// 2. dq, dk, dv of 32 pixels per wave, the pixel on the lane column; the three products put d (or e) on the accumulator rows, so a pixel's softmax
//    sums are a register reduction plus one cross-half shuffle and a lane's results are four quads of its pixel's row.
__global__ __launch_bounds__(256) void la_bwd_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ dout, int ldd,
                                                     const float* __restrict__ kstat, const float* __restrict__ fin, float* __restrict__ dqkv, int ldg,
                                                     int N, int heads, float scale) {
    __shared__ float ctx[DH * 33], dctx[DH * 33], rr[DH], kmx[DH], kin[DH];
    const int h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int hid = heads * DH;
    const float* f = fin + ((size_t)b * heads + h) * LA_FIN;
    for (int i = tid; i < DH * DH; i += 256) {
        ctx[(i / DH) * 33 + (i % DH)] = f[i];
        dctx[(i / DH) * 33 + (i % DH)] = f[DH * DH + i];
    }
    if (tid < DH) {
        const float* ks = kstat + (((size_t)b * heads + h) * DH + tid) * 2;
        rr[tid] = f[2 * DH * DH + tid];
        kmx[tid] = ks[0];
        kin[tid] = 1.0f / ks[1];
    }
    __syncthreads();
    const int n = (blockIdx.x * 4 + wave) * 32 + col;
    const bool ok = n < N;
    const size_t tok = (size_t)b * N + (ok ? n : 0);
    const float* qp = qkv + tok * ldq + h * DH;
    const float* gp = dout + tok * ldd + h * DH;
    // B operands: this pixel's dout, k^ and v at channels 16*half + j (k-step j pairs channels j and 16 + j)
    float g16[16], k16[16], v16[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 g4 = nd_ld4(gp + 16 * half + 4 * j), k4 = nd_ld4(qp + hid + 16 * half + 4 * j), v4 = nd_ld4(qp + 2 * hid + 16 * half + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 16 * half + 4 * j + e;
            g16[4 * j + e] = g4[e];
            k16[4 * j + e] = __expf(k4[e] - kmx[d]) * kin[d];
            v16[4 * j + e] = v4[e];
        }
    }
    f32x16 t = nd_zero16(), dv = nd_zero16(), u = nd_zero16();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int d = 16 * half + j;
        t = nd_mfma(ctx[col * 33 + d], g16[j], t);           // t^T[d][n]  = sum_e ctx[d][e] dout[n][e]
        dv = nd_mfma(dctx[d * 33 + col], k16[j], dv);        // dv^T[e][n] = sum_d dctx[d][e] k^[n][d]
        u = nd_mfma(dctx[col * 33 + d], v16[j], u);          // u^T[d][n]  = sum_e dctx[d][e] v[n][e]
    }
    // q~ and k^ of this pixel at the accumulator's channels: d = 8g + 4*half + (0..3) for registers 4g .. 4g+3
    float qs[16], kh[16];
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d0 = 8 * g + 4 * half;
        const f32x4 q4 = nd_ld4(qp + d0), k4 = nd_ld4(qp + hid + d0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qs[4 * g + e] = q4[e];
            kh[4 * g + e] = __expf(k4[e] - kmx[d0 + e]) * kin[d0 + e];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, qs[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { qs[r] = __expf(qs[r] - mx); sum += qs[r]; }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    float dot = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { qs[r] *= inv; t[r] *= scale; dot += qs[r] * t[r]; }
    dot += __shfl_xor(dot, 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        t[r] = qs[r] * (t[r] - dot);                                  // dq
        u[r] = kh[r] * (u[r] - rr[nd_acc_row(r, lane)]);              // dk
    }
    if (ok) {
        float* op = dqkv + tok * ldg + h * DH;
        nd_st_acc(op, t, half, 1.0f);
        nd_st_acc(op + hid, u, half, 1.0f);
        nd_st_acc(op + 2 * hid, dv, half, 1.0f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ RMSNorm
constexpr int RMS_WGS = 1024;                       // fixed: the summation order of dg must not depend on the device
constexpr int RMS_MAXQ = 4;                         // quads of a row per lane: C <= 1024

// dx of the pixels of this workgroup (one wave per pixel, the row in registers) and the workgroup's partial of dg.  xh = x / max(|x|, eps):
//   |x| >= eps:  dx = sqrt(C) / |x| * (a - xh (xh . a)),  a = g (.) dy;     |x| < eps: the norm is the constant eps, dx = sqrt(C) / eps * a
// (what autograd gives F.normalize: clamp_min passes no gradient below eps);  dg[c] = sum_pixels dy[c] xh[c] sqrt(C).
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                          const float* __restrict__ g, float* __restrict__ dx, int lddx, float* __restrict__ part,
                                                          long npix, int C, long rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float red[4][1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float rootc = sqrtf((float)C);
    f32x4 gm[RMS_MAXQ], dg[RMS_MAXQ];
#pragma unroll
    for (int k = 0; k < RMS_MAXQ; ++k) {
        dg[k] = f32x4{0, 0, 0, 0};
        gm[k] = f32x4{0, 0, 0, 0};
        if (lane * 4 + 256 * k < C) gm[k] = nd_ld4(g + lane * 4 + 256 * k);
    }
    const long r_begin = (long)blockIdx.x * rows_per_wg, r_end = min(r_begin + rows_per_wg, npix);
    for (long p = r_begin + wave; p < r_end; p += 4) {
        f32x4 xv[RMS_MAXQ], a[RMS_MAXQ];
        float ssq = 0.0f;
#pragma unroll
        for (int k = 0; k < RMS_MAXQ; ++k) {
            xv[k] = f32x4{0, 0, 0, 0};
            a[k] = f32x4{0, 0, 0, 0};
            if (lane * 4 + 256 * k < C) {
                xv[k] = nd_ld4(x + (size_t)p * ldx + lane * 4 + 256 * k);
                a[k] = nd_ld4(dy + (size_t)p * lddy + lane * 4 + 256 * k);
                ssq += xv[k].x * xv[k].x + xv[k].y * xv[k].y + xv[k].z * xv[k].z + xv[k].w * xv[k].w;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ssq += __shfl_xor(ssq, o);
        const float nrm = sqrtf(ssq);
        const float invn = 1.0f / fmaxf(nrm, 1e-12f);
        float proj = 0.0f;
#pragma unroll
        for (int k = 0; k < RMS_MAXQ; ++k) {
            xv[k] = xv[k] * invn;                                        // xh
            dg[k] += a[k] * xv[k] * rootc;
            a[k] = a[k] * gm[k];
            const f32x4 pa = a[k] * xv[k];
            proj += pa.x + pa.y + pa.z + pa.w;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) proj += __shfl_xor(proj, o);
        if (!(nrm >= 1e-12f)) proj = 0.0f;
        const float sc = rootc * invn;
#pragma unroll
        for (int k = 0; k < RMS_MAXQ; ++k)
            if (lane * 4 + 256 * k < C) nd_st4(dx + (size_t)p * lddx + lane * 4 + 256 * k, (a[k] - xv[k] * proj) * sc);
    }
    // the workgroup's column sums: the four waves meet in LDS in wave order
#pragma unroll
    for (int k = 0; k < RMS_MAXQ; ++k) nd_st4(&red[wave][lane * 4 + 256 * k], dg[k]);
    __syncthreads();
    float* o = part + (size_t)blockIdx.x * C;
    for (int c = tid; c < C; c += 256) o[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// dg[c] = sum over the workgroups' partials: 32 channels per workgroup, eight stripes (w = stripe, stripe + 8, ...) that meet in stripe order, fp64
__global__ __launch_bounds__(256) void rmsnorm_dg_kernel(const float* __restrict__ part, float* __restrict__ dg, int wgs, int C) {
    __shared__ double red[8][32];
    const int o = threadIdx.x & 31, stripe = threadIdx.x >> 5, c = blockIdx.x * 32 + o;
    double s = 0.0;
    if (c < C)
        for (int w = stripe; w < wgs; w += 8) s += (double)part[(size_t)w * C + c];
    red[stripe][o] = s;
    __syncthreads();
    if (stripe == 0 && c < C) {
#pragma unroll
        for (int k = 1; k < 8; ++k) s += red[k][o];
        dg[c] = (float)s;
    }
}

inline bool attn_strides_ok(int heads, int dh, int ld_qkv, int ld_out, int ld_dout, int ld_dqkv) {
    return ld_qkv >= 3 * heads * dh && ld_dqkv >= 3 * heads * dh && ld_out >= heads * dh && ld_dout >= heads * dh && ld_qkv % 4 == 0 && ld_out % 4 == 0 &&
           ld_dout % 4 == 0 && ld_dqkv % 4 == 0;
}

}  // namespace

extern "C" int64_t nd_attention_backward_workspace_floats(int B, int N, int heads) {
    if (B <= 0 || N <= 0 || heads <= 0) return ND_E_BADARG;
    return (int64_t)B * heads * N;
}

extern "C" int nd_attention_backward_f32(const float* qkv, int ld_qkv, const float* out, int ld_out, const float* dout, int ld_dout, const float* lse,
                                         float* dqkv, int ld_dqkv, float* workspace, int B, int N, int heads, int dh, void* stream) {
    ND_REQUIRE(qkv && out && dout && lse && dqkv && workspace, ND_E_BADARG, "nd_attention_backward: null pointer");
    ND_REQUIRE(B > 0 && N > 0 && heads > 0, ND_E_BADARG, "nd_attention_backward: non-positive size");
    ND_REQUIRE(dh == DH, ND_E_SHAPE, "nd_attention_backward: dim_head=%d (only 32 is built)", dh);
    ND_REQUIRE(attn_strides_ok(heads, dh, ld_qkv, ld_out, ld_dout, ld_dqkv), ND_E_SHAPE, "nd_attention_backward: strides (multiples of 4 floats that hold a row)");
    ND_REQUIRE(nd_aligned16(qkv) && nd_aligned16(out) && nd_aligned16(dout) && nd_aligned16(dqkv), ND_E_ALIGN, "nd_attention_backward: alignment");
    ND_REQUIRE(B <= 65535 && heads <= 65535 && (int64_t)B * N * heads < ((int64_t)1 << 38), ND_E_SHAPE,
               "nd_attention_backward: grid too large (B, heads <= 65535; B * N * heads < 2^38: one thread per (token, head) in the delta pass)");
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.0f / sqrtf((float)dh);
    const size_t total = (size_t)B * N * heads;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, ld_out, dout, ld_dout, workspace, N, heads, total);
    const dim3 grid(nd_cdiv(N, 128), heads, B);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), 0, st, qkv, ld_qkv, dout, ld_dout, lse, workspace, dqkv, ld_dqkv, N, heads, scale);
    hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), 0, st, qkv, ld_qkv, dout, ld_dout, lse, workspace, dqkv, ld_dqkv, N, heads, scale);
    return nd_launch_status("nd_attention_backward_f32");
}

extern "C" int64_t nd_linear_attention_backward_workspace_floats(int B, int N, int heads) {
    if (B <= 0 || N <= 0 || heads <= 0) return ND_E_BADARG;
    return (int64_t)B * heads * ((int64_t)nd_cdiv(N, CHUNK) * DH * DH + LA_FIN);
}

extern "C" int nd_linear_attention_backward_f32(const float* qkv, int ld_qkv, const float* dout, int ld_dout, const float* fwd_workspace, float* dqkv,
                                                int ld_dqkv, float* workspace, int B, int N, int heads, int dh, void* stream) {
    ND_REQUIRE(qkv && dout && fwd_workspace && dqkv && workspace, ND_E_BADARG, "nd_linear_attention_backward: null pointer");
    ND_REQUIRE(B > 0 && N > 0 && heads > 0, ND_E_BADARG, "nd_linear_attention_backward: non-positive size");
    ND_REQUIRE(dh == DH, ND_E_SHAPE, "nd_linear_attention_backward: dim_head=%d (only 32 is built)", dh);
    ND_REQUIRE(attn_strides_ok(heads, dh, ld_qkv, ld_dout, ld_dout, ld_dqkv), ND_E_SHAPE,
               "nd_linear_attention_backward: strides (multiples of 4 floats that hold a row)");
    ND_REQUIRE(nd_aligned16(qkv) && nd_aligned16(dout) && nd_aligned16(dqkv), ND_E_ALIGN, "nd_linear_attention_backward: alignment");
    ND_REQUIRE(B <= 65535 && heads <= 65535, ND_E_SHAPE, "nd_linear_attention_backward: grid too large");
    const int chunks = nd_cdiv(N, CHUNK);
    const float* kstat = fwd_workspace;
    const float* partial = fwd_workspace + (size_t)B * heads * DH * 2;
    float* dpart = workspace;
    float* fin = workspace + (size_t)B * heads * chunks * DH * DH;
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.0f / sqrtf((float)dh);
    hipLaunchKernelGGL(la_dctx_kernel, dim3(chunks, heads, B), dim3(256), 0, st, qkv, ld_qkv, dout, ld_dout, dpart, N, heads, chunks, scale);
    hipLaunchKernelGGL(la_bwd_finalize_kernel, dim3(heads, B), dim3(256), 0, st, partial, dpart, fin, heads, chunks);
    hipLaunchKernelGGL(la_bwd_kernel, dim3(nd_cdiv(N, 128), heads, B), dim3(256), 0, st, qkv, ld_qkv, dout, ld_dout, kstat, fin, dqkv, ld_dqkv, N, heads,
                       scale);
    return nd_launch_status("nd_linear_attention_backward_f32");
}

extern "C" int64_t nd_rmsnorm_backward_workspace_floats(int64_t npix, int C) { return npix > 0 && C > 0 ? (int64_t)RMS_WGS * C : -1; }

// What the RMSNorm backward takes: a row's quads over 64 lanes, at most RMS_MAXQ per lane.
extern "C" int nd_rmsnorm_train_takes(int C) { return C > 0 && C % 4 == 0 && C <= 256 * RMS_MAXQ; }

extern "C" int nd_rmsnorm_backward_f32(const float* dy, int lddy, const float* x, int ldx, const float* g, float* dx, int lddx, float* dg, float* workspace,
                                       int B, int HW, int C, void* stream) {
    ND_REQUIRE(dy && x && g && dx && dg && workspace, ND_E_BADARG, "nd_rmsnorm_backward: null pointer");
    ND_REQUIRE(B > 0 && HW > 0, ND_E_BADARG, "nd_rmsnorm_backward: non-positive size");
    ND_REQUIRE(nd_rmsnorm_train_takes(C), ND_E_SHAPE, "nd_rmsnorm_backward: C=%d (a multiple of 4 up to 1024)", C);
    ND_REQUIRE(lddy >= C && ldx >= C && lddx >= C && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0, ND_E_SHAPE,
               "nd_rmsnorm_backward: strides must be multiples of 4 floats >= C");
    ND_REQUIRE(nd_aligned16(dy) && nd_aligned16(x) && nd_aligned16(g) && nd_aligned16(dx), ND_E_ALIGN, "nd_rmsnorm_backward: alignment");
    const long npix = (long)B * HW;
    const long rows_per_wg = (npix + RMS_WGS - 1) / RMS_WGS;
    const int wgs = (int)((npix + rows_per_wg - 1) / rows_per_wg);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rmsnorm_bwd_kernel, dim3(wgs), dim3(256), 0, st, dy, lddy, x, ldx, g, dx, lddx, workspace, npix, C, rows_per_wg);
    hipLaunchKernelGGL(rmsnorm_dg_kernel, dim3(nd_cdiv(C, 32)), dim3(256), 0, st, workspace, dg, wgs, C);
    return nd_launch_status("nd_rmsnorm_backward_f32");
}
