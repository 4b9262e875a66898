// diffusion_train.hip -- the two ends of a diffusion training step around the network (GaussianDiffusion.forward / p_losses,
// models/denoising_diffusion_pytorch.py:481-542): what the reference spends a dozen ATen kernels on before the network sees x_t and as many after it.
//
//   nd_diffusion_noising_f32        ONE launch: (x0, seed, sample index, draw) -> t, x_t and the objective's target.
//   nd_diffusion_loss_f32           TWO launches: per-slice partial sums, then one workgroup that forms the loss in a fixed order.
//   nd_diffusion_loss_backward_f32  ONE launch: the loss gradient with respect to the network output.
//   nd_diffusion_train_advance      draw += 1 in device memory (one thread), so a captured step draws anew on every replay.
//
// Random numbers: Philox4x32-10 (philox_normal.h), key = the 64-bit seed, counter = {index, global sample = first_sample + b, draw, block}:
//   block 1  element noise: index = quad q of the sample's elements in NHWC order, the four normals go to the four consecutive NHWC elements
//            (the sampler's own convention, with block 0);
//   block 2  offset noise: index = c >> 2, component c & 3 -- one normal per (sample, channel);
//   block 3  timestep: index = 0, word 0 = w, t = (uint64(w) * T) >> 32.  w is uniform on 2^32 values, so a timestep's probability differs from
//            1 / T by less than 2^-32: the bias of the draw is below T / 2^32 relative to 1 / T (2.4e-7 at T = 1000).
// Block 0 stays the sampler's: training and sampling under one seed never share a stream.  Nothing depends on the batch size or on a sample's row in
// the batch, only on its global index.
//
// Arithmetic of the noising pass: every operation rounded on its own (no contraction), in the reference's order (:474-479, :490-492, :310-314, :539):
//   x = fl(fl(2 img) - 1) [auto_normalize]   n = fl(noise + fl(s offset)) [s > 0]   x_t = fl(fl(a x) + fl(b n))   v = fl(fl(a n) - fl(b x))
// so with explicit noise, t and offset the outputs are the reference's bit for bit.
//
// The loss: d = fl(out - target) and d * d in fp32, summed in fp64.  A sample's N = HW * C elements are cut into slices of LOSS_SLICE elements, one
// workgroup each; a slice's partial depends on neither B nor the sample's row, and the final stage adds the slices of a sample in slice order, so a
// sample's loss bits do not depend on its batch.  No atomics anywhere; every store is a vector store.
#include "nd_common.h"
#include "block_sum.h"
#include "philox_normal.h"

#pragma clang fp contract(off)

namespace {

constexpr int LOSS_SLICE = 4096;          // elements of one sample per workgroup: 256 threads x 4 float4
constexpr int LOSS_X0_MAX_C = 256;        // the mean-intensity term's per-channel sums: C a power of two up to this (a thread keeps one channel group)

__device__ __forceinline__ int clamp_t(int64_t t, int T) { return t < 0 ? 0 : (t >= T ? T - 1 : (int)t); }

__global__ __launch_bounds__(256) void noising_kernel(nd_diffusion_noising p, int psq, int G) {
    uint64_t seed = p.seed;
    int64_t first = p.first_sample;
    uint32_t draw = (uint32_t)p.draw;
    if (p.rng) { seed = (uint64_t)p.rng[0]; first = p.rng[1]; draw = (uint32_t)p.rng[2]; }
    const int HW = p.H * p.W;
    const float s = p.offset_strength;
    const bool need_off = s > 0.0f || p.offset_out;
    const size_t total = (size_t)p.B * psq;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / psq);
        const uint32_t q = (uint32_t)(i % psq), sample = (uint32_t)(first + b);
        const int pix = (int)(q / (uint32_t)G), cg = (int)(q % (uint32_t)G);
        int t;
        if (p.t_in) t = clamp_t(p.t_in[b], p.T);
        else {
            uint32_t c[4] = {0u, sample, draw, 3u};
            Philox::gen(c, (uint32_t)seed, (uint32_t)(seed >> 32));
            t = (int)(((uint64_t)c[0] * (uint64_t)p.T) >> 32);
        }
        if (q == 0) p.t_out[b] = (int64_t)t;
        const float a = p.sqrt_alphas_cumprod[t], bb = p.sqrt_one_minus_alphas_cumprod[t];
        f32x4 x;
        if (p.x0_channels_last) x = nd_ld4(p.x0 + i * 4);
        else {                                                     // NCHW: four planes HW apart, each load coalesced over the pixels of a wave
            const float* src = p.x0 + ((size_t)b * p.C + (size_t)cg * 4) * HW + pix;
            x = f32x4{src[0], src[HW], src[2 * (size_t)HW], src[3 * (size_t)HW]};
        }
        if (p.auto_normalize) x = x * 2.0f - 1.0f;
        f32x4 n = p.noise ? nd_ld4(p.noise + i * 4) : philox_normal4(seed, sample, draw, q, 1u);
        if (p.noise_out) nd_st4(p.noise_out + i * 4, n);
        if (need_off) {
            const size_t o = (size_t)b * p.C + (size_t)cg * 4;
            const f32x4 off = p.offset ? nd_ld4(p.offset + o) : philox_normal4(seed, sample, draw, (uint32_t)cg, 2u);
            if (p.offset_out && pix == 0) nd_st4(p.offset_out + o, off);
            if (s > 0.0f) n = n + s * off;
        }
        nd_st4(p.x_t + i * 4, a * x + bb * n);
        nd_st4(p.target + i * 4, p.objective == 0 ? n : (p.objective == 1 ? x : a * n - bb * x));
    }
}

__global__ void advance_draw_kernel(int64_t* rng) { rng[2] = rng[2] + 1; }

struct loss_ws {                                                   // the workspace's three regions, in this order (each a multiple of 16 bytes from the start)
    float* sign;         // [B][C]       sign of mean_hw(out) - mean_hw(target) (x0_term; read by the backward pass)
    double* sq;          // [B][ns]      sum of d^2 of a slice
    double* ch;          // [B][ns][C]   sum of (out - target) of a slice per channel (x0_term)
};
__host__ __device__ inline int loss_slices(int64_t N) { return (int)((N + LOSS_SLICE - 1) / LOSS_SLICE); }
__host__ __device__ inline loss_ws loss_regions(void* ws, int B, int C, int ns) {
    loss_ws r;
    r.sign = (float*)ws;
    r.sq = (double*)(r.sign + (size_t)B * C);                      // (C % 4 == 0: 16-byte aligned)
    r.ch = r.sq + (size_t)B * ns;
    return r;
}

// grid (ns, B): slice k of sample b
__global__ __launch_bounds__(256) void loss_partial_kernel(const float* __restrict__ out, const float* __restrict__ tgt, void* ws, int B, int C, int64_t N, int x0_term) {
    __shared__ double red[4];
    __shared__ double chl[4][LOSS_X0_MAX_C / 4][4];
    const int k = blockIdx.x, b = blockIdx.y, ns = gridDim.x, G = C >> 2;
    const loss_ws w = loss_regions(ws, B, C, ns);
    const int64_t lo = (int64_t)k * LOSS_SLICE, hi = lo + LOSS_SLICE < N ? lo + LOSS_SLICE : N;
    const float* o = out + (size_t)b * N;
    const float* t = tgt + (size_t)b * N;
    double acc = 0.0, ch[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = lo + 4 * (int64_t)threadIdx.x; e < hi; e += 4 * 256) {
        const f32x4 vo = nd_ld4(o + e), vt = nd_ld4(t + e);
        const f32x4 d = vo - vt, sq = d * d;
        acc = (((acc + (double)sq.x) + (double)sq.y) + (double)sq.z) + (double)sq.w;
        if (x0_term) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ch[j] += (double)vo[j] - (double)vt[j];
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) w.sq[(size_t)b * ns + k] = s;
    if (x0_term) {
        // G divides 64 and a slice starts at a multiple of G quads: thread tid sees channel group tid % G only.  Fold the lanes that share a group,
        // then the four waves in wave order.
        for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ch[j] += __shfl_xor(ch[j], off, ND_WAVE);
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane < G) {
#pragma unroll
            for (int j = 0; j < 4; ++j) chl[wave][lane][j] = ch[j];
        }
        __syncthreads();
        if ((int)threadIdx.x < C) {
            const int g = threadIdx.x >> 2, j = threadIdx.x & 3;
            w.ch[((size_t)b * ns + k) * C + threadIdx.x] = ((chl[0][g][j] + chl[1][g][j]) + chl[2][g][j]) + chl[3][g][j];
        }
    }
}

// one workgroup: loss = mean_b(mean_elems(d^2) w[t_b]) [+ mean_{b,c} |mean_hw(out) - mean_hw(target)|], slices in slice order, samples in a fixed tree
__global__ __launch_bounds__(256) void loss_final_kernel(void* ws, const int64_t* __restrict__ t, const float* __restrict__ weight, int T, int B, int C, int HW,
                                                         int ns, int x0_term, float* __restrict__ loss, float* __restrict__ sample_loss) {
    __shared__ double red[4];
    const loss_ws w = loss_regions(ws, B, C, ns);
    const double N = (double)HW * (double)C;
    double part = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        double s = 0.0;
        for (int k = 0; k < ns; ++k) s += w.sq[(size_t)b * ns + k];
        const double sl = s / N * (double)weight[clamp_t(t[b], T)];
        if (sample_loss) sample_loss[b] = (float)sl;
        part += sl;
    }
    double total = block_sum(part, red) / (double)B;
    if (x0_term) {
        double part2 = 0.0;
        for (int i = threadIdx.x; i < B * C; i += 256) {
            const int b = i / C, c = i % C;
            double s = 0.0;
            for (int k = 0; k < ns; ++k) s += w.ch[((size_t)b * ns + k) * C + c];
            const double m = s / (double)HW;
            w.sign[i] = m > 0.0 ? 1.0f : (m < 0.0 ? -1.0f : 0.0f);
            part2 += fabs(m);
        }
        total += block_sum(part2, red) / ((double)B * (double)C);
    }
    if (threadIdx.x == 0) *loss = (float)total;
}

// grid (ns, B): grad_out = g (2 w[t_b] / (B N) (out - target) [+ sign_{b,c} / (B N)]), formed in fp64 and rounded once
__global__ __launch_bounds__(256) void loss_backward_kernel(const float* __restrict__ out, const float* __restrict__ tgt, const int64_t* __restrict__ t,
                                                            const float* __restrict__ weight, const float* __restrict__ g, const void* ws,
                                                            float* __restrict__ grad, int T, int B, int C, int64_t N, int x0_term) {
    const int k = blockIdx.x, b = blockIdx.y, ns = gridDim.x;
    const loss_ws w = loss_regions(const_cast<void*>(ws), B, C, ns);
    const double gd = (double)*g, bn = (double)B * (double)N;
    const double sc = gd * 2.0 * (double)weight[clamp_t(t[b], T)] / bn, s2 = gd / bn;
    const int64_t lo = (int64_t)k * LOSS_SLICE, hi = lo + LOSS_SLICE < N ? lo + LOSS_SLICE : N;
    const size_t base = (size_t)b * N;
    for (int64_t e = lo + 4 * (int64_t)threadIdx.x; e < hi; e += 4 * 256) {
        const f32x4 vo = nd_ld4(out + base + e), vt = nd_ld4(tgt + base + e);
        f32x4 sg = {0.0f, 0.0f, 0.0f, 0.0f};
        if (x0_term) sg = nd_ld4(w.sign + (size_t)b * C + (size_t)(e % C));
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (float)(sc * ((double)vo[j] - (double)vt[j]) + s2 * (double)sg[j]);
        nd_st4(grad + base + e, r);
    }
}

int check_loss_shape(int B, int C, int HW, int T, int x0_term, const char* who) {
    ND_REQUIRE(B > 0 && C > 0 && HW > 0 && T > 0, ND_E_BADARG, "%s: B=%d, C=%d, HW=%d, T=%d must be positive", who, B, C, HW, T);
    ND_REQUIRE(C % 4 == 0, ND_E_SHAPE, "%s: C=%d must be a multiple of 4", who, C);
    ND_REQUIRE(B <= 65535 && (int64_t)HW * C < ((int64_t)1 << 40), ND_E_SHAPE, "%s: B=%d (<= 65535) or HW * C too large", who, B);
    ND_REQUIRE(!x0_term || (C <= LOSS_X0_MAX_C && (C & (C - 1)) == 0), ND_E_SHAPE, "%s: the mean-intensity term takes C a power of two up to %d, got %d", who,
               LOSS_X0_MAX_C, C);
    return 0;
}

}  // namespace

extern "C" int nd_diffusion_noising_f32(const nd_diffusion_noising* p, void* stream) {
    const char* who = "nd_diffusion_noising_f32";
    ND_REQUIRE(p, ND_E_BADARG, "%s: null parameter block", who);
    ND_REQUIRE(p->x0 && p->sqrt_alphas_cumprod && p->sqrt_one_minus_alphas_cumprod && p->t_out && p->x_t && p->target, ND_E_BADARG,
               "%s: x0, the two schedule tables, t_out, x_t and target are required", who);
    ND_REQUIRE(p->B > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->T > 0, ND_E_BADARG, "%s: B, C, H, W, T must be positive", who);
    ND_REQUIRE(p->objective >= 0 && p->objective <= 2, ND_E_BADARG, "%s: objective %d", who, p->objective);
    ND_REQUIRE(p->offset_strength >= 0.0f && p->offset_strength <= 3.0e38f, ND_E_BADARG, "%s: offset_strength must be finite and not negative", who);
    ND_REQUIRE(p->C % 4 == 0, ND_E_SHAPE, "%s: C=%d must be a multiple of 4", who, p->C);
    const int64_t psq = (int64_t)p->H * p->W * (p->C / 4);
    ND_REQUIRE(psq < ((int64_t)1 << 31) && (int64_t)p->H * p->W < ((int64_t)1 << 31), ND_E_SHAPE, "%s: a sample has too many elements", who);
    ND_REQUIRE(nd_aligned16(p->x0) && nd_aligned16(p->noise) && nd_aligned16(p->offset) && nd_aligned16(p->x_t) && nd_aligned16(p->target) &&
                   nd_aligned16(p->noise_out) && nd_aligned16(p->offset_out),
               ND_E_ALIGN, "%s: x0, noise, offset, x_t, target, noise_out and offset_out must be 16-byte aligned", who);
    ND_REQUIRE((((uintptr_t)p->t_in | (uintptr_t)p->t_out | (uintptr_t)p->rng) & 7u) == 0, ND_E_ALIGN, "%s: t_in, t_out and rng must be 8-byte aligned", who);
    const size_t total = (size_t)p->B * (size_t)psq;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(noising_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *p, (int)psq, p->C / 4);
    return nd_launch_status(who);
}

extern "C" int nd_diffusion_train_advance(int64_t* rng, void* stream) {
    ND_REQUIRE(rng, ND_E_BADARG, "nd_diffusion_train_advance: null rng");
    ND_REQUIRE((((uintptr_t)rng) & 7u) == 0, ND_E_ALIGN, "nd_diffusion_train_advance: rng must be 8-byte aligned");
    hipLaunchKernelGGL(advance_draw_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng);
    return nd_launch_status("nd_diffusion_train_advance");
}

extern "C" int nd_diffusion_loss_slice_elements(void) { return LOSS_SLICE; }

extern "C" int64_t nd_diffusion_loss_workspace_bytes(int B, int C, int HW) {
    if (int e = check_loss_shape(B, C, HW, 1, 0, "nd_diffusion_loss_workspace_bytes")) return e;
    const int64_t ns = loss_slices((int64_t)HW * C);
    const int64_t bytes = 8 * (int64_t)B * ns * (1 + C) + 4 * (int64_t)B * C;
    return (bytes + 15) / 16 * 16;
}

extern "C" int nd_diffusion_loss_f32(const float* model_out, const float* target, const int64_t* t, const float* loss_weight, int B, int C, int HW, int T,
                                     int x0_term, void* workspace, float* loss, float* sample_loss, void* stream) {
    const char* who = "nd_diffusion_loss_f32";
    ND_REQUIRE(model_out && target && t && loss_weight && workspace && loss, ND_E_BADARG, "%s: null pointer", who);
    if (int e = check_loss_shape(B, C, HW, T, x0_term, who)) return e;
    ND_REQUIRE(nd_aligned16(model_out) && nd_aligned16(target) && nd_aligned16(workspace), ND_E_ALIGN, "%s: model_out, target and workspace must be 16-byte aligned", who);
    const int64_t N = (int64_t)HW * C;
    const int ns = loss_slices(N);
    hipLaunchKernelGGL(loss_partial_kernel, dim3(ns, B), dim3(256), 0, (hipStream_t)stream, model_out, target, workspace, B, C, N, x0_term);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, t, loss_weight, T, B, C, HW, ns, x0_term, loss, sample_loss);
    return nd_launch_status(who);
}

extern "C" int nd_diffusion_loss_backward_f32(const float* model_out, const float* target, const int64_t* t, const float* loss_weight, const float* g,
                                              const void* workspace, float* grad_out, int B, int C, int HW, int T, int x0_term, void* stream) {
    const char* who = "nd_diffusion_loss_backward_f32";
    ND_REQUIRE(model_out && target && t && loss_weight && g && grad_out && (workspace || !x0_term), ND_E_BADARG, "%s: null pointer", who);
    if (int e = check_loss_shape(B, C, HW, T, x0_term, who)) return e;
    ND_REQUIRE(nd_aligned16(model_out) && nd_aligned16(target) && nd_aligned16(grad_out) && nd_aligned16(workspace), ND_E_ALIGN,
               "%s: model_out, target, grad_out and workspace must be 16-byte aligned", who);
    const int64_t N = (int64_t)HW * C;
    hipLaunchKernelGGL(loss_backward_kernel, dim3(loss_slices(N), B), dim3(256), 0, (hipStream_t)stream, model_out, target, t, loss_weight, g, workspace, grad_out,
                       T, B, C, N, x0_term);
    return nd_launch_status(who);
}
