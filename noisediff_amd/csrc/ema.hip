// ema.hip -- the shadow-model update of a training run (the reference's self.ema.update(), models/trainer_diffusion.py:63-69,191: ema_pytorch's
// EMA) for EVERY parameter and buffer in one pass, decided on the device.  The package reads its step counter on the host at every call (a sync per
// training step) and then runs one lerp_ / copy_ per tensor; here the counter, the warm-up flag and the decision live in device memory, so the call
// has no host read and a captured training step can contain it.
//
//   s = *step;  *step = s + 1                                       (every call)
//   s % update_every != 0                 skip
//   s <= update_after_step                copy: ema = src
//   !*initted                             copy, *initted = true, then the lerp below (a no-op in value)
//   otherwise                             ema = lerp(ema, src, 1 - decay),
//       e = max(s + 1 - update_after_step - 1, 0),  decay = e <= 0 ? 0 : clamp(1 - (1 + e / inv_gamma)^-power, min_value, beta)
//
// The decay is computed in fp64 and rounded to fp32 once.  Two launches: ema_plan_kernel (one thread) writes {action, weight} and advances the
// counter, ema_apply_kernel reads it -- a workgroup that finds `skip` returns before it touches a tensor.  Work is cut into chunks of EMA_CHUNK
// elements of one tensor, as adam.hip cuts it; the pass reads ema and src and writes ema: 12 bytes per element, HBM-bound.  No reductions, no
// atomics: bitwise repeatable.
#include "nd_common.h"

namespace {

constexpr int EMA_CHUNK = 8192;                                      // elements per workgroup: 256 threads x 8 float4

enum : int32_t { EMA_SKIP = 0, EMA_COPY = 1, EMA_LERP = 2, EMA_COPY_LERP = 3 };

struct ema_plan {
    int32_t action;
    float   weight;                                                  // 1 - decay (lerp actions), else 0
};

__global__ void ema_plan_kernel(int64_t* __restrict__ step, uint8_t* __restrict__ initted, ema_plan* __restrict__ plan, double beta,
                                int64_t update_after_step, int64_t update_every, double inv_gamma, double power, double min_value) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t s = *step;
    *step = s + 1;
    ema_plan out{EMA_SKIP, 0.0f};
    if (s % update_every == 0) {
        if (s <= update_after_step) {
            out.action = EMA_COPY;
        } else {
            out.action = *initted ? EMA_LERP : EMA_COPY_LERP;
            *initted = 1;
            const int64_t e = s + 1 - update_after_step - 1;         // the package reads the counter AFTER its increment
            double decay = 0.0;
            if (e > 0) {
                decay = 1.0 - pow(1.0 + (double)e / inv_gamma, -power);
                decay = decay < min_value ? min_value : decay;       // clamp(min = min_value, max = beta): the upper bound is applied last
                decay = decay > beta ? beta : decay;
            }
            out.weight = (float)(1.0 - decay);
        }
    }
    *plan = out;
}

// torch.lerp's form, every operation rounded on its own (no fused multiply-add)
__device__ __forceinline__ float ema_lerp(float e, float s, float w) {
#pragma clang fp contract(off)
    const float d = s - e;
    return w < 0.5f ? e + w * d : s - d * (1.0f - w);
}

__global__ __launch_bounds__(256) void ema_apply_kernel(const nd_ema_item* __restrict__ items, const int2* __restrict__ chunks,
                                                        const ema_plan* __restrict__ plan) {
    const ema_plan pl = *plan;
    if (pl.action == EMA_SKIP) return;
    const int2 ck = chunks[blockIdx.x];
    const nd_ema_item it = items[ck.x];
    const long lo = (long)ck.y * EMA_CHUNK;
    const long hi = lo + EMA_CHUNK < it.n ? lo + EMA_CHUNK : it.n;
    const bool whole = it.vec4 && hi - lo == EMA_CHUNK;              // whole chunk, 16-byte aligned tensors
    if (pl.action == EMA_COPY || it.no_ema) {
        if (whole) {
#pragma unroll 2
            for (long j = lo + 4 * threadIdx.x; j < hi; j += 4 * 256) nd_st4(it.ema + j, nd_ld4(it.src + j));
        } else {
            for (long j = lo + threadIdx.x; j < hi; j += 256) it.ema[j] = it.src[j];
        }
        return;
    }
    const bool first = pl.action == EMA_COPY_LERP;                   // the lerp starts from the copy
    const float w = pl.weight;
    if (whole) {
#pragma unroll 2
        for (long j = lo + 4 * threadIdx.x; j < hi; j += 4 * 256) {
            const f32x4 s = nd_ld4(it.src + j);
            f32x4 e = first ? s : nd_ld4(it.ema + j);
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = ema_lerp(e[k], s[k], w);
            nd_st4(it.ema + j, e);
        }
    } else {
        for (long j = lo + threadIdx.x; j < hi; j += 256) {
            const float s = it.src[j];
            it.ema[j] = ema_lerp(first ? s : it.ema[j], s, w);
        }
    }
}

}  // namespace

extern "C" int nd_ema_chunk_elements(void) { return EMA_CHUNK; }

extern "C" int nd_ema_update_f32(const nd_ema_item* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, int64_t* step_dev, uint8_t* initted_dev,
                                 void* plan_dev, double beta, int64_t update_after_step, int64_t update_every, double inv_gamma, double power, double min_value,
                                 void* stream) {
    ND_REQUIRE(items_dev && chunks_dev && n_items > 0 && n_chunks > 0, ND_E_BADARG, "nd_ema_update_f32: needs an item table and a chunk table in device memory");
    ND_REQUIRE(step_dev && initted_dev && plan_dev, ND_E_BADARG, "nd_ema_update_f32: needs the step counter, the initted flag and a plan record in device memory");
    ND_REQUIRE(beta >= 0.0 && beta <= 1.0 && update_every >= 1 && inv_gamma > 0.0, ND_E_BADARG,
               "nd_ema_update_f32: beta=%g must lie in [0, 1], update_every=%lld must be at least 1, inv_gamma=%g must be positive", beta,
               (long long)update_every, inv_gamma);
    hipLaunchKernelGGL(ema_plan_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, initted_dev, static_cast<ema_plan*>(plan_dev), beta,
                       update_after_step, update_every, inv_gamma, power, min_value);
    hipLaunchKernelGGL(ema_apply_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, items_dev, reinterpret_cast<const int2*>(chunks_dev),
                       static_cast<const ema_plan*>(plan_dev));
    return nd_launch_status("nd_ema_update_f32");
}
