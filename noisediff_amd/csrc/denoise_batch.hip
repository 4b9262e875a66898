// denoise_batch.hip -- the denoiser's training batch from generated noise patches, in one launch.
//
// SyntheticNoisDiffDenoisingDataset.__getitem__ (dataloader/dataset_denoising.py:132-168: compose, remove_darkshading :80-118, the even-aligned
// crop :120-130), Trainer.prepare's flip (models/trainer_denoising.py:100-112) and PMN's shot-noise augmentation (SNA_torch :140-166 inside the
// per-sample loop :207-217) are host numpy and a dozen small torch launches per sample in the reference.  Here one kernel reads the crop
// windows of `noise` and `clean` (and of the dark-shading planes), and writes `noisy` and `clean_out`, per output element (c, y, x):
//
//   ys = cy + (flip ? h-1-y : y), xs = cx + x                                  torch.flip(dims=[2]) of NCHW is the H axis
//   n = clip(noise, -1, 1);  v = clip(n + clean, 0, 1);  g = clip(clean, 0, 1)          clips by comparison: NaN passes through
//   shading:  im = v / ratio; im = im * 15871 + 512; im = clip(im, 0, 16383); im -= (ds_k[c][Y][X] * iso + ds_b[c][Y][X]) + blc;
//             im = max(im - 512, 0); im = im / 15871; im = im * ratio; v = clip(im, 0, 1)          (Y, X) = (y0 + ys, x0 + xs)
//   SNA:      lam = (double)g * 15871 / ratio * wb[c] / K (fp64);  k ~ Poisson(lam);
//             gt = g * 15871 / ratio; dy = gt * wb[c]; dn = k * K; dy = dy * ratio / 15871; dn = dn / 15871; dn = dn * ratio;
//             noisy = v + dn; clean_out = g + dy                               (no clip after: the reference has none)
//
// Every fp32 and fp64 operation is a single IEEE operation in the order written: contraction to fma is off for this file, so numpy repeats
// the arithmetic bit for bit.
//
// The Poisson draw is counter-based: Philox4x32-10, key = the 64-bit seed, counter = {element index within the sample (c h w + y w + x of the
// OUTPUT position), global sample index, draw index, block j}; uniforms u = (word + 0.5) 2^-32 in fp64; every decision in fp64.
//   lam == 0: 0.   0 < lam < 10: inversion by sequential search on word 0 of block 0 (at most PO_INV_MAX steps).
//   lam >= 10: Hoermann's transformed rejection (PTRS, "The transformed rejection method for generating Poisson random variables", 1993);
//   attempt t takes words 2 (t mod 2), 2 (t mod 2) + 1 of block t / 2 (at most PO_MAX_ATTEMPTS; the chance to need more is below 1e-38).
//   lam negative, NaN or infinite: NaN.
// A sample's bits depend on (seed, its global index, draw) and its own data only: not on the batch around it, the grid or the vector width.
#include "nd_common.h"

#pragma clang fp contract(off)

#include "philox_poisson.h"          // philox_poisson(lam, seed, elem, sample, draw): the draw described above, shared with raw.hip

namespace {

constexpr int DB_THREADS = 256;

struct DbArgs {
    const float* noise;  const float* clean;
    const float* ds[4];                 // k_high, b_high, k_low, b_low planes (4, Hm, Wm), or all null
    const nd_denoise_sample* table;     // [B]
    const float* sna;                   // [B][ND_DENOISE_SNA_WORDS]: wb[4], K; or null
    const int64_t* rng;                 // {seed, first_sample, draw} or null
    const float* counts_in;  float* counts_out;
    float* noisy;  float* clean_out;
    uint64_t seed;  int64_t first_sample;  int32_t draw;
    int P, h, w, Hm, Wm;
};

// Thread i of block row blockIdx.y = sample b takes output elements e = V i .. V i + V - 1 of the sample's (4, h, w): one row, V columns.
template <int V>
__global__ __launch_bounds__(DB_THREADS) void denoise_batch_kernel(DbArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w, P = A.P;
    const size_t per = (size_t)4 * h * w;
    const size_t e = ((size_t)blockIdx.x * DB_THREADS + threadIdx.x) * V;
    if (e >= per) return;
    const nd_denoise_sample s = A.table[b];
    const int c = (int)(e / ((size_t)h * w));
    const int rem = (int)(e - (size_t)c * h * w);
    const int y = rem / w, x = rem - y * w;
    const size_t o = (size_t)b * per + e;

    const bool shading = A.ds[0] != nullptr;
    // a parameter row that points outside its tensors is refused here as well as on the host: NaN out, nothing read
    bool ok = s.cx >= 0 && s.cy >= 0 && s.cx <= P - w && s.cy <= P - h && ((s.cx | s.cy) & 1) == 0;
    if (shading) ok = ok && s.x0 >= 0 && s.y0 >= 0 && s.x0 <= A.Wm - P && s.y0 <= A.Hm - P;
    if (!ok) {
        float nanv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) nanv[i] = __builtin_nanf("");
        nd_store_v<V>(A.noisy + o, nanv);
        nd_store_v<V>(A.clean_out + o, nanv);
        if (A.counts_out) nd_store_v<V>(A.counts_out + o, nanv);
        return;
    }
    const int ys = s.cy + (s.flip ? h - 1 - y : y), xs = s.cx + x;
    const size_t src = (((size_t)b * 4 + c) * P + ys) * P + xs;
    float nz[V], cl[V], v[V], g[V];
    nd_load_v<V>(A.noise + src, nz);
    nd_load_v<V>(A.clean + src, cl);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float n = nd_clip(nz[i], -1.0f, 1.0f);
        v[i] = nd_clip(n + cl[i], 0.0f, 1.0f);
        g[i] = nd_clip(cl[i], 0.0f, 1.0f);
    }
    if (shading) {
        const size_t m = ((size_t)c * A.Hm + (s.y0 + ys)) * A.Wm + (s.x0 + xs);
        const int pair = s.branch ? 0 : 2;                  // iso > 1600: the high-ISO maps
        float dk[V], dbv[V];
        nd_load_v<V>(A.ds[pair] + m, dk);
        nd_load_v<V>(A.ds[pair + 1] + m, dbv);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float im = v[i] / s.ratio;
            im = im * 15871.0f + 512.0f;
            im = nd_clip(im, 0.0f, 16383.0f);
            const float dark = (dk[i] * s.iso + dbv[i]) + s.blc;
            im = im - dark;
            im = im - 512.0f;
            im = im < 0.0f ? 0.0f : im;
            im = im / 15871.0f;
            im = im * s.ratio;
            v[i] = nd_clip(im, 0.0f, 1.0f);
        }
    }
    float wbc = 0.0f, K = 0.0f;
    bool sna = false;
    if (A.sna) {
        const float* q = A.sna + (size_t)b * ND_DENOISE_SNA_WORDS;
        sna = !(q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f);       // trainer_denoising.py:213
        wbc = q[c];
        K = q[4];
    }
    float cnt[V];
#pragma unroll
    for (int i = 0; i < V; ++i) cnt[i] = 0.0f;
    if (sna) {
        if (A.counts_in) {
            nd_load_v<V>(A.counts_in + o, cnt);
        } else {
            uint64_t seed = A.seed;
            int64_t first = A.first_sample;
            uint32_t draw = (uint32_t)A.draw;
            if (A.rng) { seed = (uint64_t)A.rng[0];  first = A.rng[1];  draw = (uint32_t)A.rng[2]; }
#pragma unroll 1
            for (int i = 0; i < V; ++i) {
                const double lam = (double)g[i] * 15871.0 / (double)s.ratio * (double)wbc / (double)K;
                cnt[i] = (float)philox_poisson(lam, seed, (uint32_t)(e + i), (uint32_t)(first + b), draw);
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float gt = g[i] * 15871.0f / s.ratio;
            float dy = gt * wbc;
            float dn = cnt[i] * K;
            dy = dy * s.ratio / 15871.0f;
            dn = dn / 15871.0f;
            dn = dn * s.ratio;
            v[i] = v[i] + dn;
            g[i] = g[i] + dy;
        }
    }
    nd_store_v<V>(A.noisy + o, v);
    nd_store_v<V>(A.clean_out + o, g);
    if (A.counts_out) nd_store_v<V>(A.counts_out + o, cnt);
}

__global__ __launch_bounds__(DB_THREADS) void philox_poisson_kernel(const float* __restrict__ rate, float* __restrict__ out, uint64_t seed,
                                                                    int64_t first_sample, uint32_t draw, int B, size_t n) {
    const size_t total = (size_t)B * n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / n;
        out[i] = (float)philox_poisson((double)rate[i], seed, (uint32_t)(i - b * n), (uint32_t)(first_sample + (int64_t)b), draw);
    }
}

// planes[c][Y][X] = bayer[2 Y + (c >= 2)][2 X + (c == 1 || c == 2)]: pack_np_raw's channel order (R, G, B, G of RGGB)
__global__ __launch_bounds__(DB_THREADS) void pack_darkshading_kernel(const float* __restrict__ bayer, float* __restrict__ planes, int H, int W) {
    const size_t total = (size_t)4 * H * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / ((size_t)H * W));
        const size_t rem = i - (size_t)c * H * W;
        const int Y = (int)(rem / W), X = (int)(rem - (size_t)Y * W);
        planes[i] = bayer[(size_t)(2 * Y + (c >= 2)) * (2 * (size_t)W) + 2 * X + (c == 1 || c == 2)];
    }
}

int db_blocks(size_t total) {
    const size_t n = (total + DB_THREADS - 1) / DB_THREADS;
    return (int)(n < 4096 ? n : 4096);
}

}  // namespace

extern "C" int nd_denoise_batch_f32(const float* noise, const float* clean, const float* ds_k_high, const float* ds_b_high, const float* ds_k_low,
                                    const float* ds_b_low, int map_h, int map_w, const nd_denoise_sample* table, const float* sna,
                                    const int64_t* rng, uint64_t seed, int64_t first_sample, int32_t draw, const float* counts_in,
                                    float* counts_out, float* noisy, float* clean_out, int B, int patch, int crop_h, int crop_w, void* stream) {
    const char* who = "nd_denoise_batch_f32";
    ND_REQUIRE(noise && clean && table && noisy && clean_out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE(B > 0 && B <= 65535 && patch > 0 && crop_h > 0 && crop_w > 0, ND_E_BADARG, "%s: B (<= 65535), patch and crop must be positive", who);
    ND_REQUIRE(draw >= 0, ND_E_BADARG, "%s: draw index %d is negative", who, draw);
    const int nmaps = (ds_k_high != nullptr) + (ds_b_high != nullptr) + (ds_k_low != nullptr) + (ds_b_low != nullptr);
    ND_REQUIRE(nmaps == 0 || nmaps == 4, ND_E_BADARG, "%s: give all four dark-shading planes or none", who);
    ND_REQUIRE(crop_h <= patch && crop_w <= patch, ND_E_SHAPE, "%s: crop %d x %d does not fit the %d patch", who, crop_h, crop_w, patch);
    ND_REQUIRE(patch % 2 == 0 && crop_h % 2 == 0 && crop_w % 2 == 0, ND_E_SHAPE, "%s: patch and crop sizes must be even (whole Bayer cells)", who);
    ND_REQUIRE((int64_t)4 * crop_h * crop_w < (1ll << 32), ND_E_SHAPE, "%s: 4 * crop_h * crop_w must fit the 32-bit element counter", who);
    ND_REQUIRE(nmaps == 0 || (map_h >= patch && map_w >= patch), ND_E_SHAPE, "%s: shading planes %d x %d are smaller than the patch", who, map_h, map_w);
    const uintptr_t in_bits = (uintptr_t)noise | (uintptr_t)clean | (uintptr_t)counts_in;
    ND_REQUIRE((in_bits & 7u) == 0, ND_E_ALIGN, "%s: noise, clean and counts_in must be 8-byte aligned", who);
    ND_REQUIRE(((uintptr_t)table & 3u) == 0 && ((uintptr_t)sna & 3u) == 0 && ((uintptr_t)rng & 7u) == 0 &&
               (((uintptr_t)ds_k_high | (uintptr_t)ds_b_high | (uintptr_t)ds_k_low | (uintptr_t)ds_b_low) & 3u) == 0, ND_E_ALIGN,
               "%s: table, sna and planes must be 4-byte aligned, rng 8-byte", who);
    const uintptr_t out_bits = (uintptr_t)noisy | (uintptr_t)clean_out | (uintptr_t)counts_out;
    ND_REQUIRE((out_bits & 7u) == 0, ND_E_ALIGN, "%s: noisy, clean_out and counts_out must be 8-byte aligned", who);
    DbArgs A;
    A.noise = noise;  A.clean = clean;
    A.ds[0] = ds_k_high;  A.ds[1] = ds_b_high;  A.ds[2] = ds_k_low;  A.ds[3] = ds_b_low;
    A.table = table;  A.sna = sna;  A.rng = rng;  A.counts_in = counts_in;  A.counts_out = counts_out;  A.noisy = noisy;  A.clean_out = clean_out;
    A.seed = seed;  A.first_sample = first_sample;  A.draw = draw;
    A.P = patch;  A.h = crop_h;  A.w = crop_w;  A.Hm = map_h;  A.Wm = map_w;
    const size_t per = (size_t)4 * crop_h * crop_w;
    const bool v4 = crop_w % 4 == 0 && (out_bits & 15u) == 0;
    const size_t threads = per / (v4 ? 4 : 2);
    const dim3 grid((unsigned)((threads + DB_THREADS - 1) / DB_THREADS), (unsigned)B);
    if (v4) hipLaunchKernelGGL(denoise_batch_kernel<4>, grid, dim3(DB_THREADS), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(denoise_batch_kernel<2>, grid, dim3(DB_THREADS), 0, (hipStream_t)stream, A);
    return nd_launch_status(who);
}

extern "C" int nd_philox_poisson_f32(const float* rate, float* out, uint64_t seed, int64_t first_sample, int32_t draw, int B, int64_t n_per_sample,
                                     void* stream) {
    ND_REQUIRE(rate && out, ND_E_BADARG, "nd_philox_poisson_f32: null pointer");
    ND_REQUIRE(B > 0 && n_per_sample > 0 && draw >= 0, ND_E_BADARG, "nd_philox_poisson_f32: B, n_per_sample must be positive and draw >= 0");
    ND_REQUIRE(n_per_sample < (1ll << 32), ND_E_SHAPE, "nd_philox_poisson_f32: n_per_sample must fit the 32-bit element counter");
    ND_REQUIRE((((uintptr_t)rate | (uintptr_t)out) & 3u) == 0, ND_E_ALIGN, "nd_philox_poisson_f32: rate and out must be 4-byte aligned");
    hipLaunchKernelGGL(philox_poisson_kernel, dim3(db_blocks((size_t)B * n_per_sample)), dim3(DB_THREADS), 0, (hipStream_t)stream, rate, out, seed,
                       first_sample, (uint32_t)draw, B, (size_t)n_per_sample);
    return nd_launch_status("nd_philox_poisson_f32");
}

extern "C" int nd_pack_darkshading_f32(const float* bayer, float* planes, int H2, int W2, void* stream) {
    ND_REQUIRE(bayer && planes, ND_E_BADARG, "nd_pack_darkshading_f32: null pointer");
    ND_REQUIRE(H2 > 0 && W2 > 0, ND_E_BADARG, "nd_pack_darkshading_f32: sizes must be positive");
    ND_REQUIRE(H2 % 2 == 0 && W2 % 2 == 0, ND_E_SHAPE, "nd_pack_darkshading_f32: a Bayer map has even sides; got %d x %d", H2, W2);
    ND_REQUIRE((((uintptr_t)bayer | (uintptr_t)planes) & 3u) == 0, ND_E_ALIGN, "nd_pack_darkshading_f32: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(pack_darkshading_kernel, dim3(db_blocks((size_t)H2 * W2)), dim3(DB_THREADS), 0, (hipStream_t)stream, bayer, planes, H2 / 2,
                       W2 / 2);
    return nd_launch_status("nd_pack_darkshading_f32");
}
