// raw.hip -- uint16 Bayer frames to and from the packed fp32 tensors the denoiser takes, one launch each.
//
// The reference starts every test_denoising.py frame and every RealSony / Poisson-Gaussian training sample from a uint16 Bayer frame with a
// dozen whole-frame numpy passes on the host (utils/raw_util.py pack_raw :17-35, pack_raw_withdarkshading :112-139; test_denoising.py
// load_image :86-114; dataloader/dataset_denoising.py :232-265, :332-360) and ends a visualised frame with postprocess_bayer (:267-293).
// Here the frames stay on the device as uint16 and four kernels do the arithmetic:
//
//   raw_pack_kernel<V, MODE>   windows of frames -> fp32 NCHW (B, 4, h, w), MODE = ND_RAW_PACK / ND_RAW_PACK_SHADED / ND_RAW_TRAIN_REAL
//   raw_pg_kernel<V>           the same windows with Poisson-Gaussian noise drawn per element (apply_noise)
//   raw_bayer_kernel<V>        fp32 (B, 4, h, w) -> uint16 (B, 2h, 2w)
//   raw_diffusion_kernel<V>    the diffusion sets' sample (dataloader/dataset.py): noise, noisy, clean (B, 4, h, w) and coord (B, 2, h, w), any subset
//
// The arithmetic of each is listed step by step in include/noisediff_hip.h.  Every fp32 and fp64 operation is a single IEEE operation in the
// order written there: contraction to fma is off for this file, so numpy repeats it bit for bit.
//
// Addressing: packed pixel (Y, X) is the 2 x 2 Bayer cell at (2Y, 2X); its four codes are two adjacent uint16 pairs, one in each Bayer row.
// A thread takes V = 4, 2 or 1 consecutive packed columns of one output row (the widest V that w and the outputs' alignment allow, chosen
// on the host) and reads 2V codes = 4V bytes from each Bayer row with the widest load the address allows: a window origin is any integer,
// so a 16-byte row start is the common case and not a promise.  No LDS; grid (tiles, B).
#include "nd_common.h"

#pragma clang fp contract(off)

#include "philox_poisson.h"
#include "raw_codes.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr uint32_t RW_NORMAL_BLOCK = 32u;           // the Philox block of the normal draw: PO_MAX_ATTEMPTS / 2, the first the Poisson draw leaves
static_assert(RW_NORMAL_BLOCK == PO_MAX_ATTEMPTS / 2, "the normal draw takes the first block the Poisson draw cannot reach");


template <int V>
__device__ __forceinline__ void rw_store_nan(float* p) {
    float nanv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) nanv[i] = __builtin_nanf("");
    nd_store_v<V>(p, nanv);
}

struct RawArgs {
    const uint16_t* frames;
    const float* ds[4];                 // k_high, b_high, k_low, b_low planes (4, Hm, Wm), or all null
    const nd_raw_sample* table;         // [B]
    float* out;  float* clean_out;
    int N, H, W, Hm, Wm, h, w;          // H, W: the packed frame
    int flags;
    float black, white;
};

__device__ __forceinline__ bool rw_window_ok(const nd_raw_sample& s, int N, int H, int W, int h, int w) {
    return s.frame >= 0 && s.frame < N && s.x0 >= 0 && s.y0 >= 0 && s.x0 <= W - w && s.y0 <= H - h;
}

template <int MODE>
__device__ __forceinline__ float rw_pack(float x, float d, const nd_raw_sample& s, float black, float white, float wb, int flags, bool shading) {
    if constexpr (MODE == ND_RAW_PACK) {
        float v = x - black;
        v = v < 0.0f ? 0.0f : v;
        if (flags & ND_RAW_RESCALE) v = v / wb;
        if (flags & ND_RAW_CLIP) v = nd_clip(v * s.ratio, 0.0f, 1.0f);
        return v;
    } else if constexpr (MODE == ND_RAW_PACK_SHADED) {
        float v = (x - black) / wb;
        v = nd_clip(v * s.ratio, 0.0f, 1.0f);
        v = v / s.ratio;
        v = v * wb + black;
        v = nd_clip(v, 0.0f, white);
        v = v - d;
        v = v - black;
        v = v < 0.0f ? 0.0f : v;
        v = v / wb;
        return nd_clip(v * s.ratio, 0.0f, 1.0f);
    } else {
        float v = x - black;
        v = v < 0.0f ? 0.0f : v;
        if (shading) v = v - d;
        v = v * s.ratio;
        v = nd_clip(v, 0.0f, wb);
        return v / wb;
    }
}

// Thread i of block row blockIdx.y = sample b takes packed columns V (i mod (w / V)) .. + V - 1 of output row i / (w / V), all four channels.
template <int V, int MODE>
__global__ __launch_bounds__(RW_THREADS) void raw_pack_kernel(RawArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w, wv = w / V;
    const size_t t = (size_t)blockIdx.x * RW_THREADS + threadIdx.x;
    if (t >= (size_t)h * wv) return;
    const int y = (int)(t / wv), x = (int)(t - (size_t)y * wv) * V;
    const nd_raw_sample s = A.table[b];
    const size_t plane = (size_t)h * w;
    const size_t o = (size_t)b * 4 * plane + (size_t)y * w + x;

    const bool shading = A.ds[0] != nullptr;
    // a parameter row that points outside its tensors is refused here as well as on the host: NaN out, nothing read
    bool ok = rw_window_ok(s, A.N, A.H, A.W, h, w);
    if (shading) ok = ok && s.x0 <= A.Wm - w && s.y0 <= A.Hm - h;
    if (MODE == ND_RAW_TRAIN_REAL) ok = ok && s.frame_clean >= 0 && s.frame_clean < A.N;
    if (!ok) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            rw_store_nan<V>(A.out + o + c * plane);
            if (MODE == ND_RAW_TRAIN_REAL) rw_store_nan<V>(A.clean_out + o + c * plane);
        }
        return;
    }
    const int Y = s.y0 + (s.flip ? h - 1 - y : y), X = s.x0 + x;
    const size_t W2 = 2 * (size_t)A.W;
    const size_t cell = (2 * (size_t)Y) * W2 + 2 * (size_t)X;                  // the cell's top-left code within a frame
    const uint16_t* src = A.frames + (size_t)s.frame * (2 * (size_t)A.H) * W2 + cell;
    uint32_t top[V], bottom[V];
    rw_load_pairs<V>(src, top);
    rw_load_pairs<V>(src + W2, bottom);
    const float black = A.black, white = A.white, wb = white - black;
    const int pair = s.branch ? 0 : 2;                                          // iso > 1600: the high-ISO maps
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float d[V], v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) d[i] = 0.0f;
        if (shading) {
            const size_t m = ((size_t)c * A.Hm + Y) * A.Wm + X;
            float dk[V], db[V];
            nd_load_v<V>(A.ds[pair] + m, dk);
            nd_load_v<V>(A.ds[pair + 1] + m, db);
#pragma unroll
            for (int i = 0; i < V; ++i) d[i] = (dk[i] * s.iso + db[i]) + s.blc;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = rw_pack<MODE>(rw_code(top[i], bottom[i], c), d[i], s, black, white, wb, A.flags, shading);
        nd_store_v<V>(A.out + o + c * plane, v);
    }
    if (MODE == ND_RAW_TRAIN_REAL) {
        const uint16_t* cl = A.frames + (size_t)s.frame_clean * (2 * (size_t)A.H) * W2 + cell;
        rw_load_pairs<V>(cl, top);
        rw_load_pairs<V>(cl + W2, bottom);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v[V];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float g = rw_code(top[i], bottom[i], c) - black;
                v[i] = (g < 0.0f ? 0.0f : g) / wb;
            }
            nd_store_v<V>(A.clean_out + o + c * plane, v);
        }
    }
}

struct PgArgs {
    const uint16_t* frames;
    const nd_raw_sample* table;
    const int64_t* rng;                 // {seed, first_sample, draw} or null
    const float* counts_in;  const float* normals_in;
    float* counts_out;  float* normals_out;
    float* noisy;  float* clean_out;
    uint64_t seed;  int64_t first_sample;  int32_t draw;
    int N, H, W, h, w;
    float black, white;
};

// Thread i of block row blockIdx.y = sample b takes output elements e = V i .. V i + V - 1 of the sample's (4, h, w): one channel, one row, V columns.
template <int V>
__global__ __launch_bounds__(RW_THREADS) void raw_pg_kernel(PgArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w;
    const size_t per = (size_t)4 * h * w;
    const size_t e = ((size_t)blockIdx.x * RW_THREADS + threadIdx.x) * V;
    if (e >= per) return;
    const nd_raw_sample s = A.table[b];
    const int c = (int)(e / ((size_t)h * w));
    const int rem = (int)(e - (size_t)c * h * w);
    const int y = rem / w, x = rem - y * w;
    const size_t o = (size_t)b * per + e;
    if (!rw_window_ok(s, A.N, A.H, A.W, h, w)) {
        rw_store_nan<V>(A.noisy + o);
        rw_store_nan<V>(A.clean_out + o);
        if (A.counts_out) rw_store_nan<V>(A.counts_out + o);
        if (A.normals_out) rw_store_nan<V>(A.normals_out + o);
        return;
    }
    const int Y = s.y0 + (s.flip ? h - 1 - y : y), X = s.x0 + x;
    const size_t W2 = 2 * (size_t)A.W;
    const uint16_t* src = A.frames + ((size_t)s.frame * (2 * (size_t)A.H) + 2 * (size_t)Y + (c >= 2)) * W2 + 2 * (size_t)X;
    uint32_t wd[V];
    rw_load_pairs<V>(src, wd);
    const float black = A.black, wb = A.white - black;
    const float ratio32 = (float)s.ratio64;
    float cf[V], cnt[V], nrm[V], noisy[V], clean[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float g = rw_code(wd[i], wd[i], c) - black;
        cf[i] = g < 0.0f ? 0.0f : g;
        clean[i] = cf[i] / wb;
    }
    if (A.counts_in) nd_load_v<V>(A.counts_in + o, cnt);
    if (A.normals_in) nd_load_v<V>(A.normals_in + o, nrm);
    if (!A.counts_in || !A.normals_in) {
        uint64_t seed = A.seed;
        int64_t first = A.first_sample;
        uint32_t draw = (uint32_t)A.draw;
        if (A.rng) { seed = (uint64_t)A.rng[0];  first = A.rng[1];  draw = (uint32_t)A.rng[2]; }
        const uint32_t sample = (uint32_t)(first + b);
#pragma unroll 1
        for (int i = 0; i < V; ++i) {
            if (!A.counts_in) {
                const float latent = cf[i] / ratio32;
                const double lam = (double)latent / s.k;
                cnt[i] = (float)philox_poisson(lam, seed, (uint32_t)(e + i), sample, draw);
            }
            if (!A.normals_in) {
                uint32_t ctr[4] = {(uint32_t)(e + i), sample, draw, RW_NORMAL_BLOCK};
                Philox::gen(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
                const double u0 = po_uniform(ctr[0]), u1 = po_uniform(ctr[1]);
                const double r = sqrt(-2.0 * log(u0));
                const double a = 6.283185307179586 * u1;
                nrm[i] = (float)(r * cos(a));
            }
        }
    }
    const double wbd = (double)wb;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const double p = s.k * (double)cnt[i];
        const double g = s.sd * (double)nrm[i];
        double t = p + g;
        t = t * s.ratio64;
        t = nd_clip<double>(t, 0.0, wbd);
        t = t / wbd;
        noisy[i] = (float)t;
    }
    nd_store_v<V>(A.noisy + o, noisy);
    nd_store_v<V>(A.clean_out + o, clean);
    if (A.counts_out) nd_store_v<V>(A.counts_out + o, cnt);
    if (A.normals_out) nd_store_v<V>(A.normals_out + o, nrm);
}

struct BayerArgs {
    const float* img;
    uint16_t* out;
    int bl[4];
    int white, h, w;
};

// Thread i of block row blockIdx.y = image b takes packed columns V (i mod (w / V)) .. + V - 1 of packed row i / (w / V): 2 x 2V codes.
template <int V>
__global__ __launch_bounds__(RW_THREADS) void raw_bayer_kernel(BayerArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w, wv = w / V;
    const size_t t = (size_t)blockIdx.x * RW_THREADS + threadIdx.x;
    if (t >= (size_t)h * wv) return;
    const int y = (int)(t / wv), x = (int)(t - (size_t)y * wv) * V;
    const size_t plane = (size_t)h * w;
    const float* src = A.img + (size_t)b * 4 * plane + (size_t)y * w + x;
    float ch[4][V];
#pragma unroll
    for (int c = 0; c < 4; ++c) nd_load_v<V>(src + c * plane, ch[c]);
    uint32_t top[V], bottom[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        top[i] = rw_to_code(ch[0][i], A.bl[0], A.white) | (rw_to_code(ch[1][i], A.bl[1], A.white) << 16);
        bottom[i] = rw_to_code(ch[3][i], A.bl[3], A.white) | (rw_to_code(ch[2][i], A.bl[2], A.white) << 16);
    }
    const size_t W2 = 2 * (size_t)w;
    uint16_t* dst = A.out + ((size_t)b * 2 * h + 2 * (size_t)y) * W2 + 2 * (size_t)x;
    rw_store_pairs<V>(dst, top);
    rw_store_pairs<V>(dst + W2, bottom);
}

dim3 rw_grid(size_t threads, int B) { return dim3((unsigned)((threads + RW_THREADS - 1) / RW_THREADS), (unsigned)B); }

int rw_check_levels(const char* who, float black, float white) {
    ND_REQUIRE(white > black && black >= 0.0f && white <= 65535.0f, ND_E_BADARG, "%s: need 0 <= black < white <= 65535", who);
    return 0;
}

int rw_check_frames(const char* who, const void* frames, int N, int H2, int W2, int B, int h, int w) {
    ND_REQUIRE(N > 0 && H2 > 0 && W2 > 0 && h > 0 && w > 0 && B > 0 && B <= 65535, ND_E_BADARG, "%s: N, H2, W2, h, w and B (<= 65535) must be positive",
               who);
    ND_REQUIRE(H2 % 2 == 0 && W2 % 2 == 0, ND_E_SHAPE, "%s: a Bayer frame has even sides; got %d x %d", who, H2, W2);
    ND_REQUIRE(h <= H2 / 2 && w <= W2 / 2, ND_E_SHAPE, "%s: the window %d x %d does not fit the packed frame %d x %d", who, h, w, H2 / 2, W2 / 2);
    ND_REQUIRE((int64_t)4 * h * w < (1ll << 32), ND_E_SHAPE, "%s: 4 * h * w must fit the 32-bit element counter", who);
    ND_REQUIRE(((uintptr_t)frames & 3u) == 0, ND_E_ALIGN, "%s: frames must be 4-byte aligned", who);
    return 0;
}

struct DiffusionArgs {
    const uint16_t* frames;             // null when only coord is asked for
    const nd_raw_sample* table;         // [B]
    float* noise;  float* noisy;  float* clean;  float* coord;      // each may be null: neither computed nor written
    int N, H, W, h, w;                  // H, W: the packed frame
    float black, white;
};

// The diffusion sets' sample (dataloader/dataset.py SonyTrainDataset / NoiseImageGenerationDataset / GenDarkFrameDataset): noisy and clean from the
// short and the long exposure of one window, their difference, and the window's coordinates within the whole frame.  Threads as in raw_pack_kernel:
// thread i of block row blockIdx.y = sample b takes packed columns V (i mod (w / V)) .. + V - 1 of output row i / (w / V), all four channels.
template <int V>
__global__ __launch_bounds__(RW_THREADS) void raw_diffusion_kernel(DiffusionArgs A) {
    const int b = blockIdx.y;
    const int h = A.h, w = A.w, wv = w / V;
    const size_t t = (size_t)blockIdx.x * RW_THREADS + threadIdx.x;
    if (t >= (size_t)h * wv) return;
    const int y = (int)(t / wv), x = (int)(t - (size_t)y * wv) * V;
    const nd_raw_sample s = A.table[b];
    const size_t plane = (size_t)h * w;
    const size_t px = (size_t)y * w + x;
    const size_t o4 = (size_t)b * 4 * plane + px, o2 = (size_t)b * 2 * plane + px;
    const bool need_short = A.noise || A.noisy, need_long = A.noise || A.clean;

    // rw_window_ok's frame test is applied to each frame this launch reads, and to none when it reads none
    nd_raw_sample win = s;
    bool ok = true;
    if (need_long) {
        win.frame = s.frame_clean;
        ok = rw_window_ok(win, A.N, A.H, A.W, h, w);
    }
    win.frame = need_short ? s.frame : 0;
    ok = ok && rw_window_ok(win, need_short ? A.N : 1, A.H, A.W, h, w);
    if (!ok) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (A.noise) rw_store_nan<V>(A.noise + o4 + c * plane);
            if (A.noisy) rw_store_nan<V>(A.noisy + o4 + c * plane);
            if (A.clean) rw_store_nan<V>(A.clean + o4 + c * plane);
            if (c < 2 && A.coord) rw_store_nan<V>(A.coord + o2 + c * plane);
        }
        return;
    }
    const int Y = s.y0 + y, X = s.x0 + x;
    const size_t W2 = 2 * (size_t)A.W;
    const size_t cell = (2 * (size_t)Y) * W2 + 2 * (size_t)X;
    uint32_t st[V], sb[V], lt[V], lb[V];
#pragma unroll
    for (int i = 0; i < V; ++i) st[i] = sb[i] = lt[i] = lb[i] = 0u;
    if (need_short) {
        const uint16_t* src = A.frames + (size_t)s.frame * (2 * (size_t)A.H) * W2 + cell;
        rw_load_pairs<V>(src, st);
        rw_load_pairs<V>(src + W2, sb);
    }
    if (need_long) {
        const uint16_t* src = A.frames + (size_t)s.frame_clean * (2 * (size_t)A.H) * W2 + cell;
        rw_load_pairs<V>(src, lt);
        rw_load_pairs<V>(src + W2, lb);
    }
    const float black = A.black, wb = A.white - black;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float ny[V], cl[V];
#pragma unroll
        for (int i = 0; i < V; ++i) ny[i] = cl[i] = 0.0f;
        if (need_short) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float sv = rw_code(st[i], sb[i], c) - black;
                sv = sv < 0.0f ? 0.0f : sv;
                sv = sv / wb;
                ny[i] = nd_clip(sv * s.ratio, 0.0f, 1.0f);
            }
        }
        if (need_long) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float g = rw_code(lt[i], lb[i], c) - black;
                cl[i] = (g < 0.0f ? 0.0f : g) / wb;                             // gt_norm is not clipped: a code above white gives more than 1
            }
        }
        if (A.noise) {
            float nz[V];
#pragma unroll
            for (int i = 0; i < V; ++i) nz[i] = ny[i] - cl[i];
            nd_store_v<V>(A.noise + o4 + c * plane, nz);
        }
        if (A.noisy) nd_store_v<V>(A.noisy + o4 + c * plane, ny);
        if (A.clean) nd_store_v<V>(A.clean + o4 + c * plane, cl);
    }
    if (A.coord) {                                                              // make_coord(H, W, rescale=True): row, then column, over the whole frame
        float cy[V], cx[V];
        const float row = (float)Y / (float)(A.H - 1), wm = (float)(A.W - 1);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            cy[i] = row;
            cx[i] = (float)(X + i) / wm;
        }
        nd_store_v<V>(A.coord + o2, cy);
        nd_store_v<V>(A.coord + o2 + plane, cx);
    }
}

}  // namespace

extern "C" int nd_raw_pack_u16_f32(const uint16_t* frames, int N, int H2, int W2, const float* ds_k_high, const float* ds_b_high,
                                   const float* ds_k_low, const float* ds_b_low, int map_h, int map_w, const nd_raw_sample* table, int mode, int flags,
                                   float black, float white, float* out, float* clean_out, int B, int h, int w, void* stream) {
    const char* who = "nd_raw_pack_u16_f32";
    ND_REQUIRE(frames && table && out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE(mode == ND_RAW_PACK || mode == ND_RAW_PACK_SHADED || mode == ND_RAW_TRAIN_REAL, ND_E_BADARG, "%s: unknown mode %d", who, mode);
    ND_REQUIRE((flags & ~(ND_RAW_RESCALE | ND_RAW_CLIP)) == 0, ND_E_BADARG, "%s: unknown flags %d", who, flags);
    ND_REQUIRE((clean_out != nullptr) == (mode == ND_RAW_TRAIN_REAL), ND_E_BADARG, "%s: clean_out goes with ND_RAW_TRAIN_REAL and with it alone", who);
    const int nmaps = (ds_k_high != nullptr) + (ds_b_high != nullptr) + (ds_k_low != nullptr) + (ds_b_low != nullptr);
    ND_REQUIRE(nmaps == 0 || nmaps == 4, ND_E_BADARG, "%s: give all four dark-shading planes or none", who);
    ND_REQUIRE(nmaps == 4 || mode != ND_RAW_PACK_SHADED, ND_E_BADARG, "%s: ND_RAW_PACK_SHADED needs the dark-shading planes", who);
    ND_REQUIRE(nmaps == 0 || mode != ND_RAW_PACK, ND_E_BADARG, "%s: ND_RAW_PACK takes no dark-shading planes", who);
    if (int r = rw_check_levels(who, black, white)) return r;
    if (int r = rw_check_frames(who, frames, N, H2, W2, B, h, w)) return r;
    ND_REQUIRE(nmaps == 0 || (map_h >= h && map_w >= w), ND_E_SHAPE, "%s: shading planes %d x %d are smaller than the window", who, map_h, map_w);
    ND_REQUIRE(((uintptr_t)table & 7u) == 0 && (((uintptr_t)ds_k_high | (uintptr_t)ds_b_high | (uintptr_t)ds_k_low | (uintptr_t)ds_b_low) & 3u) == 0,
               ND_E_ALIGN, "%s: the table must be 8-byte aligned, the planes 4-byte", who);
    const uintptr_t out_bits = (uintptr_t)out | (uintptr_t)clean_out;
    ND_REQUIRE((out_bits & 3u) == 0, ND_E_ALIGN, "%s: out and clean_out must be 4-byte aligned", who);
    RawArgs A;
    A.frames = frames;
    A.ds[0] = ds_k_high;  A.ds[1] = ds_b_high;  A.ds[2] = ds_k_low;  A.ds[3] = ds_b_low;
    A.table = table;  A.out = out;  A.clean_out = clean_out;
    A.N = N;  A.H = H2 / 2;  A.W = W2 / 2;  A.Hm = map_h;  A.Wm = map_w;  A.h = h;  A.w = w;
    A.flags = flags;  A.black = black;  A.white = white;
    const int V = rw_width(w, out_bits);
    rw_dispatch(V, [&](auto v) {
        const auto kernel = mode == ND_RAW_PACK          ? raw_pack_kernel<v(), ND_RAW_PACK>
                            : mode == ND_RAW_PACK_SHADED ? raw_pack_kernel<v(), ND_RAW_PACK_SHADED>
                                                         : raw_pack_kernel<v(), ND_RAW_TRAIN_REAL>;
        hipLaunchKernelGGL(kernel, rw_grid((size_t)h * (w / V), B), dim3(RW_THREADS), 0, (hipStream_t)stream, A);
    });
    return nd_launch_status(who);
}

extern "C" int nd_raw_poisson_gaussian_f32(const uint16_t* frames, int N, int H2, int W2, const nd_raw_sample* table, const int64_t* rng,
                                           uint64_t seed, int64_t first_sample, int32_t draw, const float* counts_in, const float* normals_in,
                                           float* counts_out, float* normals_out, float black, float white, float* noisy, float* clean_out, int B,
                                           int h, int w, void* stream) {
    const char* who = "nd_raw_poisson_gaussian_f32";
    ND_REQUIRE(frames && table && noisy && clean_out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE(draw >= 0, ND_E_BADARG, "%s: draw index %d is negative", who, draw);
    if (int r = rw_check_levels(who, black, white)) return r;
    if (int r = rw_check_frames(who, frames, N, H2, W2, B, h, w)) return r;
    ND_REQUIRE(((uintptr_t)table & 7u) == 0 && ((uintptr_t)rng & 7u) == 0, ND_E_ALIGN, "%s: table and rng must be 8-byte aligned", who);
    const uintptr_t bits = (uintptr_t)noisy | (uintptr_t)clean_out | (uintptr_t)counts_out | (uintptr_t)normals_out | (uintptr_t)counts_in |
                           (uintptr_t)normals_in;
    ND_REQUIRE((bits & 3u) == 0, ND_E_ALIGN, "%s: noisy, clean_out, counts and normals must be 4-byte aligned", who);
    PgArgs A;
    A.frames = frames;  A.table = table;  A.rng = rng;  A.counts_in = counts_in;  A.normals_in = normals_in;  A.counts_out = counts_out;
    A.normals_out = normals_out;  A.noisy = noisy;  A.clean_out = clean_out;
    A.seed = seed;  A.first_sample = first_sample;  A.draw = draw;
    A.N = N;  A.H = H2 / 2;  A.W = W2 / 2;  A.h = h;  A.w = w;  A.black = black;  A.white = white;
    const uintptr_t out_bits = (uintptr_t)noisy | (uintptr_t)clean_out | (uintptr_t)counts_out | (uintptr_t)normals_out;
    const int V = rw_width(w, out_bits);
    rw_dispatch(V, [&](auto v) { hipLaunchKernelGGL(raw_pg_kernel<v()>, rw_grid((size_t)4 * h * w / V, B), dim3(RW_THREADS), 0, (hipStream_t)stream, A); });
    return nd_launch_status(who);
}

extern "C" int nd_raw_to_bayer_u16(const float* img, uint16_t* out, const int32_t* bl, int white, int B, int h, int w, void* stream) {
    const char* who = "nd_raw_to_bayer_u16";
    ND_REQUIRE(img && out && bl, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0, ND_E_BADARG, "%s: B (<= 65535), h and w must be positive", who);
    ND_REQUIRE(white > 0 && white <= 65535, ND_E_BADARG, "%s: white %d is not a uint16 code", who, white);
    for (int c = 0; c < 4; ++c)
        ND_REQUIRE(bl[c] >= 0 && bl[c] <= white, ND_E_BADARG, "%s: black level %d of channel %d is outside [0, white = %d]", who, bl[c], c, white);
    ND_REQUIRE(((uintptr_t)img & 3u) == 0 && ((uintptr_t)out & 3u) == 0, ND_E_ALIGN, "%s: img and out must be 4-byte aligned", who);
    BayerArgs A;
    A.img = img;  A.out = out;  A.white = white;  A.h = h;  A.w = w;
    for (int c = 0; c < 4; ++c) A.bl[c] = bl[c];
    const int V = rw_width(w, (uintptr_t)out);
    rw_dispatch(V, [&](auto v) { hipLaunchKernelGGL(raw_bayer_kernel<v()>, rw_grid((size_t)h * (w / V), B), dim3(RW_THREADS), 0, (hipStream_t)stream, A); });
    return nd_launch_status(who);
}

extern "C" int nd_raw_diffusion_batch_f32(const uint16_t* frames, int N, int H2, int W2, const nd_raw_sample* table, float black, float white,
                                          float* noise, float* noisy, float* clean, float* coord, int B, int h, int w, void* stream) {
    const char* who = "nd_raw_diffusion_batch_f32";
    const bool reads = noise || noisy || clean;
    ND_REQUIRE(table, ND_E_BADARG, "%s: null table", who);
    ND_REQUIRE(reads || coord, ND_E_BADARG, "%s: give at least one of noise, noisy, clean and coord", who);
    ND_REQUIRE(frames || !reads, ND_E_BADARG, "%s: noise, noisy and clean need the frames; only coord is made without them", who);
    ND_REQUIRE(!reads || N > 0, ND_E_BADARG, "%s: N must be positive", who);
    ND_REQUIRE(H2 > 0 && W2 > 0 && H2 % 2 == 0 && W2 % 2 == 0, ND_E_BADARG, "%s: a Bayer frame has even, positive sides; got %d x %d", who, H2, W2);
    ND_REQUIRE(H2 >= 4 && W2 >= 4, ND_E_BADARG, "%s: the coordinates divide by H - 1 and W - 1: the packed frame %d x %d needs sides of 2 at least", who,
               H2 / 2, W2 / 2);
    ND_REQUIRE(h > 0 && w > 0 && B > 0 && B <= 65535, ND_E_BADARG, "%s: h, w and B (<= 65535) must be positive", who);
    ND_REQUIRE(h <= H2 / 2 && w <= W2 / 2, ND_E_BADARG, "%s: the window %d x %d does not fit the packed frame %d x %d", who, h, w, H2 / 2, W2 / 2);
    if (int r = rw_check_levels(who, black, white)) return r;
    const uintptr_t out_bits = (uintptr_t)noise | (uintptr_t)noisy | (uintptr_t)clean | (uintptr_t)coord;
    ND_REQUIRE(((uintptr_t)frames & 3u) == 0 && (out_bits & 3u) == 0 && ((uintptr_t)table & 7u) == 0, ND_E_BADARG,
               "%s: frames and outputs must be 4-byte aligned, the table 8-byte", who);
    DiffusionArgs A;
    A.frames = frames;  A.table = table;  A.noise = noise;  A.noisy = noisy;  A.clean = clean;  A.coord = coord;
    A.N = reads ? N : 0;  A.H = H2 / 2;  A.W = W2 / 2;  A.h = h;  A.w = w;  A.black = black;  A.white = white;
    const int V = rw_width(w, out_bits);
    rw_dispatch(V, [&](auto v) { hipLaunchKernelGGL(raw_diffusion_kernel<v()>, rw_grid((size_t)h * (w / V), B), dim3(RW_THREADS), 0, (hipStream_t)stream, A); });
    return nd_launch_status(who);
}
