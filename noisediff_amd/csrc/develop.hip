// develop.hip -- a packed RAW frame to an sRGB picture in one launch: LibRaw's develop steps as test_denoising.py's postprocess_bayer asks for
// them (use_camera_wb, no_auto_bright, half_size or the bilinear demosaic, output_bps 8 or 16), restated step by step in include/noisediff_hip.h.
//
//   develop_half_kernel<T, V, F32>   packed pixel (Y, X) -> one output pixel: R = s0, G = (s1 + s3) >> 1, B = s2
//   develop_full_kernel<T, Q, F32>   every site of the 2h x 2w mosaic -> one output pixel, missing colours by the bilinear rule
//
// T: uint8_t or uint16_t output; F32: the source is packed fp32 (written as codes by nd_raw_to_bayer_u16's rule first) or a uint16 mosaic.
// The scaling and the matrix are single fp32 operations in the written order: contraction to fma is off for this file, so numpy repeats
// every byte.
//
// Half size has raw_pack_kernel's shape: a thread takes V = 4, 2 or 1 consecutive packed columns (the host chooses, so w % V = 0 and there is
// no tail), reads each source plane (or Bayer row) with the widest load the address allows and writes its 3 V output values as dwords where
// they fill whole ones.  Full resolution: a workgroup stages the scaled values s of its DF_TH x DF_TW cells as uint16 with a one-site halo in
// LDS; a halo site outside the FRAME holds 0 and is left out of the count, which comes from the site's coordinates; a thread then forms the
// 2 x 2 sites of Q = 2 or 1 cells, so each of its two stores is one run of bytes in one output row.
//
// The curve is read three times per pixel.  One workgroup per CU (fewer for a small launch) first copies it into LDS as output values -- 64 KiB
// of bytes for 8-bit output, 128 KiB for 16-bit -- and then walks the thread items or tiles of the launch: the measured choice (DESIGN.md
// section 20).  -DND_DEVELOP_CURVE_LDS=0 builds the other form for tools/render_bench.py: a thread item or tile per thread or workgroup, the
// curve read from its 128 KiB table in global memory through L2.
#include "nd_common.h"
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

#include "raw_codes.h"

#ifndef ND_DEVELOP_CURVE_LDS
#define ND_DEVELOP_CURVE_LDS 1
#endif

namespace {

constexpr int DV_THREADS = ND_DEVELOP_CURVE_LDS ? 1024 : 256;
constexpr int DF_TH = ND_DEVELOP_CURVE_LDS ? 32 : 16, DF_TW = ND_DEVELOP_CURVE_LDS ? 64 : 32;      // cells of a full-resolution tile: two per thread
constexpr int DF_PITCH = 2 * DF_TW + 2;                                 // sites of a tile row with its halo: 33 or 65 dwords, an odd count
constexpr size_t DF_TILE_BYTES = (size_t)(2 * DF_TH + 2) * DF_PITCH * sizeof(uint16_t);

struct DevArgs {
    const float* f32;                   // [B][4][H][W], or null
    const uint16_t* u16;                // [B][2H][2W], or null
    const uint16_t* curve;              // [65536]
    void* out;
    int black[4];
    int white;
    float scale[4];
    float m[9];
    int B, H, W, x0, y0, h, w;
};

// the curve as the kernels read it: the table in global memory, or a workgroup's copy in LDS holding output values already
template <class T>
struct CurveGlobal {
    const uint16_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t u) const { return sizeof(T) == 1 ? (uint32_t)(p[u] >> 8) : (uint32_t)p[u]; }
};
template <class T>
struct CurveLds {
    const T* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t u) const { return p[u]; }
};

// v = max(code - black, 0); s = min(trunc(fl32(v) * scale_mul), 65535)
__device__ __forceinline__ uint32_t dv_scale(uint32_t code, int black, float mul) {
    const int v = (int)code - black;
    const float p = (float)(v < 0 ? 0 : v) * mul;
    return p < 65535.0f ? (uint32_t)p : 65535u;
}

// the four s of a cell from its codes (two words: rows 2Y and 2Y + 1, the even column in the low half)
__device__ __forceinline__ void dv_cell_u16(const DevArgs& A, uint32_t top, uint32_t bottom, uint32_t (&s)[4]) {
    s[0] = dv_scale(top & 0xFFFFu, A.black[0], A.scale[0]);
    s[1] = dv_scale(top >> 16, A.black[1], A.scale[1]);
    s[2] = dv_scale(bottom >> 16, A.black[2], A.scale[2]);
    s[3] = dv_scale(bottom & 0xFFFFu, A.black[3], A.scale[3]);
}

// o = 0 + R m0; o = o + G m1; o = o + B m2; u = clip((int)o, 0, 65535), the clip done on the float so that no cast leaves int's range
__device__ __forceinline__ uint32_t dv_mix(const float* m, float R, float G, float B) {
    float o = 0.0f + R * m[0];
    o = o + G * m[1];
    o = o + B * m[2];
    return o >= 65535.0f ? 65535u : (o > 0.0f ? (uint32_t)o : 0u);
}

template <class C>
__device__ __forceinline__ void dv_pixel(const DevArgs& A, const C& curve, uint32_t R, uint32_t G, uint32_t B, uint32_t* e) {
    const float r = (float)R, g = (float)G, b = (float)B;
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = curve(dv_mix(A.m + 3 * k, r, g, b));
}

// N output values to p as dwords where they fill whole ones, else as 16-bit words, else as bytes; p is aligned to the unit used (the host checks)
template <class T, int N>
__device__ __forceinline__ void dv_store(T* p, const uint32_t (&e)[N]) {
    constexpr int BYTES = N * (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    if constexpr (BYTES % 4 == 0) {
        constexpr int PER = 4 / (int)sizeof(T);
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < BYTES / 4; ++i) {
            uint32_t wd = 0u;
#pragma unroll
            for (int j = 0; j < PER; ++j) wd |= e[i * PER + j] << (BITS * j);
            q[i] = wd;
        }
    } else if constexpr (sizeof(T) == 1 && BYTES % 2 == 0) {
        uint16_t* q = reinterpret_cast<uint16_t*>(p);
#pragma unroll
        for (int i = 0; i < BYTES / 2; ++i) q[i] = (uint16_t)(e[2 * i] | (e[2 * i + 1] << 8));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = (T)e[i];
    }
}

// Thread item t of image b: packed columns V (t mod (w / V)) .. + V - 1 of window row t / (w / V).
template <class T, int V, bool F32, class C>
__device__ __forceinline__ void dv_half_item(const DevArgs& A, const C& curve, size_t t, int b) {
    const int wv = A.w / V;
    const int y = (int)(t / wv), x = (int)(t - (size_t)y * wv) * V;
    const int Y = A.y0 + y, X = A.x0 + x;
    uint32_t s[V][4];
    if constexpr (F32) {
        const size_t plane = (size_t)A.H * A.W;
        const float* src = A.f32 + (size_t)b * 4 * plane + (size_t)Y * A.W + X;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float ch[V];
            nd_load_v<V>(src + c * plane, ch);
#pragma unroll
            for (int i = 0; i < V; ++i) s[i][c] = dv_scale(rw_to_code(ch[i], A.black[c], A.white), A.black[c], A.scale[c]);
        }
    } else {
        const size_t W2 = 2 * (size_t)A.W;
        const uint16_t* src = A.u16 + ((size_t)b * 2 * A.H + 2 * (size_t)Y) * W2 + 2 * (size_t)X;
        uint32_t top[V], bottom[V];
        rw_load_pairs<V>(src, top);
        rw_load_pairs<V>(src + W2, bottom);
#pragma unroll
        for (int i = 0; i < V; ++i) dv_cell_u16(A, top[i], bottom[i], s[i]);
    }
    uint32_t e[3 * V];
#pragma unroll
    for (int i = 0; i < V; ++i) dv_pixel(A, curve, s[i][0], (s[i][1] + s[i][3]) >> 1, s[i][2], e + 3 * i);
    dv_store<T, 3 * V>(static_cast<T*>(A.out) + (((size_t)b * A.h + y) * A.w + x) * 3, e);
}

// floor(sum / count) over the 1 to 4 in-frame sites of a colour
__device__ __forceinline__ uint32_t dv_mean(uint32_t sum, int count) {
    return count == 4 ? sum >> 2 : (count == 2 ? sum >> 1 : (count == 3 ? sum / 3u : sum));
}

// Tile (ty, tx) of image b: DF_TH x DF_TW cells of the window from cell (ty DF_TH, tx DF_TW).  Site (i, j) of `tile` is mosaic site
// (2 (y0 + ty DF_TH) - 1 + i, 2 (x0 + tx DF_TW) - 1 + j) of the frame; the caller's barrier separates two tiles of a walking workgroup.
template <class T, int Q, bool F32, class C>
__device__ __forceinline__ void dv_full_tile(const DevArgs& A, const C& curve, uint16_t* tile, int b, int ty, int tx) {
    const int cy0 = A.y0 + ty * DF_TH, cx0 = A.x0 + tx * DF_TW;
    const size_t plane = (size_t)A.H * A.W, W2 = 2 * (size_t)A.W;
    for (int i = threadIdx.x; i < (DF_TH + 2) * (DF_TW + 2); i += DV_THREADS) {          // the tile's cells and a ring of one cell around them
        const int iy = i / (DF_TW + 2), ix = i - iy * (DF_TW + 2);
        const int Y = cy0 - 1 + iy, X = cx0 - 1 + ix;
        uint32_t s[4] = {0u, 0u, 0u, 0u};                                                // outside the frame: absent
        if (Y >= 0 && Y < A.H && X >= 0 && X < A.W) {
            if constexpr (F32) {
                const float* src = A.f32 + (size_t)b * 4 * plane + (size_t)Y * A.W + X;
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = dv_scale(rw_to_code(src[c * plane], A.black[c], A.white), A.black[c], A.scale[c]);
            } else {
                const uint16_t* src = A.u16 + ((size_t)b * 2 * A.H + 2 * (size_t)Y) * W2 + 2 * (size_t)X;
                dv_cell_u16(A, *reinterpret_cast<const uint32_t*>(src), *reinterpret_cast<const uint32_t*>(src + W2), s);
            }
        }
        const int lr = 2 * iy - 1, lc = 2 * ix - 1;                                      // of the ring's cells only the sites next to the tile are kept
        if (lr >= 0) {
            if (lc >= 0) tile[lr * DF_PITCH + lc] = (uint16_t)s[0];
            if (lc + 1 < DF_PITCH) tile[lr * DF_PITCH + lc + 1] = (uint16_t)s[1];
        }
        if (lr + 1 < 2 * DF_TH + 2) {
            if (lc >= 0) tile[(lr + 1) * DF_PITCH + lc] = (uint16_t)s[3];
            if (lc + 1 < DF_PITCH) tile[(lr + 1) * DF_PITCH + lc + 1] = (uint16_t)s[2];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DF_TH * (DF_TW / Q); i += DV_THREADS) {
        const int cy = i / (DF_TW / Q), cx = (i - cy * (DF_TW / Q)) * Q;
        const int y = ty * DF_TH + cy, x = tx * DF_TW + cx;
        if (y >= A.h || x >= A.w) continue;
        const int Y = A.y0 + y;
        const int up = Y > 0, dn = Y < A.H - 1;
        uint32_t top[6 * Q], bot[6 * Q];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const int X = A.x0 + x + k;
            const int lf = X > 0, rt = X < A.W - 1;
            const uint16_t* p = tile + (2 * cy + 1) * DF_PITCH + 2 * (cx + k) + 1;       // the cell's R site; P(dr, dc) below is p[dr * DF_PITCH + dc]
            uint32_t P[4][4];
#pragma unroll
            for (int dr = 0; dr < 4; ++dr)
#pragma unroll
                for (int dc = 0; dc < 4; ++dc) P[dr][dc] = p[(dr - 1) * DF_PITCH + dc - 1];
            // R site (2Y, 2X): green on its four sides, blue on its four corners
            dv_pixel(A, curve, P[1][1], dv_mean(P[0][1] + P[2][1] + P[1][0] + P[1][2], 2 + up + lf),
                     dv_mean(P[0][0] + P[0][2] + P[2][0] + P[2][2], 1 + up + lf + (up & lf)), top + 6 * k);
            // G1 site (2Y, 2X + 1): red left and right, blue above and below
            dv_pixel(A, curve, dv_mean(P[1][1] + P[1][3], 1 + rt), P[1][2], dv_mean(P[0][2] + P[2][2], 1 + up), top + 6 * k + 3);
            // G2 site (2Y + 1, 2X): red above and below, blue left and right
            dv_pixel(A, curve, dv_mean(P[1][1] + P[3][1], 1 + dn), P[2][1], dv_mean(P[2][0] + P[2][2], 1 + lf), bot + 6 * k);
            // B site (2Y + 1, 2X + 1): green on its four sides, red on its four corners
            dv_pixel(A, curve, dv_mean(P[1][1] + P[1][3] + P[3][1] + P[3][3], 1 + dn + rt + (dn & rt)),
                     dv_mean(P[1][2] + P[3][2] + P[2][1] + P[2][3], 2 + dn + rt), P[2][2], bot + 6 * k + 3);
        }
        T* dst = static_cast<T*>(A.out) + (((size_t)b * 2 * A.h + 2 * (size_t)y) * (2 * (size_t)A.w) + 2 * (size_t)x) * 3;
        dv_store<T, 6 * Q>(dst, top);
        dv_store<T, 6 * Q>(dst + 2 * (size_t)A.w * 3, bot);
    }
}

extern __shared__ __align__(16) unsigned char dv_lds[];

#if !ND_DEVELOP_CURVE_LDS

template <class T, int V, bool F32>
__global__ __launch_bounds__(DV_THREADS) void develop_half_kernel(DevArgs A) {
    const size_t t = (size_t)blockIdx.x * DV_THREADS + threadIdx.x;
    if (t >= (size_t)A.h * (A.w / V)) return;
    dv_half_item<T, V, F32>(A, CurveGlobal<T>{A.curve}, t, blockIdx.y);
}

template <class T, int Q, bool F32>
__global__ __launch_bounds__(DV_THREADS) void develop_full_kernel(DevArgs A) {
    dv_full_tile<T, Q, F32>(A, CurveGlobal<T>{A.curve}, reinterpret_cast<uint16_t*>(dv_lds), blockIdx.z, blockIdx.y, blockIdx.x);
}

constexpr size_t DV_CURVE_BYTES = 0;

#else

constexpr int DV_CURVE = 65536;
constexpr size_t DV_CURVE_BYTES = 2 * DV_CURVE;        // reserved for either T: one attribute per kernel

// the workgroup's copy of the curve as output values: eight codes per thread and round
template <class T>
__device__ __forceinline__ const T* dv_curve_to_lds(const uint16_t* curve) {
    T* lds = reinterpret_cast<T*>(dv_lds);
    for (int i = threadIdx.x; i < DV_CURVE / 8; i += DV_THREADS) {
        const uint4 t = reinterpret_cast<const uint4*>(curve)[i];
        if constexpr (sizeof(T) == 2) {
            reinterpret_cast<uint4*>(lds)[i] = t;
        } else {
            const uint32_t wd[4] = {t.x, t.y, t.z, t.w};
            uint2 o;
            o.x = ((wd[0] >> 8) & 0xFFu) | ((wd[0] >> 24) << 8) | (((wd[1] >> 8) & 0xFFu) << 16) | ((wd[1] >> 24) << 24);
            o.y = ((wd[2] >> 8) & 0xFFu) | ((wd[2] >> 24) << 8) | (((wd[3] >> 8) & 0xFFu) << 16) | ((wd[3] >> 24) << 24);
            reinterpret_cast<uint2*>(lds)[i] = o;
        }
    }
    __syncthreads();
    return lds;
}

template <class T, int V, bool F32>
__global__ __launch_bounds__(DV_THREADS) void develop_half_kernel(DevArgs A) {
    const CurveLds<T> curve{dv_curve_to_lds<T>(A.curve)};
    const size_t n = (size_t)A.h * (A.w / V);
    for (int b = 0; b < A.B; ++b)
        for (size_t t = (size_t)blockIdx.x * DV_THREADS + threadIdx.x; t < n; t += (size_t)gridDim.x * DV_THREADS) dv_half_item<T, V, F32>(A, curve, t, b);
}

template <class T, int Q, bool F32>
__global__ __launch_bounds__(DV_THREADS) void develop_full_kernel(DevArgs A) {
    const CurveLds<T> curve{dv_curve_to_lds<T>(A.curve)};
    const int tiles_x = (A.w + DF_TW - 1) / DF_TW, tiles = tiles_x * ((A.h + DF_TH - 1) / DF_TH);
    for (int i = blockIdx.x; i < A.B * tiles; i += gridDim.x) {
        const int b = i / tiles, r = i - b * tiles;
        dv_full_tile<T, Q, F32>(A, curve, reinterpret_cast<uint16_t*>(dv_lds + DV_CURVE_BYTES), b, r / tiles_x, r % tiles_x);
        __syncthreads();
    }
}

#endif

template <class T, int V, bool F32>
int dv_launch(bool full, const DevArgs& A, hipStream_t st) {
    const void* kernel = full ? (const void*)develop_full_kernel<T, (V >= 2 ? 2 : 1), F32> : (const void*)develop_half_kernel<T, V, F32>;
    const size_t lds = DV_CURVE_BYTES + (full ? DF_TILE_BYTES : 0);
    dim3 grid = full ? dim3(nd_cdiv(A.w, DF_TW), nd_cdiv(A.h, DF_TH), A.B) : dim3((unsigned)(((size_t)A.h * (A.w / V) + DV_THREADS - 1) / DV_THREADS), A.B);
    if (ND_DEVELOP_CURVE_LDS) {
        static nd_device_once once[2];
        if (int r = nd_reserve_lds(once[full], kernel, lds, "nd_raw_develop")) return r;
        const size_t work = full ? (size_t)grid.x * grid.y * grid.z : grid.x;            // tiles, or workgroups' worth of thread items per image
        grid = dim3((unsigned)(work < (size_t)nd_device_cus() ? work : (size_t)nd_device_cus()));
    }
    void* args[] = {const_cast<DevArgs*>(&A)};
    const hipError_t e = hipLaunchKernel(kernel, grid, dim3(DV_THREADS), args, lds, st);
    if (e != hipSuccess) {
        nd_set_error("nd_raw_develop: %s", hipGetErrorString(e));
        return (int)e;
    }
    return nd_launch_status("nd_raw_develop");
}

template <class T, bool F32>
int dv_launch_width(bool full, int V, const DevArgs& A, hipStream_t st) {
    return V == 4 ? dv_launch<T, 4, F32>(full, A, st) : (V == 2 ? dv_launch<T, 2, F32>(full, A, st) : dv_launch<T, 1, F32>(full, A, st));
}

}  // namespace

extern "C" int nd_raw_develop(const float* src_f32, const uint16_t* src_u16, int B, int H, int W, const nd_develop_params* p, const uint16_t* curve,
                              void* out, int h, int w, void* stream) {
    const char* who = "nd_raw_develop";
    ND_REQUIRE(p && curve && out, ND_E_BADARG, "%s: null pointer", who);
    ND_REQUIRE((src_f32 != nullptr) != (src_u16 != nullptr), ND_E_BADARG, "%s: give the fp32 source or the uint16 source, one of them", who);
    ND_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && h > 0 && w > 0, ND_E_BADARG, "%s: B (<= 65535), H, W, h and w must be positive", who);
    ND_REQUIRE(H <= (1 << 24) && W <= (1 << 24), ND_E_SHAPE, "%s: a packed frame side is 2^24 at most; got %d x %d", who, H, W);
    ND_REQUIRE((p->bps == 8 || p->bps == 16) && (p->full == 0 || p->full == 1), ND_E_BADARG, "%s: bps is 8 or 16 and full 0 or 1; got %d, %d", who,
               p->bps, p->full);
    ND_REQUIRE(p->white > 0 && p->white <= 65535, ND_E_BADARG, "%s: white %d is not a uint16 code", who, p->white);
    for (int c = 0; c < 4; ++c) {
        ND_REQUIRE(p->black[c] >= 0 && p->black[c] <= p->white, ND_E_BADARG, "%s: black level %d of channel %d is outside [0, white = %d]", who,
                   p->black[c], c, p->white);
        ND_REQUIRE(std::isfinite(p->scale_mul[c]) && p->scale_mul[c] >= 0.0f, ND_E_BADARG, "%s: scale_mul[%d] must be finite and not negative", who, c);
    }
    for (int i = 0; i < 9; ++i) ND_REQUIRE(std::isfinite(p->rgb_cam[i]), ND_E_BADARG, "%s: rgb_cam[%d] is not finite", who, i);
    ND_REQUIRE(p->x0 >= 0 && p->y0 >= 0 && p->x0 <= W - w && p->y0 <= H - h, ND_E_SHAPE, "%s: the window %d x %d at (%d, %d) leaves the packed frame %d x %d",
               who, h, w, p->x0, p->y0, H, W);
    ND_REQUIRE(!p->full || nd_cdiv(h, DF_TH) <= 65535, ND_E_SHAPE, "%s: a full-resolution window has at most %d rows", who, 65535 * DF_TH);
    ND_REQUIRE(!p->full || (int64_t)B * nd_cdiv(h, DF_TH) * nd_cdiv(w, DF_TW) < (1ll << 31), ND_E_SHAPE, "%s: the tiles of a launch are counted in 32 bits", who);
    ND_REQUIRE((((uintptr_t)src_f32 | (uintptr_t)src_u16 | (uintptr_t)out) & 3u) == 0 && nd_aligned16(curve), ND_E_ALIGN,
               "%s: the source and out must be 4-byte aligned, the curve 16-byte", who);
    DevArgs A;
    A.f32 = src_f32;  A.u16 = src_u16;  A.curve = curve;  A.out = out;  A.white = p->white;
    for (int c = 0; c < 4; ++c) { A.black[c] = p->black[c];  A.scale[c] = p->scale_mul[c]; }
    for (int i = 0; i < 9; ++i) A.m[i] = p->rgb_cam[i];
    A.B = B;  A.H = H;  A.W = W;  A.x0 = p->x0;  A.y0 = p->y0;  A.h = h;  A.w = w;
    // every store unit of dv_store is aligned with out 4-byte aligned and w % V = 0: an output row, and a thread's offset in it, is a whole number of units
    const int V = w % 4 == 0 ? 4 : (w % 2 == 0 ? 2 : 1);
    const bool full = p->full != 0;
    hipStream_t st = (hipStream_t)stream;
    if (p->bps == 8) return src_f32 ? dv_launch_width<uint8_t, true>(full, V, A, st) : dv_launch_width<uint8_t, false>(full, V, A, st);
    return src_f32 ? dv_launch_width<uint16_t, true>(full, V, A, st) : dv_launch_width<uint16_t, false>(full, V, A, st);
}
