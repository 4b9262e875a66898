// frame.hip -- whole synthetic noisy frames from sampled patches, one launch per batch of patches (nd_frame_assemble).
//
// io.patch_grid overlaps the patches of a frame by a quarter of the crop.  Each packed pixel has ONE owner, the patch in which it lies furthest
// from a patch border (noisediff_amd/frame.py, FrameLayout), so a frame is a scatter of disjoint rectangles: nothing is averaged, no atomics.
// A thread block row blockIdx.y = patch b walks that patch's owned rectangle and writes up to three frame-sized outputs: the noise as sampled,
// the noisy image composed with the long exposure (io.compose_noisy) and the uint16 mosaic of the short exposure.  The arithmetic is listed
// step by step in include/noisediff_hip.h; every fp32 and fp64 operation is one IEEE operation in that order (contraction to fma is off).
//
// Addressing: the OUTPUTS decide the vector width.  A thread takes an aligned run of V = 4, 2 or 1 packed columns of the frame (the widest V
// that W and the outputs' alignment allow, chosen on the host), so its stores are whole 4 V-byte words; the seams between owners fall on any
// column, so the first and the last run of a rectangle's row may be cut and are then done column by column with the same code at V = 1.
// The patch and the long exposure are read by the widest load each address allows (nd_load_v, rw_load_pairs).  No LDS; grid (tiles, B).
#include "nd_common.h"

#pragma clang fp contract(off)

#include "raw_codes.h"

namespace {

constexpr int FR_THREADS = 256;

struct FrameArgs {
    const float* patches;               // [B][4][c][c]
    const uint16_t* frames;             // [N][2H][2W] or null: clean = 0
    const nd_frame_patch* table;        // [B]
    float* noise;  float* noisy;  uint16_t* shrt;                   // each may be null: neither computed nor written
    int N, H, W, c, F;                  // H, W: the packed frame
    int runs;                           // runs of V columns a rectangle's row can touch at most
    float black, white;
};

__device__ __forceinline__ bool fr_row_ok(const nd_frame_patch& s, const FrameArgs& A, bool reads) {
    bool ok = s.frame_out >= 0 && s.frame_out < A.F && s.x0 >= 0 && s.y0 >= 0 && s.x0 <= A.W - A.c && s.y0 <= A.H - A.c;
    ok = ok && s.ax0 >= s.x0 && s.ax0 <= s.ax1 && s.ax1 <= s.x0 + A.c && s.ay0 >= s.y0 && s.ay0 <= s.ay1 && s.ay1 <= s.y0 + A.c;
    if (reads) ok = ok && s.frame_clean >= 0 && s.frame_clean < A.N;
    if (A.shrt) ok = ok && s.ratio > 0.0f && s.ratio <= 3.402823466e+38f;
    return ok;
}

// the code of one composed value at the short exposure: min(trunc(p wb / ratio + black + 0.5), white), NaN -> p = 0
__device__ __forceinline__ uint32_t fr_short_code(float ny, double wb, double ratio, double black, double white) {
    const float p = ny == ny ? ny : 0.0f;
    double t = (double)p * wb;
    t = t / ratio;
    t = t + black;
    t = t + 0.5;
    return t < white ? (uint32_t)t : (uint32_t)white;           // t >= black + 0.5 > 0 for every ratio fr_row_ok lets through
}

// packed columns X .. X + V - 1 of packed row Y of patch b's rectangle, all four channels, every requested output
template <int V>
__device__ __forceinline__ void fr_columns(const FrameArgs& A, const nd_frame_patch& s, int b, int Y, int X, bool reads) {
    const size_t cc = (size_t)A.c * A.c, plane = (size_t)A.H * A.W;
    const float* src = A.patches + (size_t)b * 4 * cc + (size_t)(Y - s.y0) * A.c + (X - s.x0);
    const size_t o = (size_t)s.frame_out * 4 * plane + (size_t)Y * A.W + X;
    const size_t W2 = 2 * (size_t)A.W;
    const bool composed = A.noisy || A.shrt;
    uint32_t top[V], bottom[V];
#pragma unroll
    for (int i = 0; i < V; ++i) top[i] = bottom[i] = 0u;
    if (reads) {
        const uint16_t* lg = A.frames + ((size_t)s.frame_clean * (2 * (size_t)A.H) + 2 * (size_t)Y) * W2 + 2 * (size_t)X;
        rw_load_pairs<V>(lg, top);
        rw_load_pairs<V>(lg + W2, bottom);
    }
    const float black = A.black, wb = A.white - black;
    const double wbd = (double)wb, ratio = (double)s.ratio, blackd = (double)black, whited = (double)A.white;
    uint32_t code[4][V];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        float n[V];
        nd_load_v<V>(src + ch * cc, n);
        if (A.noise) nd_store_v<V>(A.noise + o + ch * plane, n);
        if (composed) {
            float ny[V];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float clean = 0.0f;
                if (reads) {
                    const float g = rw_code(top[i], bottom[i], ch) - black;
                    clean = (g < 0.0f ? 0.0f : g) / wb;                            // not clipped: a code above white gives more than 1
                }
                const float nc = nd_clip(n[i], -1.0f, 1.0f);
                ny[i] = nd_clip(nc + clean, 0.0f, 1.0f);
                if (A.shrt) code[ch][i] = fr_short_code(ny[i], wbd, ratio, blackd, whited);
            }
            if (A.noisy) nd_store_v<V>(A.noisy + o + ch * plane, ny);
        }
    }
    if (A.shrt) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            top[i] = code[0][i] | (code[1][i] << 16);
            bottom[i] = code[3][i] | (code[2][i] << 16);
        }
        uint16_t* dst = A.shrt + ((size_t)s.frame_out * (2 * (size_t)A.H) + 2 * (size_t)Y) * W2 + 2 * (size_t)X;
        rw_store_pairs<V>(dst, top);
        rw_store_pairs<V>(dst + W2, bottom);
    }
}

// Thread i of block row blockIdx.y = patch b takes run i mod runs of row i / runs of the patch's rectangle; run r of a row covers the frame's
// columns V (ax0 / V + r) .. + V - 1, cut to [ax0, ax1).  The grid is sized for a rectangle as large as the patch: the table lives in device
// memory and is not read on the host.
template <int V>
__global__ __launch_bounds__(FR_THREADS) void frame_assemble_kernel(FrameArgs A) {
    const int b = blockIdx.y;
    const size_t t = (size_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (t >= (size_t)A.c * A.runs) return;
    const int ry = (int)(t / A.runs), run = (int)(t - (size_t)ry * A.runs);
    const nd_frame_patch s = A.table[b];
    const bool reads = A.frames && (A.noisy || A.shrt);
    if (!fr_row_ok(s, A, reads)) return;
    if (ry >= s.ay1 - s.ay0) return;
    const int Y = s.ay0 + ry;
    const int X = (s.ax0 / V + run) * V;
    if (X >= s.ax1) return;
    if (X >= s.ax0 && X + V <= s.ax1) {
        fr_columns<V>(A, s, b, Y, X, reads);
        return;
    }
    if constexpr (V > 1) {
        const int first = X < s.ax0 ? s.ax0 : X, last = X + V < s.ax1 ? X + V : s.ax1;
        for (int x = first; x < last; ++x) fr_columns<1>(A, s, b, Y, x, reads);
    }
}

}  // namespace

extern "C" int nd_frame_assemble(const float* patches, const uint16_t* frames, int N, int H2, int W2, const nd_frame_patch* table, float black,
                                 float white, float* noise, float* noisy, uint16_t* short_out, int B, int c, int F, void* stream) {
    const char* who = "nd_frame_assemble";
    const bool composed = noisy || short_out;
    ND_REQUIRE(table && patches, ND_E_BADARG, "%s: null table or patches", who);
    ND_REQUIRE(noise || composed, ND_E_BADARG, "%s: give at least one of noise, noisy and short_out", who);
    ND_REQUIRE(H2 > 0 && W2 > 0 && H2 % 2 == 0 && W2 % 2 == 0, ND_E_BADARG, "%s: a Bayer frame has even, positive sides; got %d x %d", who, H2, W2);
    ND_REQUIRE(c > 0 && B > 0 && B <= 65535 && F > 0, ND_E_BADARG, "%s: c, B (<= 65535) and F must be positive", who);
    ND_REQUIRE(c <= H2 / 2 && c <= W2 / 2, ND_E_BADARG, "%s: the patch %d x %d does not fit the packed frame %d x %d", who, c, c, H2 / 2, W2 / 2);
    ND_REQUIRE(!(frames && composed) || N > 0, ND_E_BADARG, "%s: noisy and short_out read the frames: N must be positive", who);
    ND_REQUIRE(white > black && black >= 0.0f && white <= 65535.0f, ND_E_BADARG, "%s: need 0 <= black < white <= 65535", who);
    const uintptr_t out_bits = (uintptr_t)noise | (uintptr_t)noisy | (uintptr_t)short_out;
    ND_REQUIRE((((uintptr_t)patches | (uintptr_t)frames | (uintptr_t)table | out_bits) & 3u) == 0, ND_E_BADARG,
               "%s: patches, frames, the table and the outputs must be 4-byte aligned", who);
    FrameArgs A;
    A.patches = patches;  A.frames = frames;  A.table = table;  A.noise = noise;  A.noisy = noisy;  A.shrt = short_out;
    A.N = N;  A.H = H2 / 2;  A.W = W2 / 2;  A.c = c;  A.F = F;  A.black = black;  A.white = white;
    const int V = rw_width(A.W, out_bits);
    A.runs = V == 1 ? c : (c - 1) / V + 2;                      // c columns from any start touch at most floor((c - 1) / V) + 2 aligned runs
    const size_t threads = (size_t)c * A.runs;
    const dim3 grid((unsigned)((threads + FR_THREADS - 1) / FR_THREADS), (unsigned)B);
    rw_dispatch(V, [&](auto v) { hipLaunchKernelGGL(frame_assemble_kernel<v()>, grid, dim3(FR_THREADS), 0, (hipStream_t)stream, A); });
    return nd_launch_status(who);
}
