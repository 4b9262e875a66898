/*
 * noisediff_hip.h -- C ABI of libnoisediff_hip.so (gfx950 / MI355X).
 *
 * The reference (IVRL/NoiseDiff) has no native layer: its "kernels" are ATen ops
 * dispatched from Python.  This library is the native layer under
 * the two Python plug-in interfaces of the sampling hot path -- the arch class
 * (models/modules.py:32-41 -> models/archs/Diffusion_arch.py:447-646) and
 * GaussianDiffusion (models/denoising_diffusion_pytorch.py:167-451).  Each entry
 * point below names the reference code it replaces.  The Python side that binds
 * them with ctypes is noisediff_amd/_lib.py; INTEGRATION.md shows the binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated; activations are
 *     NHWC ("pixel-major": [B][H][W][C], `ld` = floats between consecutive pixels);
 *   - `stream` is a hipStream_t passed as void*; nothing here allocates, frees,
 *     synchronises or touches the default stream, so every call is legal inside
 *     hipStreamBeginCapture/EndCapture;
 *   - return value: 0 = ok, >0 = hipError_t of the launch, <0 = ND_E_* argument error.
 *     No exceptions cross the boundary; nd_last_error() gives a message.
 */
#ifndef NOISEDIFF_HIP_H
#define NOISEDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ND_E_BADARG   (-1)   /* null pointer / non-positive size            */
#define ND_E_SHAPE    (-2)   /* shape not supported by the kernel's tiling   */
#define ND_E_ALIGN    (-3)   /* pointer or stride not 16-byte aligned        */
#define ND_E_STATE    (-4)   /* graph/plan handle misuse                     */

/* ------------------------------------------------------------------ library */
int         nd_version(void);                 /* 1000*major + minor                     */
const char* nd_last_error(void);              /* thread-local, never NULL               */
int         nd_device_arch(char* buf, int n); /* gcnArchName of the current device      */

/* ------------------------------------------------------------------ operand descriptors */

/* How a GEMM-like kernel reads its activation operand (the "A" side).              */
enum nd_prologue {
    ND_PRO_NONE        = 0,  /* raw values                                              */
    ND_PRO_AFFINE_SILU = 1,  /* silu((x - M[b,c]) * A[b,c] + D[b,c]): GroupNorm + time
                                scale/shift + SiLU of Block.forward, Diffusion_arch.py:137-143 */
    ND_PRO_AFFINE_MAP_SILU = 2, /* same, then *(S[p,c]+1)+Sh[p,c] before SiLU: ResnetBlock2's
                                per-pixel scale/shift, Diffusion_arch.py:188-192           */
    ND_PRO_LAYERNORM   = 3,  /* LayerNorm over C of (x + vec[b,c]): AttnBlock.norm2 on
                                x + CrossAttention(...), Diffusion_arch.py:438-439          */
    ND_PRO_SILU        = 4,  /* silu(x): ResnetBlock2.mlp[0], Diffusion_arch.py:177         */
    ND_PRO_LEAKY       = 5,  /* LeakyReLU(0.2)(x): LSID's nn.LeakyReLU after every conv,
                                models/archs/SID_arch.py:58,108-168 (applied by the consumer)   */
    ND_PRO_LEAKY_SECOND = 6, /* LeakyReLU(0.2) on the p1 channels of a virtual concat only:
                                torch.cat((up(x), conv_k)), SID_arch.py:135,142,150,158          */
    ND_PRO_AFFINE_GENMAP_SILU = 7  /* ND_PRO_AFFINE_MAP_SILU with the maps FORMED IN THE KERNEL (r6; nd_conv3x3_wino4_nhwc_f32 only): scale | shift =
                                ResnetBlock2.mlp[1] (a 1x1 convolution 8 -> 2C, Diffusion_arch.py:177,188) of the ACTIVATED position embedding.  `map` =
                                silu(pos_emb) [B][H][W][8] (32 bytes per pixel instead of 8 C), `gamma` = mlp[1].weight [2C][8] (rows 0..C-1 scale,
                                C..2C-1 shift), `beta` = mlp[1].bias [2C].  One source, C a multiple of 16.                                             */
};

typedef struct nd_src {
    const float* p0;      /* first source                                               */
    const float* p1;      /* second source of a virtual concat (torch.cat dim=1,
                             Diffusion_arch.py:598,628,631,640) or NULL                 */
    int32_t c0, c1;       /* channels taken from p0 / p1 (multiples of 4)               */
    int32_t ld0, ld1;     /* pixel strides in floats                                    */
    int32_t mode;         /* enum nd_prologue                                           */
    int32_t upsample;     /* 1: p0 is (H/2, W/2), read through nearest x2 (nn.Upsample,
                             Diffusion_arch.py:74); conv3x3 only                        */
    int32_t unshuffle;    /* 1: p0 is (2H, 2W, c0/4) read as 'b c (h p1)(w p2) -> b (c p1 p2) h w'
                             (Diffusion_arch.py:80) with K order (p1 p2 c); pointwise only */
    int32_t map_blocked;  /* AFFINE_MAP: 0: `map` is [B][H][W][scale C | shift C] (the layout torch.chunk(2, dim=1) reads,
                             Diffusion_arch.py:188); 1: blocked by 16 channels, [B][H][W][C/16][scale 16 | shift 16] -- one
                             128-byte line per pixel and 16-channel K chunk; nd_conv3x3_wino4_nhwc_f32 only (C % 16 == 0) */
    const float* mad;     /* [B][3][C] M, A, D for the AFFINE modes (from nd_groupnorm_finalize_f32) */
    const float* map;     /* [B][H][W][2C] scale / shift map (AFFINE_MAP), layout per map_blocked */
    const float* vec;     /* [B][C] per-sample vector added before LayerNorm            */
    const float* gamma;   /* [C] LayerNorm weight                                       */
    const float* beta;    /* [C] LayerNorm bias                                         */
    const float* rowstats;/* [B*HW][2] per-pixel {mean, rstd} of (x + vec) from nd_layernorm_stats_f32;
                             required for LAYERNORM when C > 64 (for C <= 64 the GEMM derives them itself) */
} nd_src;

enum nd_act { ND_ACT_NONE = 0, ND_ACT_GELU = 1, ND_ACT_SILU = 2 };

/* ------------------------------------------------------------------ conv 3x3 */

/* nn.Conv2d(cin, cout, 3, padding=1) on NHWC fp32 with exact-fp32 MFMA accumulation
 * (v_mfma_f32_32x32x2_f32 == an fmaf chain).  Replaces Block.proj (Diffusion_arch.py:131,136),
 * the last-stage down/up convs (:533,:547) and Upsample's conv (:75).
 * Weights are pre-packed by nd_pack_conv3x3_weight.  When `stats` != NULL the epilogue
 * also emits per-(sample, slot, channel) partial sums {sum, M2} of the output for the
 * following GroupNorm (Block.norm :132); `slot_count[slot]` receives the number of pixels
 * behind each slot.  Query the slot count with nd_conv3x3_stat_slots.
 * Five kernels compute this operator from the same descriptor (below), each within limits of its own: channel multiples, chunk boundaries of a concat, pixel and
 * byte counts, the prologues it reads.  nd_conv3x3_takes answers whether a kernel takes a descriptor and is the ONLY statement of those limits (csrc/conv3x3_desc.h,
 * run by the entry points themselves): callers ask it and keep policy only -- which kernel they prefer where several take the layer. */
typedef struct nd_conv3x3 {
    nd_src   src;
    const float* weight;   /* packed, see nd_pack_conv3x3_weight                         */
    const float* bias;     /* [cout] or NULL                                             */
    float*   out;          /* [B][H][W] x ldo                                            */
    float*   stats;        /* [B][slots][cout][2] or NULL                                */
    float*   slot_count;   /* [slots] or NULL                                            */
    int32_t  B, H, W;      /* OUTPUT spatial size                                        */
    int32_t  cin, cout, ldo;
} nd_conv3x3;

int nd_conv3x3_nhwc_f32(const nd_conv3x3* d, void* stream);
/* 1 where `kernel`'s entry takes the sizes, strides, prologue and addressing of `d`, else 0.  Host code: no GPU, no HIP call, nd_last_error untouched (a question
 * is not a failure).  Reads no pointer of `d`: a descriptor with the integers alone will do.  `splits` > 1: the split-K entry of an F(4x4) kernel with that many ranges. */
enum nd_conv3x3_kernel { ND_CONV3X3_DIRECT = 0, ND_CONV3X3_WINO = 1, ND_CONV3X3_WINO2 = 2, ND_CONV3X3_WINO4 = 3, ND_CONV3X3_WINO4_16 = 4 };
int nd_conv3x3_takes(int kernel, const nd_conv3x3* d, int splits);   /* 1 / 0; splits <= 1: the plain form */
int nd_conv3x3_stat_slots(int H, int W, int cout, int B);
/* which conv3x3_kernel<TW, MB, NB> instance a shape runs on: TW*100 + MB*10 + NB (for profiling reports) */
int nd_conv3x3_tiling_id(int B, int H, int W, int cout);
/* OIHW (cout,cin,3,3) -> [tap][cin/4][coutP][4], coutP = cout rounded up to 64; zero padded. */
int64_t nd_pack_conv3x3_weight_floats(int cin, int cout);
int nd_pack_conv3x3_weight(const float* oihw, float* packed, int cin, int cout, void* stream);
/* training (loss.backward() of p_losses, models/trainer_diffusion.py:187): the same packing of the DATA-GRADIENT operator of a layer
 * (nn.Conv2d(cin, cout, 3, padding=1), Diffusion_arch.py:131), read in place from the forward layer's OIHW weight
 * `oihw_fwd` (cout x cin there = cin x cout here): g'[co][ci][r][s] = oihw_fwd[ci][co][2 - r][2 - s].  `cin`, `cout` are the
 * data-gradient convolution's (cin = the forward layer's cout).  Likewise for the two Winograd packings below. */
int nd_pack_conv3x3_weight_dgrad(const float* oihw_fwd, float* packed, int cin, int cout, void* stream);

/* Same operator, same descriptor, computed with Winograd F(2x2,3x3) (2.25x fewer multiplies; fp32 transforms,
 * ~1e-6 relative difference to the direct form).  `weight` must come from nd_pack_conv3x3_wino_weight
 * (U = G g G^T in 128 KB blocks [cinP/32][coutP/64][16 positions][8 quads][64][4]); statistics slots:
 * nd_conv3x3_wino_stat_slots.  Used for images >= 16x16. */
int nd_conv3x3_wino_nhwc_f32(const nd_conv3x3* d, void* stream);
/* Same contract, one-workgroup-per-CU variant: all 16 Winograd position accumulators stay in registers across the
 * K loop and the halo tile is double-buffered in LDS (conv3x3_wino2.hip). */
int nd_conv3x3_wino2_nhwc_f32(const nd_conv3x3* d, void* stream);
int nd_conv3x3_wino_stat_slots(int H, int W);
int64_t nd_pack_conv3x3_wino_weight_floats(int cin, int cout);
int nd_pack_conv3x3_wino_weight(const float* oihw, float* packed, int cin, int cout, void* stream);
int nd_pack_conv3x3_wino_weight_dgrad(const float* oihw_fwd, float* packed, int cin, int cout, void* stream);

/* The same operator with Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32 (1.78x fewer multiplies than F(2x2,3x3); ~1e-5 relative
 * difference to the direct form): the kernel that carries the sampling path (conv3x3_wino4.hip).  Takes plain / two-source
 * (concat on a 16-channel boundary) inputs, the GroupNorm-affine (+ per-pixel map) + SiLU and LeakyReLU prologues, nearest-x2
 * upsample addressing of a single source and the statistics epilogue; needs cin > 16, cout <= 2048, W <= 2048, sources below
 * 1 GiB / 2^24 pixels (rejected otherwise: the caller picks nd_conv3x3_wino2_nhwc_f32).  `weight` from
 * nd_pack_conv3x3_wino4_weight (U = G g G^T in blocks [cin/8][coutP/16][18 position pairs][64 lanes][4]). */
int nd_conv3x3_wino4_nhwc_f32(const nd_conv3x3* d, void* stream);
/* The same kernel on 16 x 16-pixel regions with TWO co-resident workgroups per CU (two waves per SIMD: one workgroup's LDS round trips,
 * barriers, store queue and transforms run under the other's MFMAs; r4).  Same packed weights, statistics slots and descriptor, and the
 * same bits as nd_conv3x3_wino4_nhwc_f32 (identical arithmetic in identical order).  Plain and GroupNorm-affine + SiLU sources only
 * (Block.proj of ResnetBlock, Diffusion_arch.py:128-170; the resampling convs :75,533,547); also the F(4x4) path of images narrower
 * than 32 pixels (BASELINE config 2's 16 x 16 stage). */
int nd_conv3x3_wino4_16_nhwc_f32(const nd_conv3x3* d, void* stream);
/* its statistics epilogue writes ONE slot per 16 x 16-pixel tile (the F(2x2) kernels: two) */
int nd_conv3x3_wino4_stat_slots(int H, int W);
int64_t nd_pack_conv3x3_wino4_weight_floats(int cin, int cout);
int nd_pack_conv3x3_wino4_weight(const float* oihw, float* packed, int cin, int cout, void* stream);
int nd_pack_conv3x3_wino4_weight_dgrad(const float* oihw_fwd, float* packed, int cin, int cout, void* stream);
/* Many weights in one launch (the training path repacks every Block.proj weight, forward and data-gradient form, once per optimizer step):
 * nd_pack_item records in DEVICE memory (shared with nd_pack_pointwise_weights_batch below); item.w = OIHW weight (the FORWARD layer's when
 * item.transposed != 0, which selects the _dgrad form; cin / cout are then the data-gradient operator's), item.packed = its
 * nd_pack_conv3x3_wino4_weight_floats(cin, cout) floats. */
typedef struct nd_pack_item {
    const float* w;
    float*       packed;
    int32_t      cin, cout, transposed, reserved;
} nd_pack_item;
int nd_pack_conv3x3_wino4_weights_batch(const nd_pack_item* items_dev, int n_items, void* stream);
/* Split-K form of nd_conv3x3_wino4_nhwc_f32 for plain and GroupNorm-affine + SiLU sources -- the forward and data-gradient convolutions of
 * Block.proj under GaussianDiffusion.p_losses (models/archs/Diffusion_arch.py:128-144; models/denoising_diffusion_pytorch.py:481-531) at
 * training batch sizes (512 -> 512 at
 * 32 x 32 with 4 samples is 64 workgroup items for 256 CUs, each walking 32 K chunks): cin is cut into `splits` ranges (2, 4 or 8; whole
 * 16-channel chunks, at least two per range), every (range, sample, region, cout tile) is a workgroup item that writes partial sums to
 * `workspace` ([splits][B][H][W][cout] floats), and a second kernel adds them in range order and the bias into d->out -- and, when d->stats is
 * set, leaves the statistics slots of the summed output as the plain kernel's epilogue does (one slot per 16 x 16 tile).  _plan returns the
 * split count for a shape (1 = use the plain entry) -- a function of the shape alone, so results never depend on the device. */
int nd_conv3x3_wino4_splitk_plan(int B, int H, int W, int cin, int cout);
int64_t nd_conv3x3_wino4_splitk_workspace_floats(int B, int H, int W, int cout, int splits);
int nd_conv3x3_wino4_splitk_nhwc_f32(const nd_conv3x3* d, float* workspace, int splits, void* stream);
/* Split-K on the 16 x 16-region form, for SAMPLING (r4): layers with few (region, cout tile) items per sample -- the 16 x 16 and 32 x 32 stages of
 * BASELINE config 2 (Diffusion_arch.py:533,547 at H/8) -- are cut along cin.  _plan looks at the SAMPLE's geometry only (no batch argument), so a
 * sample's bits never depend on the batch it is sharded into: 2, 4 or 8 ranges so that a sample has about 32 items, at least four chunks per range.
 * Workspace: nd_conv3x3_wino4_splitk_workspace_floats. */
int nd_conv3x3_wino4_16_splitk_plan(int H, int W, int cin, int cout);
int nd_conv3x3_wino4_16_splitk_nhwc_f32(const nd_conv3x3* d, float* workspace, int splits, void* stream);

/* ------------------------------------------------------------------ conv 3x3, training */

/* Weight gradient of nn.Conv2d(cin, cout, 3, padding=1): dw[co][ci][r][s] = sum_{b,y,x} dy[b][y][x][co] * x[b][y+r-1][x+s-1][ci]
 * (zero padding), x and dy NHWC fp32, dw in the torch OIHW layout.  The backward of Block.proj and the resampling convs under
 * GaussianDiffusion.p_losses (models/denoising_diffusion_pytorch.py:481-531; loss.backward() at models/trainer_diffusion.py:187).
 * Exact-fp32 MFMA; the split over pixel tiles depends on the shape only and the partial sums are added in a fixed order, so the
 * result is bitwise repeatable.  `workspace`: nd_conv3x3_wgrad_workspace_floats(...) floats.  `dbias` (may be NULL): the bias
 * gradient db[co] = sum_{b,y,x} dy[b][y][x][co], from the same dy tiles (same fixed order).
 * Two forms, chosen by the shape alone.  H % 4 == 0, W % 16 == 0, both channel counts multiples of 16, fewer than 2^30 pixels and each tensor below
 * 1 GiB per sample: the Winograd-domain F(4x4,3x3)
 * form -- per 4 x 4 pixel tile the 6 x 6 transforms of the input patch and of the dY block, 36 position-wise products (a quarter of the
 * nine-tap form's MFMAs), one back-transform G^T M G at the end; error ~4e-6 of max|dW| against a float64 sum.  Anything else: nine tap
 * GEMMs over the pixels (4e-7).  ND_WGRAD_WINO=0 forces the nine-tap form (A/B); nd_conv3x3_wgrad_form pins any of them.
 * These limits are written once, in csrc/conv3x3_wgrad.hip; callers ask nd_conv3x3_wgrad_plan / nd_conv3x3_wgrad_cat_takes (no HIP call, nd_last_error untouched).
 * The DATA gradient of the same layer is the forward operator itself: nd_conv3x3_*_nhwc_f32 on weights packed by
 * nd_pack_conv3x3_*_weight_dgrad (taps flipped, channel roles swapped) -- see noisediff_amd/train.py. */
int64_t nd_conv3x3_wgrad_workspace_floats(int B, int H, int W, int cin, int cout);
/* Tests and A/B tools: pin the form -- 0 by the shape (default), 1 nine taps, 2 Winograd domain on four waves, 3 on eight waves (cout % 64 == 0;
 * else four); anything else only queries.  Returns the previous setting.  Process-wide; ask for the workspace size AFTER setting it. */
/* The same for an input that is the virtual concatenation cat((x0, x1), channels) -- the up path's skip connections -- without the concatenated
 * tensor: dw (cout, c0 + c1, 3, 3).  Winograd-domain forms only (the limits above with c0 and c1 multiples of 32, cout of 16; never under pin 1):
 * ND_E_SHAPE otherwise (one nd_conv3x3_wgrad_nhwc_f32 per source).  nd_conv3x3_wgrad_cat_takes: 1 exactly where this entry does not refuse the shape.
 * Workspace: nd_conv3x3_wgrad_workspace_floats(B, H, W, c0 + c1, cout). */
int nd_conv3x3_wgrad_cat_nhwc_f32(const float* x0, int ldx0, int c0, const float* x1, int ldx1, int c1, const float* dy, int ldy, float* dw_oihw,
                                  float* dbias, float* workspace, int B, int H, int W, int cout, void* stream);
int nd_conv3x3_wgrad_cat_takes(int B, int H, int W, int c0, int c1, int cout, int ldx0, int ldx1, int ldy);
int nd_conv3x3_wgrad_form(int form);
/* The form nd_conv3x3_wgrad_nhwc_f32 runs on dense tensors of this shape under the current pin: 1, 2 or 3 as nd_conv3x3_wgrad_form numbers them. */
int nd_conv3x3_wgrad_plan(int B, int H, int W, int cin, int cout);
int nd_conv3x3_wgrad_nhwc_f32(const float* x, int ldx, const float* dy, int ldy, float* dw_oihw, float* dbias, float* workspace,
                              int B, int H, int W, int cin, int cout, void* stream);
/* LSID training (models/archs/SID_arch.py:105-175; noisediff_amd/lsid_train.py): the same weight gradients for an input that is LeakyReLU(0.2) of the
 * RAW tensor passed -- the activation is applied as the operand is staged, no activated copy.  Same forms, split and summation order as above.
 * _leaky: x is raw, the layer's input is leaky(x) (every 3x3 convolution of LSID but conv1_1).  _cat_leaky_second: the input is
 * cat((x0, leaky(x1)), channels) -- torch.cat((up(x), conv_k)) in front of conv6_1 .. conv9_1 (:135,142,150,158), as ND_PRO_LEAKY_SECOND reads it
 * forward; any channel counts that are multiples of 4 (the Winograd-domain form where nd_conv3x3_wgrad_cat_nhwc_f32 takes the shape, else the nine-tap
 * form per source into its columns of dw).  Workspace: nd_conv3x3_wgrad_cat_workspace_floats. */
int nd_conv3x3_wgrad_leaky_nhwc_f32(const float* x, int ldx, const float* dy, int ldy, float* dw_oihw, float* dbias, float* workspace,
                                    int B, int H, int W, int cin, int cout, void* stream);
int64_t nd_conv3x3_wgrad_cat_workspace_floats(int B, int H, int W, int c0, int c1, int cout);
int nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32(const float* x0, int ldx0, int c0, const float* x1, int ldx1, int c1, const float* dy, int ldy,
                                               float* dw_oihw, float* dbias, float* workspace, int B, int H, int W, int cout, void* stream);
/* The gradient join at every LeakyReLU of the LSID training backward: dz = (d_direct + pool_scatter(d_pool)) * (z > 0 ? 1 : 0.2), one streaming pass.
 * z, dz: [B][H][W][C] dense (z = the convolution's RAW output); d_direct (may be NULL): [B][H][W] x ld_direct, the gradient of leaky(z) through
 * its direct consumers (e.g. the skip half of a concat convolution's data gradient); d_pool (may be NULL): [B][ceil(H/2)][ceil(W/2)][C], the gradient
 * of nn.MaxPool2d(2, 2, ceil_mode=True)(leaky(z)), routed to the first maximum of each window in row-major order (torch's max_pool2d backward, ties
 * and partial border windows included).  dz may alias d_direct when ld_direct == C. */
int nd_leaky_grad_join_f32(const float* z, float* dz, const float* d_direct, int ld_direct, const float* d_pool, int B, int H, int W, int C,
                           void* stream);

/* nn.GroupNorm(groups, C) forward and backward on NHWC fp32 for training: Block.norm (Diffusion_arch.py:132,138) under
 * GaussianDiffusion.p_losses -> loss.backward().  Statistics per (sample, group) over (C / groups) x HW values, eps inside the
 * square root, affine weight and bias -- torch.nn.functional.group_norm's definition.  Forward: y = (x - mean) rstd gamma + beta and
 * `mean_rstd` [B][groups][2] for the backward.  Backward: dx, dgamma [C], dbeta [C] from dy, x and the saved statistics.
 * Every pass streams NHWC once (partial sums per pixel slot, fp64 finalize, one elementwise pass); fixed summation order.
 * `workspace`: nd_groupnorm_train_workspace_floats(B, HW, C) floats, shared by both directions.
 * nd_groupnorm_train_takes(C, groups): 1 / 0, the channel counts these entries and the nd_groupnorm_silu_train_* ones take (C a multiple of 4 and of groups,
 * <= 1024, at most 512 per group) -- the only statement of that limit, like nd_conv3x3_takes. */
int nd_groupnorm_train_takes(int C, int groups);
int64_t nd_groupnorm_train_workspace_floats(int B, int HW, int C);
int nd_groupnorm_train_forward_f32(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* mean_rstd,
                                   float* workspace, int B, int HW, int C, int groups, float eps, void* stream);
int nd_groupnorm_train_backward_f32(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* mean_rstd,
                                    float* dx, int lddx, float* dgamma, float* dbeta, float* workspace, int B, int HW, int C, int groups,
                                    void* stream);

/* Block's tail as one training operator: y = silu(GroupNorm(x) * (scale + 1) + shift) (Block.forward, Diffusion_arch.py:137-143) with the
 * per-(sample, channel) scale / shift of the time embedding (`scale_shift` [B][2C] = scale | shift as ResnetBlock.mlp emits it, :150-152,162-164;
 * NULL: plain GroupNorm + SiLU).  Forward saves `mean_rstd` [B][groups][2] and `mad` [B][3][C]; backward returns dx, dgamma, dbeta and
 * `dscale_shift` [B][2C] (NULL iff scale_shift is NULL).  Two passes over the tensor per direction (the separate ops take four and seven).
 * `workspace`: nd_groupnorm_silu_train_workspace_floats(B, HW, C) floats. */
int64_t nd_groupnorm_silu_train_workspace_floats(int B, int HW, int C);
int nd_groupnorm_silu_train_forward_f32(const float* x, int ldx, const float* gamma, const float* beta, const float* scale_shift, const float* res, int ldr,
                                        float* y, int ldy, float* mean_rstd, float* mad, float* workspace, int B, int HW, int C, int groups, float eps,
                                        void* stream);   /* res (may be NULL): + the ResnetBlock's shortcut, h + res_conv(x) (Diffusion_arch.py:170), in the same pass */
int nd_groupnorm_silu_train_backward_f32(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* beta,
                                         const float* scale_shift, const float* mean_rstd, const float* mad, float* dx, int lddx,
                                         float* dgamma, float* dbeta, float* dscale_shift, float* workspace, int B, int HW, int C, int groups,
                                         void* stream);

/* ResnetBlock2's modulation + activation for training (Diffusion_arch.py:173-196: scale / shift are per-pixel MAPS from the position
 * embedding): y = silu(n * (scale + 1) + shift), n [N][>= C] the GroupNorm's output, map [N][>= 2C] = scale | shift as ResnetBlock2.mlp emits it.
 * Backward: dn, and dmap [N][2C] = d scale | d shift, one pass each (the separate ops take four and five). */
int nd_modulate_silu_forward_f32(const float* n, int ldn, const float* map, int ldm, float* y, int ldy, int64_t N, int C, void* stream);
int nd_modulate_silu_backward_f32(const float* dy, int lddy, const float* n, int ldn, const float* map, int ldm, float* dn, int lddn, float* dmap, int lddm,
                                  int64_t N, int C, void* stream);

/* out[b][c] = sum over the HW tokens of x[b][p][c]: the gradient of a per-sample vector broadcast over the tokens -- AttnBlock's one-token ISO
 * cross attention adds to_out(to_v(ctx)) to every token (Diffusion_arch.py:435-437).  Fixed order; workspace: nd_token_sum_workspace_floats.
 * nd_token_sum_takes(C): 1 / 0, the widths it takes (a multiple of 4 up to 1024). */
int nd_token_sum_takes(int C);
int64_t nd_token_sum_workspace_floats(int B, int HW, int C);
int nd_token_sum_f32(const float* x, int ldx, float* out, float* workspace, int B, int HW, int C, void* stream);

/* nn.LayerNorm(C) over the channels of NHWC tokens for training (AttnBlock.norm1 / norm2, Diffusion_arch.py:427-428): forward
 * y = (x - mean) rstd gamma + beta with `stats` [N][2] = {mean, rstd} per token saved for the backward; backward dx, dgamma [C],
 * dbeta [C].  C a multiple of 4 in 16 .. 1024 (a row lives in 16 / 32 / 64 lanes; nd_layernorm_train_takes(C) answers 1 / 0); eps inside the square root, biased
 * variance -- torch.nn.functional.layer_norm's definition.  One streaming pass per direction, fixed summation order.
 * `workspace` (backward): nd_layernorm_train_workspace_floats(N, C) floats. */
int nd_layernorm_train_takes(int C);
int64_t nd_layernorm_train_workspace_floats(int64_t N, int C);
int nd_layernorm_train_forward_f32(const float* x, int ldx, const float* gamma, const float* beta, float* y, int ldy, float* stats,
                                   int64_t N, int C, float eps, void* stream);
int nd_layernorm_train_backward_f32(const float* dy, int lddy, const float* x, int ldx, const float* gamma, const float* stats,
                                    float* dx, int lddx, float* dgamma, float* dbeta, float* workspace, int64_t N, int C, void* stream);

/* Weight and bias gradient of a token Linear / 1x1 convolution: dw[co][ci] = sum_p dy[p][co] * x[p][ci], dbias[co] = sum_p dy[p][co]
 * over N tokens (x, dy: [N][ld] fp32, NHWC pixels are tokens; dw in torch's (cout, cin) layout; dbias may be NULL).  The backward of
 * res_conv, Mlp.fc1/fc2, FeedForward, proj_out and the attention projections (Diffusion_arch.py:156,345-347,410-419,432) under
 * GaussianDiffusion.p_losses.  Exact-fp32 MFMA, fixed split and summation order (bitwise repeatable).
 * `workspace`: nd_linear_wgrad_workspace_floats(N, cin, cout) floats.  (The data gradient is a plain GEMM, dy @ W.) */
int64_t nd_linear_wgrad_workspace_floats(int64_t N, int cin, int cout);
int nd_linear_wgrad_f32(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* workspace,
                        int64_t N, int cin, int cout, void* stream);
/* The same with LeakyReLU(0.2) applied to x as it is staged (LSID's conv10 on the raw conv9_2 output, SID_arch.py:168-172). */
int nd_linear_wgrad_leaky_f32(const float* x, int ldx, const float* dy, int ldy, float* dw, float* dbias, float* workspace,
                              int64_t N, int cin, int cout, void* stream);
/* Weight gradient of nn.ConvTranspose2d(cin, cout, 2, stride=2, bias=False) on leaky(x) followed by the crop to (up_h, up_w) (SID_arch.py:134-158):
 * dw[ci][c][p1][p2] = sum over (b, y, x) of leaky(x[b][y][x][ci]) * d_up[b][2y + p1][2x + p2][c], terms past the crop absent; x [B][h][w] x ldx raw,
 * d_up [B][up_h][up_w] x ld_up (may be a channel slice), dw in torch's (cin, cout, 2, 2) layout.  Fixed split and order, as nd_linear_wgrad_f32.
 * Workspace: nd_convt2x2_wgrad_workspace_floats(B, h, w, cin, cout). */
int64_t nd_convt2x2_wgrad_workspace_floats(int B, int h, int w, int cin, int cout);
int nd_convt2x2_wgrad_leaky_f32(const float* x, int ldx, const float* d_up, int ld_up, float* dw, float* workspace, int B, int h, int w,
                                int cin, int cout, int up_h, int up_w, void* stream);

/* ------------------------------------------------------------------ pointwise GEMM */

/* out[p, n] = epi( sum_k pro(in[p, k]) * W[k, n] + bias[n] ) per pixel: nn.Conv2d(k=1) and
 * nn.Linear on tokens are the same op in NHWC.  Replaces res_conv (:156), Downsample's conv
 * (:81), Mlp.fc1/fc2 (:345-347), ResnetBlock2.mlp (:178), FeedForward (:410-419),
 * AttnBlock.proj_out (:432), final_conv (:554).
 * Epilogue, in order: +bias, act, +res0, +res1, +vec[b,n], +silu((t - M)*A + D) where t is a
 * raw conv output (ResnetBlock tail `h + res_conv(x)`, :170). */
typedef struct nd_pointwise {
    nd_src   src;
    const float* weight;   /* packed [cinP/4][coutP][4], see nd_pack_pointwise_weight     */
    const float* bias;     /* [cout] or NULL                                             */
    float*   out;
    const float* res0; const float* res1;   /* [B][HW] x ldr0/ldr1 or NULL               */
    const float* vec;      /* [B][cout] or NULL                                          */
    const float* gn_t;     /* tensor t for the fused GroupNorm+SiLU add, or NULL          */
    const float* gn_mad;   /* [B][3][cout]                                               */
    int32_t  B, HW, W;     /* HW = output pixels per sample; W = output width (unshuffle) */
    int32_t  cin, cout, ldo, ldr0, ldr1, ldt;
    int32_t  act;          /* enum nd_act                                                */
    int32_t  shuffle_c;    /* > 0: ConvTranspose2d(k=2, s=2) scatter (SID_arch.py:84-99): cout = 4*shuffle_c ordered
                              (p1 p2 c); row p=(y,x) writes channel c of output pixel (2y+p1, 2x+p2) of a
                              (shuffle_h, shuffle_w) image (rows/cols beyond it are cropped, :135)   */
    int32_t  shuffle_h, shuffle_w;
} nd_pointwise;

int nd_pointwise_gemm_nhwc_f32(const nd_pointwise* d, void* stream);
/* The data gradient of ConvTranspose2d(k=2, s=2) + crop (SID_arch.py:134-158): d->src.unshuffle = 1 with p0 = d_up, an image of (src_h, src_w)
 * <= (2 H, 2 W) pixels (H = HW / W), read as its pixel unshuffle with zeros for the rows / columns the forward cropped away; weight packed by
 * nd_pack_pointwise_weight(w.reshape(cin, 4 c) of the ConvTranspose weight (cin, c, 2, 2), ..., cin = 4 c, cout = cin, unshuffle_c = c). */
int nd_pointwise_gemm_unshuffle_crop_nhwc_f32(const nd_pointwise* d, int src_h, int src_w, void* stream);

/* ------------------------------------------------------------------ scoring of denoised frames (test_denoising.py:220-263,318-343)
 * Images are fp32 NCHW [B][C][H][W], contiguous.  Results are per image; an image's results do not depend on B and a repeated call gives
 * the same bits (fixed reduction order, no atomics).  Each call is two launches; the workspace is the caller's.
 *
 * nd_image_quality_f32: skimage's peak_signal_noise_ratio and structural_similarity(channel_axis=2, data_range=R) of est against target,
 * both clipped to [0, R] first (NaN kept), as tensor2im does.  PSNR = 10 log10(R^2 / mse), mse = mean of fl32(fl32(x - y)^2) accumulated in
 * fp64; SSIM with a 7 x 7 uniform window, cov_norm 49/48, K1 0.01, K2 0.03, window sums and S in fp64, S averaged over the interior
 * [3, H-3) x [3, W-3), then over channels.  `scale` (may be NULL): per-image fp32 k of nd_illum_scale_f32; est is then read as
 * clip(fl32(k * clamp(est, 0, 1)), 0, R), the illumination-corrected prediction without a pass over memory.  psnr / ssim / mse: fp64 [B].
 * H and W must be at least 7 (ND_E_SHAPE).  Workspace: nd_image_quality_workspace_bytes(B, C, H, W) bytes, 8-byte aligned. */
int64_t nd_image_quality_workspace_bytes(int B, int C, int H, int W);
int nd_image_quality_f32(const float* est, const float* target, const float* scale, double data_range, double* psnr, double* ssim,
                         double* mse, void* workspace, int B, int C, int H, int W, void* stream);
/* IlluminanceCorrect's scale (:252-263): p = clamp(pred, 0, 1), num = sum p s and den = sum p p over the elements with source != 1, in fp64;
 * k64 = num / den (NaN or inf when den is 0, as the reference), k32 = k64 rounded to fp32.  source_batch: 1 (one source for every image) or
 * B.  Workspace: nd_illum_scale_workspace_bytes(B, C, H, W) bytes. */
int64_t nd_illum_scale_workspace_bytes(int B, int C, int H, int W);
int nd_illum_scale_f32(const float* pred, const float* source, int source_batch, float* k32, double* k64, void* workspace,
                       int B, int C, int H, int W, void* stream);
/* out = k32[b] * clamp(pred, 0, 1) in fp32: IlluminanceCorrect's output.  out may alias pred. */
int nd_illum_apply_f32(const float* pred, const float* k32, float* out, int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------ scoring of generated noise (utils/util.py:185-255, utils/raw_util.py:161-189)
 * The KL-divergence yardstick of the noise-generation literature (get_histogram, kl_div_forward / _inverse / _sym / kl_div_3, the 66-bin
 * edges of kldiv_patch_set) and the signal-dependence check (sliding_window, compute_poisson_lambda_by_patch).  A repeated call gives the
 * same bits, a set's (image's) result does not depend on the other sets of the call, the workspace is the caller's and the outputs need
 * no zeroing.  Argument errors: ND_E_BADARG (null pointer, non-positive size, misaligned pointer, q_sets) or ND_E_SHAPE (n_bins).
 *
 * nd_histogram_f32: np.histogram(x[s], edges)[0] for each of the S sets of n fp32 values (x: [S][n], contiguous, 4-byte aligned).  edges:
 * n_edges = n_bins + 1 doubles on the device, 1 <= n_bins <= 4096; counts: int64 [S][n_bins]; both 8-byte aligned.  v is counted in bin i
 * when edges[i] <= (double)v < edges[i + 1], the last bin also takes v == edges[n_bins]; NaN, +-inf and values outside
 * [edges[0], edges[n_bins]] are counted nowhere.  The comparison is in double against the edges as given (np.arange's edges are not
 * round).  The edges must be finite and STRICTLY increasing: numpy also accepts repeated edges, this library does not, and it cannot
 * check a device array -- that is the caller's contract (noisediff_amd.noise_stats checks the host array it uploads).  Two launches:
 * every workgroup counts into a uint32 histogram in LDS (integer LDS atomics: the order does not matter) and stores it to the workspace,
 * the second launch sums a set's partials in a fixed order.  A workgroup takes nd_histogram_chunk_elements() elements per trip.
 * Workspace: nd_histogram_workspace_bytes(S, n, n_bins) bytes, 4-byte aligned.  S <= 65535, n <= 2^40. */
int     nd_histogram_chunk_elements(void);
int64_t nd_histogram_workspace_bytes(int S, int64_t n, int n_bins);
int nd_histogram_f32(const float* x, int S, int64_t n, const double* edges, int n_edges, int64_t* counts, void* workspace, void* stream);
/* kl_div_3 (:199-227) of S pairs of histograms, everything in fp64, one workgroup per set, fixed summation order: with p = p_counts / n_p and
 * q = q_counts / n_q (n: the element count np.prod(data.shape) of get_histogram, dropped values included, not the sum of the counts),
 * out[s] = { sum p log(p / q), sum q log(q / p), their mean } over the bins with p > 0 and q > 0; no such bin gives 0.0.  p_counts: int64
 * [S][n_bins]; q_counts: [q_sets][n_bins] with q_sets 1 (one histogram for every set) or S; out: fp64 [S][3].
 * nd_kl_div_hist_f64: the same for hists that are already fp64 fractions; a bin whose p or q is NaN or inf is dropped, as the reference does. */
int nd_kl_div_f64(const int64_t* p_counts, const int64_t* q_counts, int64_t n_p, int64_t n_q, int n_bins, int S, int q_sets, double* out,
                  void* stream);
int nd_kl_div_hist_f64(const double* p, const double* q, int n_bins, int S, int q_sets, double* out, void* stream);
/* compute_poisson_lambda_by_patch (:161-189) for an fp32 NCHW image: per pixel the mean and the unbiased standard deviation (divisor 8) of
 * its 3 x 3 window with ZERO padding (F.unfold(3, padding 1) + torch.std_mean), both formed in fp32 from the nine values in two passes.
 * std, mean: fp32 [B][C][H][W], either may be NULL and is then not written.  fit: fp64 [B * C][7] = { N = H W, sum m, sum s, sum m m,
 * sum m s, slope, intercept }, the sums over the fp32 m and s of every pixel accumulated in fp64 in a fixed order, slope =
 * (N sum ms - sum m sum s) / (N sum mm - (sum m)^2) and intercept = (sum s - slope sum m) / N: LinearRegression().fit(mean, std)'s coef_
 * and intercept_.  A zero denominator gives NaN for both.  H, W >= 1.  Workspace: nd_patch_std_mean_workspace_bytes(B, C, H, W) bytes, 8-byte aligned. */
int64_t nd_patch_std_mean_workspace_bytes(int B, int C, int H, int W);
int nd_patch_std_mean_f32(const float* x, float* std, float* mean, double* fit, void* workspace, int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------ noise level function (utils/raw_util.py:248-322)
 * get_poisson_lambda, get_poisson_lambda_all_images and get_regression_result_all_images: the noisy pixels grouped by the clean value they
 * sit on, the unbiased std of every group, and sklearn's TheilSenRegressor of std on clean value.  Nothing allocates, frees, synchronises or
 * reads on the host inside an entry point, so each can be captured; argument errors are ND_E_BADARG before any device call.
 *
 * The table: uint64 [n_levels][4] = { count, sum q, low and high 64 bits of sum q^2 }, q = rint(noisy * 2^30) + 2^32 (unsigned, below
 * 2^33); counters: uint64 [2].  Both 8-byte aligned; nd_level_table_bytes(n_levels) is the table's size.  nd_level_moments_reset zeroes
 * both (one plain launch).  1 <= n_levels <= 2^24, 0 < scale <= 2^24.
 *
 * nd_level_moments_f32 ADDS n elements (1 <= n <= 2^31 - 1; clean, noisy: fp32, 4-byte aligned, any length, vector loads when both start
 * on 16 bytes) to the table.  The level of an element is l = rint(clean * scale) in fp32; it is on the grid when 0 <= l < n_levels and
 * fabsf(clean - (float)l / (float)scale) < 1e-6f, the reference's own membership test applied to the value the packer produces for code l
 * (scale = white - black = 15871, n_levels = 15872 for the Sony frames).  Two deviations from the reference: an element off the grid adds 1
 * to counters[0] and is left out (the reference opens a group of its own for such a value); an on-grid element whose noisy is NaN, +-inf or
 * |noisy| >= 4 adds 1 to counters[1] and is left out (the reference turns the level's std into a NaN and then drops the level).  Every sum
 * is formed by 64-bit INTEGER atomic adds, the high word of sum q^2 taking the carry of the low one (old + v < old on the value the atomic
 * returns): integer adds commute, so the table is exact and does not depend on the order of the elements, on the split into calls or on
 * the batch.  A wave whose 256 elements of a trip share one level adds them in registers and issues the atomics from one lane.  A table may
 * take 2^31 - 1 elements in total (about 178 SID frames): within that n sum q^2 - (sum q)^2 fits 128 bits.  The entry point cannot see the
 * total without a synchronisation: the caller counts what it adds (noisediff_amd.noise_level.LevelMoments raises before the launch that
 * would pass the limit).
 *
 * nd_level_stats_f64: per level count (int64), mean = (sum q / n - 2^32) 2^-30 and std = sqrt((n sum q^2 - (sum q)^2) / n / (n - 1)) 2^-30
 * (fp64 [n_levels] each): the integer part exactly in 128-bit arithmetic, one correctly rounded conversion, two IEEE divisions.  n < 2
 * gives a NaN std, as torch.std does, n == 0 also a NaN mean.
 *
 * nd_level_curve_f64: the fit's input.  The "unique values" are the levels with count >= 1 in ascending order, U of them; with
 * below_median = 1 the first (U - 1) / 2 + 1 are kept (value <= torch.median(unique), the lower median), else all; levels whose std is NaN
 * are dropped; x[i] = (double)((float)l / (float)scale), y[i] = std[l], compacted in level order; *m (device int32) = their number.  x, y:
 * fp64 [n_levels], NaN past m.
 *
 * nd_theil_sen_f64: TheilSenRegressor().fit for one feature.  A pair (i, j) of curve points gives slope = (y_j - y_i) / (x_j - x_i) and
 * intercept = y_i - slope x_i; the fit is the spatial median of these points exactly as sklearn's _spatial_median and
 * _modified_weiszfeld_step define it: start at the mean; a step forms d = P - old, the mask |d| >= DBL_EPSILON, in_X = (a point was masked
 * out), qn = |sum d / |d||, dir = sum(P / |d|) / sum(1 / |d|) when qn > DBL_EPSILON (else dir = 1, qn = 1),
 * new = max(0, 1 - in_X / qn) dir + min(1, in_X / qn) old, and stops when sum (old - new)^2 < tol^2; if no step stops it, the new of step
 * max_iter is the result.  pairs == NULL (n_pairs = 0): all m (m - 1) / 2 pairs i < j, x strictly increasing (the curve is); else the
 * n_pairs >= 1 pairs of the int32 [n_pairs][2] table (an index outside [0, m) gives a NaN point).  *m is read on the device and clamped to
 * [0, max_m]; x, y hold max_m values (1 <= max_m <= 2^24).  out: fp64 [4] = { intercept, slope, steps taken, pairs used }.  m == 0 gives
 * (0, 0) as the reference returns, m == 1 without a table gives NaN (the reference raises); a pair with equal x is a NaN or infinite point
 * and the result is then not finite (the caller's contract).  All arithmetic is fp64, no pair is stored (a step recomputes them), every
 * sum has a fixed order (per-workgroup partials in workspace slots, the slots summed in order; the grid is a constant, so the bits
 * depend on x, y, m and the table alone).  2 + 2 max_iter
 * plain launches; once the device's done flag is set the remaining ones exit at their first instruction.  1 <= max_iter <= 65536, tol >= 0.
 * Workspace: nd_theil_sen_workspace_bytes(max_m, n_pairs) bytes, 8-byte aligned, needs no zeroing.
 * DEVIATION from the reference: above 141 points sklearn fits a random subset of 10 000 pairs (max_subpopulation, random_state=None) and
 * its result changes from run to run; this library fits ALL pairs and is repeatable.  The pair table lets a caller fit any subset,
 * sklearn's own included. */
int64_t nd_level_table_bytes(int n_levels);
int nd_level_moments_reset(uint64_t* table, int n_levels, uint64_t* counters, void* stream);
int nd_level_moments_f32(const float* clean, const float* noisy, int64_t n, float scale, int n_levels, uint64_t* table, uint64_t* counters,
                         void* stream);
int nd_level_stats_f64(const uint64_t* table, int n_levels, int64_t* count, double* mean, double* std, void* stream);
int nd_level_curve_f64(const int64_t* count, const double* std, int n_levels, float scale, int below_median, double* x, double* y, int32_t* m,
                       void* stream);
int64_t nd_theil_sen_workspace_bytes(int max_m, int64_t n_pairs);
int nd_theil_sen_f64(const double* x, const double* y, const int32_t* m, int max_m, const int32_t* pairs, int64_t n_pairs, int max_iter,
                     double tol, double* out, void* workspace, void* stream);

/* ------------------------------------------------------------------ the denoiser's training batch (dataset_denoising.py:80-168, trainer_denoising.py:100-166,207-217)
 * nd_denoise_batch_f32: ONE launch from generated noise patches to the (noisy, clean) pair TrainableLSID takes.  noise, clean: fp32 NCHW
 * [B][4][patch][patch]; noisy, clean_out: [B][4][crop_h][crop_w].  Per output element (c, y, x), with the row of `table` for its sample:
 *   source row ys = cy + (flip ? crop_h-1-y : y), column xs = cx + x (the flip is torch.flip(dims=[2]): the H axis);
 *   n = clip(noise, -1, 1); v = clip(n + clean, 0, 1); g = clip(clean, 0, 1)   (clips keep NaN);
 *   with the four dark-shading planes (all or none; [4][map_h][map_w] of nd_pack_darkshading_f32; `branch` != 0 reads the high-ISO pair):
 *     im = v / ratio; im = im * 15871 + 512; im = clip(im, 0, 16383); im -= (ds_k[c][y0+ys][x0+xs] * iso + ds_b[c][y0+ys][x0+xs]) + blc;
 *     im = max(im - 512, 0); im = im / 15871; im = im * ratio; v = clip(im, 0, 1)       -- fp32, one IEEE operation each, in this order;
 *   with `sna` ([B][ND_DENOISE_SNA_WORDS] fp32: wb[4], K; NULL = no augmentation; a row whose wb is all zero is skipped):
 *     lam = (double)g * 15871 / ratio * wb[c] / K in fp64, k ~ Poisson(lam) by nd_philox_poisson_f32's generator with element index
 *     c crop_h crop_w + y crop_w + x, sample index first_sample + b and draw index `draw`; then in fp32
 *     gt = g * 15871 / ratio; dy = gt * wb[c]; dn = k * K; dy = dy * ratio / 15871; dn = dn / 15871; dn = dn * ratio;
 *     noisy = v + dn; clean_out = g + dy (no clip); without it noisy = v, clean_out = g.
 * table, sna and rng are DEVICE memory, read by the kernel: a captured graph replays with new crops, flips and augmentations once the
 * caller has rewritten them.  rng ({seed, first_sample, draw} as int64, or NULL) overrides the three arguments, as nd_sampler_state.rng does.
 * counts_in (fp32 [B][4][crop_h][crop_w] or NULL): use these counts and draw nothing; counts_out (or NULL): the counts used (0 where
 * the augmentation is off).  A table row that points outside the patch or the planes gives NaN for its sample and reads nothing.
 * patch, crop_h, crop_w even; noise, clean, counts and outputs 8-byte aligned (16-byte stores when crop_w % 4 == 0 and the outputs allow). */
typedef struct nd_denoise_sample {
    int32_t x0, y0;         /* origin of the patch in the packed frame: where the shading planes are read                   */
    int32_t cx, cy;         /* crop offset inside the patch: even, 0 <= cx <= patch - crop_w, 0 <= cy <= patch - crop_h      */
    int32_t flip;           /* != 0: rows reversed                                                                         */
    int32_t branch;         /* != 0: the high-ISO planes (iso > 1600)                                                      */
    float iso, ratio, blc;  /* blc = blc_mean[iso]                                                                         */
    int32_t reserved[3];
} nd_denoise_sample;
#define ND_DENOISE_SNA_WORDS 8
int nd_denoise_batch_f32(const float* noise, const float* clean, const float* ds_k_high, const float* ds_b_high, const float* ds_k_low,
                         const float* ds_b_low, int map_h, int map_w, const nd_denoise_sample* table, const float* sna, const int64_t* rng,
                         uint64_t seed, int64_t first_sample, int32_t draw, const float* counts_in, float* counts_out, float* noisy,
                         float* clean_out, int B, int patch, int crop_h, int crop_w, void* stream);
/* out[b][i] ~ Poisson((double)rate[b][i]) as fp32, i < n_per_sample: Philox4x32-10 keyed by `seed`, counter {i, first_sample + b, draw, block};
 * uniforms (word + 0.5) 2^-32 in fp64 and every decision in fp64.  rate 0: 0; rate < 10: inversion on word 0 of block 0; else Hoermann's
 * transformed rejection, attempt t on words 2 (t % 2), 2 (t % 2) + 1 of block t / 2.  A negative, NaN or infinite rate gives NaN. */
int nd_philox_poisson_f32(const float* rate, float* out, uint64_t seed, int64_t first_sample, int32_t draw, int B, int64_t n_per_sample,
                          void* stream);
/* A Bayer map [H2][W2] -> planes [4][H2/2][W2/2] in pack_np_raw's channel order: plane c at (Y, X) is bayer[2Y + (c >= 2)][2X + (c == 1 || c == 2)]. */
int nd_pack_darkshading_f32(const float* bayer, float* planes, int H2, int W2, void* stream);

/* ------------------------------------------------------------------ raw Bayer frames (utils/raw_util.py:17-35,112-139, test_denoising.py:86-114,267-293,
 * dataloader/dataset_denoising.py:172-372).  frames: uint16 [N][H2][W2] in DEVICE memory, H2 and W2 even; packed pixel (Y, X) has channel
 * 0 = Bayer (2Y, 2X), 1 = (2Y, 2X+1), 2 = (2Y+1, 2X+1), 3 = (2Y+1, 2X): pack_raw's order and nd_pack_darkshading_f32's.  One row of `table`
 * (DEVICE memory, rewritten between replays of a captured launch) per output sample: output row y of the h x w window reads packed row
 * y0 + (flip ? h-1-y : y) (torch.flip(dims=[2])) and column x0 + x of frame `frame`.  x0, y0: any integers with the window inside the frame
 * (and inside the shading planes where they are read).  A row that points outside gives NaN for its sample and reads nothing.
 * black, white: the sensor's levels (512, 16383); wb = white - black in fp32.  d = (ds_k[c][Y][X] * iso + ds_b[c][Y][X]) + blc in fp32 from
 * the planes of nd_pack_darkshading_f32 (`branch` != 0: the high-ISO pair).  Every operation below is one IEEE operation, in this order. */
typedef struct nd_raw_sample {
    int32_t frame;          /* index of the frame the window is read from                                                  */
    int32_t frame_clean;    /* ND_RAW_TRAIN_REAL: index of the long-exposure frame written to clean_out                      */
    int32_t x0, y0;         /* window origin in packed pixels                                                              */
    int32_t flip;           /* != 0: rows reversed                                                                         */
    int32_t branch;         /* != 0: the high-ISO planes (iso > 1600)                                                      */
    float iso, ratio, blc;  /* blc = blc_mean[iso]                                                                         */
    int32_t reserved;
    double k, sd, ratio64;  /* nd_raw_poisson_gaussian_f32: the gain, sqrt(var) and the ratio in fp64                        */
} nd_raw_sample;
enum nd_raw_mode {
    ND_RAW_PACK = 0,        /* v = max(x - black, 0); ND_RAW_RESCALE: v = v / wb; ND_RAW_CLIP: v = clip(v * ratio, 0, 1)     (pack_raw) */
    ND_RAW_PACK_SHADED = 1, /* v = (x - black) / wb; v = clip(v * ratio, 0, 1); v = v / ratio; v = v * wb + black; v = clip(v, 0, white);
                             * v = v - d; v = max(v - black, 0); v = v / wb; v = clip(v * ratio, 0, 1)
                             * (pack_raw_withdarkshading(...) * ratio and load_image's clip); needs the planes                         */
    ND_RAW_TRAIN_REAL = 2   /* v = max(x - black, 0); v = v - d (with planes); v = v * ratio; v = clip(v, 0, wb); v = v / wb; and
                             * clean_out = max(x' - black, 0) / wb from frame_clean  (RealSonyDenoisingDataset.__getitem__)             */
};
#define ND_RAW_RESCALE 1
#define ND_RAW_CLIP 2
/* out (and clean_out for ND_RAW_TRAIN_REAL, NULL otherwise): fp32 NCHW [B][4][h][w], x = (float)code.  The four planes: all or none,
 * [4][map_h][map_w].  frames and the table 4-byte aligned at least (the table 8-byte), outputs 4-byte; a thread takes 4, 2 or 1 packed
 * columns (the widest that w and the outputs' alignment allow) and loads by the widest form each address allows. */
int nd_raw_pack_u16_f32(const uint16_t* frames, int N, int H2, int W2, const float* ds_k_high, const float* ds_b_high, const float* ds_k_low,
                        const float* ds_b_low, int map_h, int map_w, const nd_raw_sample* table, int mode, int flags, float black, float white,
                        float* out, float* clean_out, int B, int h, int w, void* stream);
/* PossionGaussianDenoisingDataset.apply_noise (:332-345) fused with pack_raw(rescale=False) and the two divisions of __getitem__ (:359-360):
 *   c = max(x - black, 0) (fp32); latent = c / (float)ratio64 (fp32); lam = (double)latent / k; n ~ Poisson(lam); z ~ N(0, 1);
 *   noisy = fl32(clip((k n + sd z) ratio64, 0, wb) / wb), every operation in fp64; clean_out = c / wb (fp32).
 * n: nd_philox_poisson_f32's generator, key = seed, counter {element index c h w + y w + x of the OUTPUT position, first_sample + b, draw,
 * block}.  z: Box-Muller in fp64 on words 0 and 1 of block 32 of the same counter (the Poisson draw stops at block 31):
 * u = (word + 0.5) 2^-32, z = sqrt(-2 log(u0)) cos((2 pi) u1), rounded to fp32 before it is used, so that normals_out replays it exactly.
 * rng ({seed, first_sample, draw} as int64 in device memory, or NULL) overrides the three arguments.  counts_in / normals_in (fp32
 * [B][4][h][w] or NULL) replace the draws; counts_out / normals_out (or NULL) return what was used. */
int nd_raw_poisson_gaussian_f32(const uint16_t* frames, int N, int H2, int W2, const nd_raw_sample* table, const int64_t* rng, uint64_t seed,
                                int64_t first_sample, int32_t draw, const float* counts_in, const float* normals_in, float* counts_out,
                                float* normals_out, float black, float white, float* noisy, float* clean_out, int B, int h, int w,
                                void* stream);
/* The write half of postprocess_bayer (test_denoising.py:267-293).  img: fp32 [B][4][h][w]; out: uint16 [B][2h][2w].  p = clip(x, 0, 1) by
 * comparisons; t = (double)p * (white - bl[c]) + bl[c] in fp64; the code is t truncated toward zero, at channel c's Bayer position; a NaN
 * gives code 0.  bl: black_level_per_channel, four ints in HOST memory, read during the call; 0 <= bl[c] <= white <= 65535. */
int nd_raw_to_bayer_u16(const float* img, uint16_t* out, const int32_t* bl, int white, int B, int h, int w, void* stream);
/* The sample of the diffusion sets (dataloader/dataset.py: SonyTrainDataset.__getitem__ :106-145, NoiseImageGenerationDataset :242-281,
 * GenDarkFrameDataset :376-414) for a batch of windows.  noise, noisy, clean: fp32 NCHW [B][4][h][w]; coord: [B][2][h][w].  Row b of `table`
 * gives the short exposure (frame), the long one (frame_clean), x0, y0 and ratio; flip, branch, iso, blc, k, sd and ratio64 are not read.
 * Output position (y, x) is packed pixel (Y, X) = (y0 + y, x0 + x); x and x' are the short and the long frame's codes as (float), H = H2 / 2,
 * W = W2 / 2, wb = white - black.  One IEEE fp32 operation per step:
 *   sv = x - black; sv = sv < 0 ? 0 : sv; sv = sv / wb; noisy = clip(sv * ratio, 0, 1) by comparisons (a NaN passes through);
 *   g = x' - black; g = g < 0 ? 0 : g; clean = g / wb   -- not clipped: gt_norm is not, and a code above white gives more than 1;
 *   noise = noisy - clean;
 *   coord[0] = (float)Y / (float)(H - 1); coord[1] = (float)X / (float)(W - 1)   -- util.make_coord(H, W, rescale=True) channels first:
 *   the row, then the column, over the WHOLE frame's H and W.
 * Each output may be NULL and is then neither computed nor written; one at least is given.  `frame` is validated and read only for noise or
 * noisy, `frame_clean` only for noise or clean; with coord alone frames may be NULL and N is ignored (the dark-frame set).  A row whose window
 * leaves the frame, or whose needed frame index is outside [0, N), gives NaN in every requested output of its sample and reads nothing.
 * Every refusal is ND_E_BADARG, before any device call: odd sides, a packed side below 2 (the coordinates divide by H - 1 and W - 1), h, w or
 * B <= 0, h > H, w > W, a NULL table, no output, NULL frames with noise, noisy or clean requested, frames or an output not 4-byte aligned.
 * A thread takes 4, 2 or 1 packed columns: the widest that w and the given outputs' alignment allow. */
int nd_raw_diffusion_batch_f32(const uint16_t* frames, int N, int H2, int W2, const nd_raw_sample* table, float black, float white, float* noise,
                               float* noisy, float* clean, float* coord, int B, int h, int w, void* stream);
/* The calibrated physics-based noise model of ELD / PMN on windows of resident frames (physics_noise.hip): Poisson shot noise, Gaussian or
 * Tukey-lambda read noise, row noise, quantisation noise and a bias, the baseline a learned synthesizer is scored against.  Units are codes
 * above black at the short exposure (DN); wb = white - black in fp32.  Output element (c, y, x) of sample b reads packed row
 * Y = y0 + (flip ? h-1-y : y) and column X = x0 + x of frame `frame`.  Every line is one IEEE operation (a product and the sum that takes it
 * are two, no fused multiply-add), in this order:
 *   c0 = max((float)code - black, 0) (fp32); clean_out = c0 / wb (fp32); latent = c0 / (float)ratio (fp32); lamP = (double)latent / K;
 *   n ~ Poisson(lamP): nd_philox_poisson_f32's generator, key = seed, counter {e, first_sample + b, draw, blocks 0..31}, e = c h w + y w + x
 *     of the OUTPUT position (as nd_raw_poisson_gaussian_f32); a lamP that is negative, NaN or infinite gives NaN; K > 0;
 *   r = the unit read variate, rounded to fp32, from block 32 of the same counter, uniforms u = (word + 0.5) 2^-32 in fp64:
 *     read_kind 0: sqrt(-2 log(u0)) cos((2 pi) u1) on words 0 and 1, nd_raw_poisson_gaussian_f32's normal exactly;
 *     read_kind 1: the Tukey-lambda quantile of u2 (word 2): a = log(u2); b = log1p(-u2); lam != 0: p = lam a; q = lam b;
 *       Q = (expm1(p) - expm1(q)) / lam; lam == 0: Q = a - b.  s_read is then the SCALE of the unit variate (scipy.stats.tukeylambda's
 *       scale=, PMN's sigTL), not a standard deviation: the unit variance is 2.06 at lam = 0.149 and 4.61 at lam = -0.091, infinite for
 *       lam <= -0.5.  The expm1 form and not pow: the calibrated |lam| go down to 0.0026.  Any other read_kind gives NaN;
 *   g = the unit row variate, rounded to fp32: the same Box-Muller on words 0 and 1 of counter {4 Y + c, row_stream, draw, block 33}.  One
 *     variate per (absolute row Y, channel c) (PMN's randn(C, H, 1)), keyed by the SOURCE row: a flipped window carries the row noise with
 *     its rows, and windows of one frame that are given one row_stream agree on every row they share;
 *   uq = (float)(u3 - 0.5), word 3 of block 32;
 *   t = K n; t = t + s_read r; t = t + s_row g; t = t + qstep uq; t = t + bias (fp64; a zero scale is still multiplied and added);
 *   t = clip(t, -black, wb) by comparisons, a NaN passes (the sensor's range at the short exposure);
 *   v = t ratio; v = v / wb; with ND_PHYS_CLIP01: v = clip(v, 0, 1); noisy = fl32(v); noise_out = noisy - clean_out (fp32).
 * With read_kind 0, s_row = qstep = bias = 0 and ND_PHYS_CLIP01, noisy has the values of nd_raw_poisson_gaussian_f32 for the same key with
 * k = K and sd = s_read.  `table`: DEVICE memory, rewritten between replays of a captured launch; a row that points outside the frame gives
 * NaN for its sample and reads nothing.  rng ({seed, first_sample, draw} as int64 in device memory, or NULL) overrides the three arguments;
 * row_stream comes from the table alone.  counts, reads, quants: fp32 [B][4][h][w]; rows: fp32 [B][4][h], indexed by the OUTPUT row.  An
 * *_in array replaces its draw, an *_out array returns what was used; each may be NULL, and so may noise_out.  h and w are independent: a
 * whole frame is one window with h = H2 / 2, w = W2 / 2.  A thread takes 4, 2 or 1 packed columns (the widest that w and the alignment of
 * noisy, clean_out, noise_out, counts_out, reads_out and quants_out allow) for all four channels.  One launch, no allocation, no
 * synchronisation.  Every refusal is ND_E_BADARG, before any device call: what nd_raw_poisson_gaussian_f32 refuses (a NULL frames, table,
 * noisy or clean_out, a negative draw, levels outside 0 <= black < white <= 65535, a size that is not positive, B > 65535, odd sides, a
 * window larger than the packed frame, 4 h w >= 2^32, frames or an array not 4-byte aligned, table or rng not 8-byte aligned), and a flag
 * other than ND_PHYS_CLIP01. */
typedef struct nd_physics_sample {          /* 8-byte aligned, 88 bytes */
    int32_t frame;          /* index of the frame the window is read from                                                  */
    int32_t x0, y0;         /* window origin in packed pixels                                                              */
    int32_t flip;           /* != 0: rows reversed                                                                         */
    int32_t read_kind;      /* 0: Gaussian read noise, 1: Tukey-lambda                                                     */
    uint32_t row_stream;    /* counter word 1 of the row variates; the host's default is first_sample + b                  */
    int32_t reserved[2];
    double ratio;           /* exposure ratio                                                                              */
    double K;               /* system gain, DN per electron                                                                */
    double s_read;          /* scale of the read variate, DN                                                               */
    double lam;             /* the Tukey-lambda shape; read with read_kind 1 only                                          */
    double s_row;           /* scale of the row variate, DN                                                                */
    double qstep;           /* quantisation step q * wb, DN                                                                */
    double bias;            /* DN                                                                                          */
} nd_physics_sample;
#define ND_PHYS_CLIP01 1
int nd_raw_physics_noise_f32(const uint16_t* frames, int N, int H2, int W2, const nd_physics_sample* table, const int64_t* rng, uint64_t seed,
                             int64_t first_sample, int32_t draw, const float* counts_in, const float* reads_in, const float* rows_in,
                             const float* quants_in, float* counts_out, float* reads_out, float* rows_out, float* quants_out, float black,
                             float white, int flags, float* noisy, float* clean_out, float* noise_out, int B, int h, int w, void* stream);
/* ------------------------------------------------------------------ calibrating the physics-based model from dark frames (calibrate.hip)
 * What ELD / PMN do on the host with numpy and scipy.stats (row means, ppcc_max, probplot), on uint16 dark frames [N][H2][W2] that stay on the
 * device.  Units are codes (DN).  h = H2 / 2, w = W2 / 2, a frame's n = 4 h w values are ordered (channel, packed row, packed column) with the
 * channels and the Bayer cell of nd_raw_pack_u16_f32.  2 <= h, w <= 32768, 1 <= N <= 32767.  Every entry is plain launches on `stream`: no
 * allocation, no synchronisation, no host read, no floating-point atomics; every fp64 sum has a fixed order (a workgroup's partial in its own
 * workspace slot, the slots summed in slot order, a constant grid per frame), so the bits of a frame depend on that frame alone.  Argument
 * errors are ND_E_BADARG before any device call.
 *
 * nd_dark_stack_add_u16: sums[y][x] += sum over the N frames of their code at (y, x); sums: int32 [H2][W2], 8-byte aligned, zeroed by the
 * caller before the first call.  Integer adds: exact, and the split of the frames over calls does not matter.  The caller counts the frames
 * and stops at 32767 (32767 * 65535 < 2^31).  nd_dark_stack_mean_f64: mean[y][x] = (double)sums[y][x] / (double)count, one IEEE division.
 *
 * The integer pixel value: t = D code - P, with D = 1 and P = black when T is NULL, and D = N and P = T[y][x] (the sums of a dark stack over
 * these N frames) otherwise: N times the deviation from the mean dark frame, the fixed pattern gone exactly.  0 <= black <= 65535.
 * nd_calib_row_sums_i64: R[n][c][Y] = sum over X of t, int64 [N][4][h], exact.  One wave per (frame, packed row).
 * nd_calib_residual_f64: x[n][c][Y][X] = (double)(t w - R[n][c][Y]) / (double)(w D), fp64 [N][4 h w], 16-byte aligned: the numerator is an
 *   exact integer below 2^53 and the denominator is exact, so x is the correctly rounded deviation of a pixel from its row's mean.
 * Both read V = 4, 2 or 1 packed columns per thread (the widest w allows), as the raw entries do.
 * nd_calib_row_stats_f64: out fp64 [N][8] = { sigR_pmn, sigR, bias[0..3], V_x, 0 } per frame.  With S_c = sum_Y R[c][Y] and Q_c = sum_Y R[c][Y]^2
 *   as integers: bias[c] = (double)S_c / (double)(h w D); v = fl(sum_c (h Q_c - S_c^2)) / (double)(4 h h) / (double)(w D) / (double)(w D), the
 *   integer formed exactly in 128 bits and converted once: the ddof-0 variance of the 4 h row means about their channel's mean;
 *   sigR_pmn = sqrt(v); V_x = var_x[n * var_stride] (fp64, DEVICE memory: the ddof-0 variance of the frame's x, nd_probplot_f64's out[4]);
 *   sigR = sqrt(max(v - V_x / (double)(w - 1), 0)), a NaN passing.
 *
 * Probability plots of SORTED values xs: fp64 [N][n], ascending per frame, 3 <= n.  The order-statistic medians are scipy's: m[n-1] = 0.5^(1/n)
 * (pow on the host), m[0] = 1 - m[n-1], m[i-1] = ((double)i - 0.3175) / ((double)n + 0.365).  The theoretical quantile q of m: kind 1, the unit
 * Tukey-lambda one in nd_raw_physics_noise_f32's form, a = log m; b = log1p(-m); lam != 0: (expm1(lam a) - expm1(lam b)) / lam; lam == 0: a - b;
 * kind 0, the standard normal one (normcdfinv).  Every element is evaluated: the twin -q of m[n-1-i] is NOT used, because 1 - m[i] is not
 * m[n-1-i] in fp64.  nd_calib_quantiles_f64 writes q[0..n) for one shape (what the sums below are made of).
 * One evaluation forms, with xc = x - xs[n / 2] (a shift, so that the one-pass sums do not cancel), S = { sum xc, sum q, sum xc^2, sum q^2,
 * sum xc q } and from them cxx = S2 - S0 S0 / n, cqq = S3 - S1 S1 / n, cxq = S4 - S0 S1 / n; slope = cxq / cqq; mean = xs[n / 2] + S0 / n;
 * intercept = mean - slope (S1 / n); r = cxq / (sqrt(cxx) sqrt(cqq)) clipped to [-1, 1] by comparisons: scipy.stats.probplot's
 * (slope, intercept, r).  A constant frame gives r = NaN.
 * nd_probplot_f64: one evaluation per frame; out fp64 [N][6] = { slope, intercept, r, mean, cxx / n, 0 }.  lam: fp64 [N] in DEVICE memory
 *   (kind 1), NULL with kind 0.
 * nd_ppcc_max_f64: scipy.stats.ppcc_max with a bounded bracket: Brent's bounded minimisation (golden section and parabolic steps, the
 *   algorithm of scipy.optimize.minimize_scalar(method="bounded") statement by statement) of 1 - r(lam) on (lo, hi), per frame, the state in
 *   the workspace.  2 max_eval + 1 launches: an evaluation over grid (slots, N) and a one-workgroup-per-frame step that sums the slots,
 *   updates the bracket and writes the next lam; once a frame's done flag is set its workgroups return at once.  out fp64 [N][3] = { lam,
 *   r, evaluations }.  The search of a frame ends when |xf - xm| <= 2 tol1 - (b - a) / 2 with tol1 = sqrt(2.2e-16) |xf| + xtol / 3, after
 *   max_eval evaluations, or at a NaN objective (then lam = r = NaN).  -0.5 < lo < hi, xtol > 0, 3 <= max_eval <= 64.
 * Workspace of both: nd_ppcc_workspace_bytes(N) bytes, 8-byte aligned, needs no zeroing. */
int nd_dark_stack_add_u16(const uint16_t* frames, int N, int H2, int W2, int32_t* sums, void* stream);
int nd_dark_stack_mean_f64(const int32_t* sums, int H2, int W2, int count, double* mean, void* stream);
int nd_calib_row_sums_i64(const uint16_t* frames, int N, int H2, int W2, const int32_t* T, int black, int64_t* R, void* stream);
int nd_calib_residual_f64(const uint16_t* frames, int N, int H2, int W2, const int32_t* T, int black, const int64_t* R, double* x, void* stream);
int nd_calib_row_stats_f64(const int64_t* R, int N, int h, int w, int D, const double* var_x, int var_stride, double* out, void* stream);
int nd_calib_quantiles_f64(int64_t n, int kind, double lam, double* q, void* stream);
int64_t nd_ppcc_workspace_bytes(int N);
int nd_probplot_f64(const double* xs, int N, int64_t n, int kind, const double* lam, double* out, void* workspace, void* stream);
int nd_ppcc_max_f64(const double* xs, int N, int64_t n, double lo, double hi, double xtol, int max_eval, double* out, void* workspace,
                    void* stream);
/* Whole synthetic noisy frames from sampled patches (frame.hip): one launch scatters the OWNED rectangle of each patch of a batch into
 * frame-sized outputs.  patches: fp32 NCHW [B][4][c][c], what the sampler returns for c x c patches of io.patch_grid; frames: the long exposures,
 * uint16 [N][H2][W2] as above, or NULL for dark frames; H = H2 / 2, W = W2 / 2.  Row b of `table` (DEVICE memory, rewritten between replays of a
 * captured launch) places patch b: its origin (x0, y0) in packed pixels of frame `frame_clean`, and the rectangle [ax0, ax1) x [ay0, ay1) of
 * output frame `frame_out`, in frame coordinates, that it owns.  Packed pixel (Y, X) of the rectangle takes n = patches[b][ch][Y - y0][X - x0]:
 *   noise: fp32 [F][4][H][W] = n, bits unchanged (a NaN stays a NaN);
 *   noisy: fp32 [F][4][H][W] = io.compose_noisy against the long exposure, one IEEE fp32 operation per step, no fused multiply-add:
 *     g = (float)x' - black; g = g < 0 ? 0 : g; clean = g / wb  (nd_raw_diffusion_batch_f32's clean, not clipped; 0 with frames NULL);
 *     nc = clip(n, -1, 1); noisy = clip(nc + clean, 0, 1), both by comparisons (a NaN passes through);
 *   short_out: uint16 [F][2H][2W], the frame as the sensor would have recorded it at the short exposure, channel ch at the Bayer site
 *     nd_raw_to_bayer_u16 uses: p = noisy, NaN -> 0; t = (double)p * (double)wb; t = t / (double)ratio; t = t + (double)black; t = t + 0.5;
 *     code = min(trunc(t), white): rounded to nearest, so that packing the frame back is unbiased.
 * Each output may be NULL and is then neither computed nor written; one at least is given.  An empty rectangle is valid and writes nothing.
 * A row writes nothing either when it is invalid: frame_out outside [0, F), frame_clean outside [0, N) where the frames are read, a patch
 * window that leaves the frame, a rectangle that leaves its patch window, or, with short_out, a ratio that is not positive and finite.
 * Rectangles of one launch that share pixels of one output frame give an undefined result there (no atomics; the host side refuses them).
 * A thread takes an aligned run of 4, 2 or 1 packed columns of the FRAME (the widest that W and the given outputs' alignment allow); a run cut by
 * a rectangle's edge is done column by column, with the same arithmetic.  All offsets are 64-bit.  No allocation, no synchronisation.
 * Every refusal is ND_E_BADARG, before any device call: odd or non-positive sides, c, B or F <= 0, B > 65535, c > H or c > W, a NULL table or
 * NULL patches, no output, frames given with noisy or short_out requested and N <= 0, levels outside 0 <= black < white <= 65535, a pointer
 * that is not 4-byte aligned. */
typedef struct nd_frame_patch {
    int32_t frame_out;      /* index of the output frame, [0, F)                                                           */
    int32_t frame_clean;    /* index of the long exposure in `frames`, [0, N); not read with frames NULL                    */
    int32_t x0, y0;         /* patch origin in packed pixels                                                               */
    int32_t ax0, ay0;       /* the owned rectangle, frame coordinates: first column and row                                */
    int32_t ax1, ay1;       /* one past its last column and row                                                            */
    float ratio;            /* exposure ratio of the short frame; read for short_out only                                  */
    int32_t reserved[3];
} nd_frame_patch;
int nd_frame_assemble(const float* patches, const uint16_t* frames, int N, int H2, int W2, const nd_frame_patch* table, float black, float white,
                      float* noise, float* noisy, uint16_t* short_out, int B, int c, int F, void* stream);
/* A packed RAW frame developed to an sRGB picture (develop.hip): what test_denoising.py's postprocess_bayer gets from
 * rawpy.postprocess(use_camera_wb=True, half_size=True, no_auto_bright=True, output_bps=8, bright=1), LibRaw's develop steps restated; also
 * half_size=False with the bilinear demosaic and output_bps=16.  NOT checked against LibRaw bit for bit: the yardstick is tests/render_ref.py.
 * Integer arithmetic except where fp32 is named; every fp32 step is one IEEE operation in the written order, no fused multiply-add.
 * The source is ONE of src_f32 (fp32 [B][4][H][W], channels as above) and src_u16 (uint16 [B][2H][2W]), the other NULL; H, W: the packed frame.
 * Per CFA value of channel c:
 *   from a code x: v = max(x - black[c], 0); from a packed value: x is nd_raw_to_bayer_u16's code first (clip by comparisons, NaN -> 0,
 *   t = (double)p * (white - black[c]) + black[c], truncated), then the same v;
 *   s = min(trunc(fl32(v) * scale_mul[c]), 65535), one fp32 multiply, truncation toward zero.
 * full = 0: window pixel (y, x) = packed pixel (y0 + y, x0 + x) gives one output pixel, R = s0, G = (s1 + s3) >> 1, B = s2; out is [B][h][w][3].
 * full = 1: every site (r, q) of the window's 2h x 2w mosaic gives one output pixel; out is [B][2h][2w][3].  The site keeps its own colour's s
 *   (both greens are G); each missing colour is floor(sum / count) over the sites of that colour in the 3 x 3 window around (r, q) that lie inside
 *   the FRAME (not the window): (a + b) >> 1 at green sites and (a + b + c + d) >> 2 at red and blue sites in the interior, the mean of the 1 to 3
 *   sites there are on the frame's outermost ring (dcraw's lin_interpolate and border_interpolate(1)).
 * Colour and tone, for output channel k: o = 0 + R * rgb_cam[3k]; o = o + G * rgb_cam[3k + 1]; o = o + B * rgb_cam[3k + 2] in fp32, each product
 *   rounded before it is added; u = clip((int)o, 0, 65535), truncation toward zero; the value written is curve[u] >> 8 as uint8 (bps = 8) or
 *   curve[u] as uint16 (bps = 16), channels interleaved.
 * params: HOST memory, read during the call; the B images share it.  curve: uint16[65536] in DEVICE memory, 16-byte aligned.  The sources and
 * out: 4-byte aligned (ND_E_ALIGN).  ND_E_SHAPE, before any launch: a window that leaves the frame, a side above 2^24.  ND_E_BADARG: a null
 * pointer, both or neither source, a non-positive size, B > 65535, bps not 8 or 16, full not 0 or 1, white outside (0, 65535], a black level
 * outside [0, white], a scale_mul that is negative or not finite, an rgb_cam entry that is not finite.  Nothing allocates or synchronises. */
typedef struct nd_develop_params {
    int32_t black[4];       /* black_level_per_channel                                                                    */
    int32_t white;          /* the white point of the packed values (16383)                                               */
    float scale_mul[4];     /* fl32((double)pre[c] * 65535.0 / maximum), pre = the camera multipliers over their smallest */
    float rgb_cam[9];       /* camera to sRGB, row-major 3 x 3                                                            */
    int32_t x0, y0;         /* window origin in packed pixels                                                             */
    int32_t bps;            /* 8 or 16                                                                                    */
    int32_t full;           /* 0: half size; 1: full resolution, bilinear                                                 */
} nd_develop_params;
int nd_raw_develop(const float* src_f32, const uint16_t* src_u16, int B, int H, int W, const nd_develop_params* params, const uint16_t* curve,
                   void* out, int h, int w, void* stream);
/* (cout, cin) row-major (Linear / 1x1 conv weight) -> [cinP/4][coutP][4]; `unshuffle_c` > 0
 * permutes K from (c p1 p2) to (p1 p2 c) for a pixel-unshuffled input with c = unshuffle_c. */
int64_t nd_pack_pointwise_weight_floats(int cin, int cout);
int nd_pack_pointwise_weight(const float* w, float* packed, int cin, int cout, int unshuffle_c, void* stream);
/* training: the packing of the DATA-GRADIENT operator dx = dy @ W of a Linear / 1x1 convolution (res_conv, Mlp.fc1 / fc2, FeedForward:
 * Diffusion_arch.py:156,345-347,410-419), read in place from its forward weight
 * `w_t` ((cin, cout) row-major here = torch's (out_features, in_features) of the forward layer; cin = the forward layer's cout). */
int nd_pack_pointwise_weight_t(const float* w_t, float* packed, int cin, int cout, void* stream);
/* Many packings in ONE launch (training: the forward and the data-gradient packing of every Linear / 1x1 weight once per optimizer step;
 * noisediff_amd/train.py keeps the table).  `items_dev`: n_items records in DEVICE memory; item i packs `w` ((cout, cin) row-major, or with
 * `transposed` the forward weight (cin, cout) of the layer whose data gradient this packing serves) into `packed` (nd_pack_pointwise_weight_floats
 * floats), exactly as nd_pack_pointwise_weight / nd_pack_pointwise_weight_t do. */
int nd_pack_pointwise_weights_batch(const nd_pack_item* items_dev, int n_items, void* stream);

/* The same operator (same descriptor, prologues, epilogues, errors) with every product on the bf16 matrix cores at the operands' FULL fp32
 * significand: each fp32 operand is split exactly into three bf16 terms (v = v1 + v2 + v3, round-to-nearest-even remainders), six of the nine
 * term products are kept (the dropped ones lie below 2^-25 of the product -- under the rounding of an fp32 FMA), accumulation in fp32.  Replaces
 * the same reference layers as nd_pointwise_gemm_nhwc_f32 where they are wide: FeedForward's Linears and AttnBlock.proj_out at C >= 128
 * (Diffusion_arch.py:405-443), res_conv of the up path (:156), Attention.to_qkv / to_out (:252-253).  `weight`: nd_pack_pointwise_weight_split
 * ((cout, cin) row-major -> [cin/16][term 3][cout/32][64 lanes][8 bf16]).  Takes: cin % 32 == 0, cin >= 64, cout % 128 == 0, plain pixel
 * addressing, LayerNorm with src.rowstats, a concat on a 32-channel boundary; anything else: ND_E_SHAPE.
 * The questions, like nd_conv3x3_takes (1 / 0, no HIP call, nd_last_error untouched; the only statement of the limits, csrc/pointwise.hip): does
 * nd_pointwise_gemm_nhwc_f32 / nd_pointwise_gemm_split_nhwc_f32 take a layer of this shape?  They read the descriptor's sizes, widths, strides and modes and,
 * of its pointers, only whether src.rowstats is given; the split question includes the fp32 one. */
int nd_pointwise_gemm_split_nhwc_f32(const nd_pointwise* d, void* stream);
int nd_pointwise_gemm_takes(const nd_pointwise* d);
int nd_pointwise_gemm_split_takes(const nd_pointwise* d);
int64_t nd_pack_pointwise_weight_split_floats(int cin, int cout);
int nd_pack_pointwise_weight_split(const float* w, float* packed, int cin, int cout, void* stream);

/* Downsample = pixel-unshuffle + 1x1 (Diffusion_arch.py:80-81) on the streaming kernels: the same descriptor as nd_pointwise_gemm_nhwc_f32 with
 * src.unshuffle = 1 (the source is the (2 H, 2 W) image with c0 / 4 channels at a pixel stride of ld0; HW, W: the OUTPUT's), staged as the plain source with a
 * doubled pixel and row stride plus one constant per 32-channel chunk.  cout % 128 == 0: the split-product kernel, `weight` an
 * nd_pack_pointwise_weight_split_unshuffle packing (unshuffle_c = cin / 4; nd_pack_pointwise_weight_split_floats floats); otherwise the pipelined fp32 kernel,
 * `weight` an nd_pack_pointwise_weight packing with unshuffle_c = cin / 4.  Takes (nd_pointwise_downsample_takes: 1 / 0, no HIP call, nd_last_error untouched; it
 * reads the sizes, widths, strides and modes and WHETHER res0 / res1 / gn_t / vec are given): one source, (c0 / 4) % 32 == 0, cout % 64 == 0, no prologue, no
 * residual operands, no output shuffle; anything else: ND_E_SHAPE. */
int nd_pointwise_downsample_nhwc_f32(const nd_pointwise* d, void* stream);
int nd_pointwise_downsample_takes(const nd_pointwise* d);
int nd_pack_pointwise_weight_split_unshuffle(const float* w, float* packed, int cin, int cout, int unshuffle_c, void* stream);

/* The tail of a wide AttnBlock (Diffusion_arch.py:434-443), ff.net.2 then proj_out with only additions between them, as ONE linear map over [h1; x]:
 *   y = Wp (W2 h1 + b2 + x + cb) + bp + x = [Wp W2 | Wp + I] [h1; x] + (Wp b2 + bp) + Wp cb.
 * nd_pack_attn_tail_fold writes w_out (C, 3 C) row-major = [Wp W2 | Wp + I] and b_out [C] = Wp b2 + bp from W2 (C, 2 C) and Wp (C, C) in torch layout, every
 * C-term sum in fp64 on the device and rounded once to fp32 (b2 / bp may be NULL: zeros); nd_pack_attn_tail_fold_floats(C) = 3 C C, the floats of w_out.
 * The GEMM is nd_pointwise_gemm_split_nhwc_f32 on nd_pack_pointwise_weight_split(w_out, cin = 3 C, cout = C) with the sources (h1, x) and
 * vec = Wp cb + b_out per sample (proj_out itself over the rows of cb, with b_out as its bias). */
int64_t nd_pack_attn_tail_fold_floats(int C);
int nd_pack_attn_tail_fold(const float* w2, const float* b2, const float* wp, const float* bp, float* w_out, float* b_out, int C, void* stream);

/* Two 1x1 layers with nothing between them but an addition, the second one narrow (cout 4 or 8), as ONE streaming dot product -- the end of the
 * U-Net, final_conv(res_conv(cat(xp, x0)) + silu(GN(c2))) + shot (Diffusion_arch.py:156,170,554,644):
 *   out[p] = W [p0[p]; p1[p]; silu((t[p] - M[b]) * A[b] + D[b])] + bias [+ res0[p]],    W = [Wf Wr | Wf],  bias = Wf br + bf
 * `weight` / `bias` are nd_pack_narrow_fold's outputs ([cin/4][cout][4] and [cout], cin = c0 + c1 + c2 = cin_r + mid): the mid-term sums of
 * Wf (cout, mid) times Wr (mid, cin_r) and of Wf br + bf are formed in fp64 and rounded once to fp32; nd_pack_narrow_fold_floats: the floats of
 * `weight`.  mad: [B][3][c2] as nd_groupnorm_finalize_f32 writes it.  Any pixel count.  Takes (nd_pointwise_narrow_fold_takes): channel counts
 * in fours, p1 optional (c1 = 0), cout 4 or 8, cin * cout <= 8192; anything else: ND_E_SHAPE.  Strides multiples of 4, pointers 16-byte aligned. */
typedef struct nd_narrow_fold {
    const float* p0; const float* p1;   /* plain sources [B][HW] x ld0 / ld1 (c0 / c1 channels); p1 NULL iff c1 == 0 */
    const float* t;  const float* mad;  /* the activated source x ldt (c2 channels) and its per-sample M | A | D     */
    const float* weight; const float* bias;
    const float* res0;                  /* [B][HW] x ldr0 or NULL                                                    */
    float*   out;
    int32_t  B, HW, c0, c1, c2, ld0, ld1, ldt, cout, ldo, ldr0, reserved;
} nd_narrow_fold;
int nd_pointwise_narrow_fold_nhwc_f32(const nd_narrow_fold* d, void* stream);
int nd_pointwise_narrow_fold_takes(int c0, int c1, int c2, int cout);
int64_t nd_pack_narrow_fold_floats(int cin, int cout);
int nd_pack_narrow_fold(const float* wf, const float* bf, const float* wr, const float* br, float* w_out, float* b_out, int cin_r, int mid, int cout,
                        void* stream);

/* ------------------------------------------------------------------ chained pointwise layers
 * Two or three per-pixel Linear layers in one kernel, the intermediate activations never leaving registers:
 *   Mlp (Diffusion_arch.py:340-356):            out = fc2(act(fc1(x)))
 *   AttnBlock tail (:405-443, with src.vec = v): out = proj_out(ff2(GELU(ff1(LN(x + v)))) + x + v) + x
 * src: p0/p1 virtual concat, mode ND_PRO_NONE or ND_PRO_LAYERNORM (gamma, beta; src.vec[b] is added to the row first).
 * Stage i computes  h = act_i(W_i . h_prev + bias_i + res_i)  with res_i one of enum nd_chain_res.  Weights come from
 * nd_pack_chain_weight (operand order of the transposed MFMA product, K padded to 8 for the first stage and to 32 for
 * the later ones, N to 32).  Only the width combinations NoiseDiffNet uses are instantiated
 * (nd_pointwise_chain_supported); HW must be a multiple of 32. */
enum nd_chain_res { ND_CHAIN_RES_NONE = 0, ND_CHAIN_RES_INPUT = 1 /* + x + v */, ND_CHAIN_RES_INPUT_RAW = 2 /* + x */ };
typedef struct nd_chain_stage {
    const float* weight;
    const float* bias;     /* [cout] or NULL */
    int32_t  cin, cout;
    int32_t  act;          /* enum nd_act, applied after bias and residual */
    int32_t  res;          /* enum nd_chain_res; needs cout == input width */
} nd_chain_stage;
typedef struct nd_chain {
    nd_src   src;
    nd_chain_stage st[3];
    float*   out;
    int32_t  n_stages, B, HW, ldo;
} nd_chain;
int nd_pointwise_chain_nhwc_f32(const nd_chain* d, void* stream);
int nd_pointwise_chain_supported(int cin, int n1, int n2, int n3);   /* n3 = 0: two stages */
int nd_pointwise_chain_takes(int HW, int cin, int n1, int n2, int n3);   /* the same and HW a positive multiple of 32: what both chain entries take */
int64_t nd_pack_chain_weight_floats(int cin, int cout, int first_stage);
int nd_pack_chain_weight(const float* w, float* packed, int cin, int cout, int first_stage, void* stream);
/* The same chains (same descriptor, widths, prologues, residuals, errors) with the products on the bf16 matrix cores at full fp32 significand
 * (three-term split, six products, fp32 accumulation: see nd_pointwise_gemm_split_nhwc_f32); the stages' `weight` pointers are
 * nd_pack_chain_weight_split packings (three bf16 terms per value in the operand order of v_mfma_f32_32x32x16_bf16, K padded to 16 for the first
 * stage and to 32 for the later ones, N to 32). */
int nd_pointwise_chain_split_nhwc_f32(const nd_chain* d, void* stream);
int64_t nd_pack_chain_weight_split_floats(int cin, int cout, int first_stage);
int nd_pack_chain_weight_split(const float* w, float* packed, int cin, int cout, int first_stage, void* stream);
/* A two-stage split chain behind a ResnetBlock tail (the shot-noise branch's end, shot_mlp3(shot_time(s2) + r): Diffusion_arch.py:168-170,603-604):
 * the chain's input row is  silu((t - M[b]) * A[b] + D[b]) + r0 [+ r1]  with t = chain.src.p0 (one plain source, ND_PRO_NONE, no vec), mad [B][3][cin]
 * as nd_groupnorm_finalize_f32 writes it -- what nd_affine_silu_add_f32 would store and the chain read back.  Stages without residuals; weights are
 * nd_pack_chain_weight_split packings.  Widths: cin 64 or 48, first stage up to 64 wide, second up to 32 (nd_pointwise_chain_tail_takes, n3 = 0);
 * anything else is refused with ND_E_SHAPE -- run the two launches.  HW a multiple of 32, tensors below 4 GiB, strides multiples of 4. */
typedef struct nd_chain_tail {
    nd_chain chain;
    const float* mad;
    const float* r0;       /* [B][HW] x ldr0 */
    const float* r1;       /* [B][HW] x ldr1 or NULL */
    int32_t  ldr0, ldr1;
} nd_chain_tail;
int nd_pointwise_chain_tail_split_nhwc_f32(const nd_chain_tail* d, void* stream);
int nd_pointwise_chain_tail_takes(int cin, int n1, int n2, int n3);

/* ------------------------------------------------------------------ GroupNorm plumbing */

/* Combine conv partials (Chan's parallel variance, fp64) into per-(b, group) mean / rstd
 * (nn.GroupNorm eps, biased variance) and fold gamma/beta and the optional time
 * scale/shift into M, A, D so that Block.forward's  GN -> x*(scale+1)+shift  (:137-141)
 * becomes (x - M) * A + D.  scale/shift: [B] rows of stride ld_ss, scale at +0, shift at +cout. */
int nd_groupnorm_finalize_f32(const float* stats, const float* slot_count, int slots,
                              const float* gamma, const float* beta,
                              const float* scale_shift, int ld_ss,
                              float* mad, int B, int C, int groups, float eps, void* stream);
/* training (Block.forward under p_losses): the same finalize, which also saves `mean_rstd` [B][groups][2] for the backward pass
 * (nd_groupnorm_silu_train_backward_f32) -- the convolution's statistics epilogue then feeds the norm in training as it does in sampling,
 * and the forward tail is nd_affine_silu_add_f32. */
int nd_groupnorm_finalize_train_f32(const float* stats, const float* slot_count, int slots, const float* gamma, const float* beta,
                                    const float* scale_shift, int ld_ss, float* mad, float* mean_rstd, int B, int C, int groups, float eps,
                                    void* stream);

/* Per-pixel LayerNorm statistics over channels of (x + vec[b]): stats[p] = {mean, 1/sqrt(var + eps)}
 * (nn.LayerNorm: biased variance; AttnBlock.norm2, Diffusion_arch.py:430,439).  vec may be NULL. */
int nd_layernorm_stats_f32(const float* x, int ldx, const float* vec, float* stats,
                           int B, int HW, int C, float eps, void* stream);

/* out = silu((t - M)*A + D) [+ res0] [+ res1]: the tail of ResnetBlock.forward (:168-170)
 * when res_conv is the identity, plus `shot_emb + r` (:603). */
int nd_affine_silu_add_f32(const float* t, int ldt, const float* mad,
                           const float* res0, int ldr0, const float* res1, int ldr1,
                           float* out, int ldo, int B, int HW, int C, void* stream);

/* ------------------------------------------------------------------ small dense ops on rows */

/* out[b, n] = act_out( sum_k act_in(in[b, k]) * W[n, k] + bias[n] ), W in torch (N, K) layout.
 * time_mlp (:502-507), every ResnetBlock.mlp (:149-152, batched as one tall matrix),
 * CrossAttention.to_v / to_out on the 1-token context (:385,:402). */
int nd_linear_rows_f32(const float* in, int ld_in, const float* W, const float* bias,
                       float* out, int ld_out, int B, int K, int N,
                       int act_in, int act_out, void* stream);
/* SinusoidalPosEmb.forward (:100-107): emb[b] = cat(sin(t*f), cos(t*f)), t int64 -> fp32 multiply.
 * freqs[half] = exp(arange(half) * -(ln(theta)/(half-1))) is a constant of the model, computed
 * once on the host so that the angle t*f is bit-identical to the reference's. */
int nd_sinusoidal_time_emb_f32(const int64_t* time, const float* freqs, float* emb, int B, int half, void* stream);
/* The whole time conditioning of one diffusion step in one launch (SURVEY 8b minimum symbol set):
 * out[b, j] = (Wp . silu(W2 . gelu(W1 . emb(time[b]) + b1) + b2) + bp)[j] with emb = SinusoidalPosEmb (:100-107), W1/W2 =
 * time_mlp[1]/[3] (:502-507), Wp/bp = every ResnetBlock.mlp[1] Linear stacked into one (J, 4 dim) matrix (:149-152; the SiLU
 * is ResnetBlock.mlp[0]).  Weights in torch (N, K) layout.  Dynamic LDS: nd_cond_step_lds_bytes(B, dim) <= 160 KB. */
int64_t nd_cond_step_lds_bytes(int B, int dim);
int nd_cond_step_f32(const int64_t* time, const float* freqs, const float* W1, const float* b1, const float* W2, const float* b2,
                     const float* Wp, const float* bp, float* out, int ld_out, int B, int dim, int J, void* stream);
/* The same step with the head (emb -> time_mlp -> SiLU) looked up instead of computed: `table` (table_rows x 4 dim) holds the head's result for
 * timestep = row index, built once per weight set by nd_cond_table_build_f32 (same kernel code: the very same bits).  A timestep outside the
 * table falls back to computing the head.  Replaces the same ATen call sites as nd_cond_step_f32 (Diffusion_arch.py:100-107, 502-507, 149-152). */
int nd_cond_table_build_f32(const float* freqs, const float* W1, const float* b1, const float* W2, const float* b2, float* table, int rows, int dim,
                            void* stream);
int nd_cond_step_table_f32(const int64_t* time, const float* freqs, const float* W1, const float* b1, const float* W2, const float* b2,
                           const float* Wp, const float* bp, float* out, int ld_out, int B, int dim, int J, const float* table, int table_rows,
                           void* stream);
/* ... and with the projection tabulated as well: `ptable` (table_rows x J, row t = the J outputs for timestep t, filled by calling nd_cond_step_table_f32 on the
 * timesteps 0 .. table_rows-1 with ld_out = J).  When every sample's timestep lies in the table the launch copies B rows (the same bits); otherwise it computes. */
int nd_cond_step_ptable_f32(const int64_t* time, const float* freqs, const float* W1, const float* b1, const float* W2, const float* b2,
                            const float* Wp, const float* bp, float* out, int ld_out, int B, int dim, int J, const float* table, int table_rows,
                            const float* ptable, void* stream);
/* nn.Embedding lookup (:591): out[b] = table[idx[b]], idx int64. */
int nd_embedding_rows_f32(const int64_t* idx, const float* table, float* out, int B, int rows, int dim, void* stream);

/* ------------------------------------------------------------------ full-resolution special layers */

/* init_conv: nn.Conv2d(4, cout, 7, padding=3) (:478,:606).  x NHWC with 4 channels;
 * weight packed [7*7*4][cout] by nd_pack_conv7x7_weight. */
int nd_conv7x7_c4_f32(const float* x, const float* wpacked, const float* bias, float* out, int ldo,
                      int B, int H, int W, int cout, void* stream);
/* training: weight and bias gradient of that stem, dw (cout, 4, 7, 7) OIHW = sum over the pixels of dy[p][co] x[p + tap][ci] (zero padding) and
 * db[co] = sum dy[p][co]; x NHWC with 4 channels, dy NHWC with pixel stride ldy.  The patch matrix is never built (GEMM with K = pixels straight from a
 * halo tile in LDS); fixed summation order (bitwise repeatable).  Taken for H % 4 == 0, W % 32 == 0, cout in {32, 48, 64, 96, 128}:
 * nd_conv7x7_c4_wgrad_workspace_floats returns -1 otherwise (unfold the image and use nd_linear_wgrad_f32).  dbias may be NULL. */
int64_t nd_conv7x7_c4_wgrad_workspace_floats(int B, int H, int W, int cout);
int nd_conv7x7_c4_wgrad_f32(const float* x, const float* dy, int ldy, float* dw_oihw, float* dbias, float* workspace, int B, int H, int W, int cout,
                            void* stream);
int nd_pack_conv7x7_weight(const float* oihw, float* packed, int cout, void* stream);
/* The same stem (same arguments, shapes, errors) with the products on the bf16 matrix cores at the operands' full fp32 significand: three bf16 terms per
 * fp32 value, six of nine term products, fp32 accumulation (see nd_pointwise_gemm_split_nhwc_f32).  `wsplit`: nd_pack_conv7x7_weight_split
 * ((cout, 4, 7, 7) OIHW -> [cout/32][13 K steps][term 3][64 lanes][8 bf16], nd_pack_conv7x7_weight_split_floats(cout) floats). */
int nd_conv7x7_c4_split_f32(const float* x, const float* wsplit, const float* bias, float* out, int ldo,
                            int B, int H, int W, int cout, void* stream);
int64_t nd_pack_conv7x7_weight_split_floats(int cout);
int nd_pack_conv7x7_weight_split(const float* oihw, float* packed, int cout, void* stream);
/* LearnedSinusoidalPosEmb (:331-337): position NCHW (B,2,H,W) -> NHWC (B,H,W,3*hid):
 * w = conv1x1(position); cat(w, sin(2 pi w), cos(2 pi w)). */
int nd_pos_enc_f32(const float* position_nchw, const float* w /*[hid][2]*/, const float* bias,
                   float* out, int B, int H, int W, int hid, void* stream);
/* nn.MaxPool2d(2, 2, ceil_mode=True) on NHWC (SID_arch.py:60): out (ceil(H/2), ceil(W/2)). */
int nd_maxpool2x2_nhwc_f32(const float* in, float* out, int B, int H, int W, int C, void* stream);
/* layout plumbing for the 4-channel API tensors (reference tensors are NCHW) */
int nd_nchw_to_nhwc_f32(const float* in, float* out, int B, int C, int H, int W, void* stream);
int nd_nhwc_to_nchw_f32(const float* in, float* out, int B, int C, int H, int W, void* stream);
/* NCHW (B,C,H,W) -> NHWC with Cpad >= C channels, the tail zero-filled (a 4-channel image as an 8-channel conv input) */
int nd_nchw_to_nhwc_pad_f32(const float* in, float* out, int B, int C, int H, int W, int Cpad, void* stream);

/* ------------------------------------------------------------------ sampler */

/* Device-resident loop state so that one captured step graph can be replayed T times:
 * step counter, current/next timestep table and the per-timestep coefficient table. */
typedef struct nd_sampler_state {
    int32_t* step;          /* [1] device counter, incremented by nd_sampler_advance       */
    const int32_t* t_cur;   /* [n_steps] timestep fed to the network at each step          */
    const int32_t* t_next;  /* [n_steps] DDIM: next timestep (-1 at the end); DDPM unused  */
    const float* coef;      /* [n_steps][8] per-step scalars, see sampler.hip              */
    int64_t* time_out;      /* [B] int64 buffer the network's time embedding reads         */
    const int64_t* rng;     /* [2] device {seed, first_sample} or NULL.  When set it OVERRIDES the seed /
                               first_sample arguments of nd_sampler_step_*: a captured step graph then
                               serves every seed and every rank shard (no re-capture per sample() call) */
    int32_t n_steps, B;
} nd_sampler_state;

/* time_out[b] = t_cur[*step]  (p_sample's batched_times, denoising_diffusion_pytorch.py:369,419) */
int nd_sampler_begin_step(const nd_sampler_state* s, void* stream);
int nd_sampler_advance(const nd_sampler_state* s, void* stream);

/* One reverse-diffusion update on NHWC (B,H,W,C) tensors, in place on x:
 *  DDPM (p_sample :366-373 + p_mean_variance :356-364 + q_posterior :322-329),
 *  DDIM (ddim_sample :418-439, model_predictions :331-354 with clip + rederived eps).
 * objective: 0 pred_noise, 1 pred_x0, 2 pred_v.  noise: explicit draws (parity mode; the draw of
 * step i is at noise + i * noise_step_stride floats, the i-th torch.randn_like of the reference)
 * or NULL => Philox4x32-10 keyed (seed, first_sample + b, step) (throughput mode). */
int nd_sampler_step_ddpm_f32(float* x, const float* model_out, const float* noise, int64_t noise_step_stride,
                             const nd_sampler_state* s, int objective,
                             uint64_t seed, int64_t first_sample,
                             int B, int HW, int C, void* stream);
int nd_sampler_step_ddim_f32(float* x, const float* model_out, const float* noise, int64_t noise_step_stride,
                             const nd_sampler_state* s, int objective,
                             uint64_t seed, int64_t first_sample,
                             int B, int HW, int C, void* stream);
/* x_T ~ N(0,1): torch.randn(shape) (:381,:413) from the same Philox stream (step = -1). */
int nd_philox_normal_f32(float* out, uint64_t seed, int64_t first_sample, int32_t step,
                         int B, int HW, int C, void* stream);

/* ------------------------------------------------------------------ full attention (config 4) */

/* Attention.forward (:255-266) core on MFMA: out = softmax(q k^T / sqrt(dh)) v per (b, head).
 * qkv NHWC [B][N][3*heads*dh] as produced by the to_qkv 1x1 conv ('b (h c) x y' channel order,
 * q | k | v thirds); out [B][N][heads*dh].  dh must be 32. */
int nd_attention_mfma_f32(const float* qkv, int ld_qkv, float* out, int ld_out,
                          int B, int N, int heads, int dh, void* stream);
/* LinearAttention.forward (:218-235) core, O(N dh^2): q softmax over channels (x dh^-1/2), k softmax over pixels,
 * out = (k v^T)^T q per (b, head).  Same qkv / out layout as nd_attention_mfma_f32; `workspace` holds
 * nd_linear_attention_workspace_floats(B, N, heads) floats.  Defined but not wired in the reference net. */
int64_t nd_linear_attention_workspace_floats(int B, int N, int heads);
int nd_linear_attention_f32(const float* qkv, int ld_qkv, float* out, int ld_out, float* workspace,
                            int B, int N, int heads, int dh, void* stream);
/* RMSNorm.forward (:89-90) over channels: out = x / max(||x||, 1e-12) * g * sqrt(C). */
int nd_rmsnorm_nhwc_f32(const float* x, int ldx, const float* g, float* out, int ldo,
                        int B, int HW, int C, void* stream);
/* out = RMSNorm(x) * g + res: LinearAttention's closing RMSNorm (Diffusion_arch.py:213-216) with the residual of the per-stage wiring */
int nd_rmsnorm_add_nhwc_f32(const float* x, int ldx, const float* g, const float* res, int ldr, float* out, int ldo, int B, int HW, int C, void* stream);

/* ------------------------------------------------------------------ training the attention modules (forward with saved state, backward)
 * fp32, fixed summation order, no atomics: a repeated call gives the same bits and a sample's result does not depend on its batch.
 * dqkv has qkv's layout ([B][N][q | k | v thirds]): it is the gradient of to_qkv's output as it stands.  All 3 * heads * dh channels of every
 * token are written (not accumulated: no clearing needed); floats beyond them in a row of ld_dqkv are left untouched.  dh must be 32
 * (ND_E_SHAPE otherwise), any N >= 1; all strides multiples of 4 floats, pointers 16-byte aligned. */

/* nd_attention_mfma_f32 (same kernel body, `out` bit for bit the same) that also writes lse[b][h][i] = m_i + log(l_i) of the scaled scores
 * (models/attend.py:101-116), fp32 [B][heads][N]: what the backward recomputes the probabilities from. */
int nd_attention_train_forward_f32(const float* qkv, int ld_qkv, float* out, int ld_out, float* lse,
                                   int B, int N, int heads, int dh, void* stream);
/* Backward of Attention's core (Diffusion_arch.py:255-266), flash-style on the exact-fp32 matrix instruction: delta_i = sum_d dO_i O_i,
 * P = exp(S - lse) recomputed per tile (no N x N tensor), dV = P^T dO, dP = dO V^T, dS = P (.) (dP - delta), dQ = scale dS K, dK = scale dS^T Q.
 * Three launches: delta; a pass whose workgroups own key tiles (dK, dV); a pass whose workgroups own query tiles (dQ).
 * `workspace`: nd_attention_backward_workspace_floats(B, N, heads) floats.  Grid limits: B, heads <= 65535, B * N * heads < 2^38 (ND_E_SHAPE). */
int64_t nd_attention_backward_workspace_floats(int B, int N, int heads);
int nd_attention_backward_f32(const float* qkv, int ld_qkv, const float* out, int ld_out, const float* dout, int ld_dout, const float* lse,
                              float* dqkv, int ld_dqkv, float* workspace, int B, int N, int heads, int dh, void* stream);
/* Backward of LinearAttention's core (Diffusion_arch.py:218-235).  `fwd_workspace`: the workspace nd_linear_attention_f32 left for the SAME
 * qkv (the key statistics and the per-chunk context partials) -- the saved state of the forward.  With q~ = softmax_d(q), s = dh^-1/2,
 * k^ = softmax_n(k), ctx = k^ v^T:  dctx = s q~ dout^T;  dq = q~ (.) (t - sum_d q~ t), t = s ctx dout;  dv = dctx^T k^;
 * dk = k^ (.) (dctx v - r), r[d] = sum_e dctx[d][e] ctx[d][e].  Two passes over N (per-chunk partials of dctx reduced in chunk order, then
 * the three gradients per pixel), O(N dh^2).  `workspace`: nd_linear_attention_backward_workspace_floats(B, N, heads) floats. */
int64_t nd_linear_attention_backward_workspace_floats(int B, int N, int heads);
int nd_linear_attention_backward_f32(const float* qkv, int ld_qkv, const float* dout, int ld_dout, const float* fwd_workspace, float* dqkv,
                                     int ld_dqkv, float* workspace, int B, int N, int heads, int dh, void* stream);
/* Backward of RMSNorm (Diffusion_arch.py:84-90; forward nd_rmsnorm_nhwc_f32 / nd_rmsnorm_add_nhwc_f32), the norm recomputed from x:
 * dx [B][HW][C] and dg [C] (per-workgroup partials, then fp64 in a fixed order).  Where |x| < 1e-12 the clamp makes the norm a constant and
 * dx = g dy sqrt(C) / 1e-12, as autograd of F.normalize gives it (no 0/0).  The residual of the _add form receives dy itself: no kernel.
 * C % 4 == 0, C <= 1024 (nd_rmsnorm_train_takes(C): 1 / 0).  `workspace`: nd_rmsnorm_backward_workspace_floats(B * HW, C) floats. */
int nd_rmsnorm_train_takes(int C);
int64_t nd_rmsnorm_backward_workspace_floats(int64_t npix, int C);
int nd_rmsnorm_backward_f32(const float* dy, int lddy, const float* x, int ldx, const float* g, float* dx, int lddx, float* dg, float* workspace,
                            int B, int HW, int C, void* stream);

/* ------------------------------------------------------------------ optimizer step of the training path
 * torch.optim.Adam's update (the reference's optimizer: models/trainer_diffusion.py:94; L2 weight decay added to the gradient, no amsgrad)
 * for all parameters of a group in ONE launch -- PyTorch's foreach form makes ~10 passes over the parameters.  `items_dev`: n_items records
 * in DEVICE memory, one per parameter: p, m (exp_avg), v (exp_avg_sq) are updated in place from g; step_size = lr / (1 - beta1^t) and
 * bias2_sqrt = sqrt(1 - beta2^t) with the parameter's own step count t (after the increment), computed by the caller in double precision;
 * vec4 != 0 promises that the four tensors are 16-byte aligned (with vec4 == 0 every chunk, whole ones included, takes the scalar path).
 * beta1, beta2 are the DOUBLES the caller gave the optimizer: the kernels use (float)(1.0 - beta1), (float)(1.0 - beta2) and (float)beta2 --
 * the complements taken in double and rounded once, as torch.optim.Adam does; the capturable forms take pow of the doubles.  `chunks_dev`: n_chunks pairs (item index, chunk index) of int32 in device
 * memory, one per nd_adam_chunk_elements() elements of a parameter (the last chunk of a parameter may be short).  noisediff_amd.train.Adam
 * is the host side (a torch.optim.Adam subclass with the same state dict). */
typedef struct nd_adam_item {
    float*       p;
    const float* g;
    float*       m;
    float*       v;
    int64_t      n;
    float        step_size, bias2_sqrt;
    int32_t      vec4, reserved;
    float*       step;        /* capturable form only: the parameter's step counter (one float in device memory) */
} nd_adam_item;
int nd_adam_chunk_elements(void);
int nd_adam_step_f32(const nd_adam_item* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, double beta1, double beta2, float eps,
                     float weight_decay, void* stream);
/* The same with nothing computed on the host (a training step captured as one graph): item.step points at the parameter's step counter in device
 * memory (a float, as torch.optim.Adam(capturable=True) keeps it); the call adds one to every counter and derives step_size / bias2_sqrt from it
 * (item.step_size, item.bias2_sqrt are ignored).  Two launches. */
int nd_adam_step_capturable_f32(const nd_adam_item* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, float lr, double beta1, double beta2,
                                float eps, float weight_decay, void* stream);
/* The capturable form with the learning rate read from device memory: lr = (double)*lr_dev, one float (PyTorch's tensor lr, which schedulers fill in
 * place), read in the kernel -- a captured step follows a changed rate without a new capture.  A null lr_dev is ND_E_BADARG. */
int nd_adam_step_capturable_lr_f32(const nd_adam_item* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, const float* lr_dev, double beta1,
                                   double beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------ shadow-model (EMA) update of a training run (ema.hip)
 * ema_pytorch's EMA.update, the reference's self.ema.update (models/trainer_diffusion.py:63-69,191), for all tensors in one pass, decided on the
 * device: no host read, so a captured training step can hold it.  `items_dev`: n_items records in DEVICE memory, one per (shadow, online) tensor
 * pair; vec4 != 0 promises that both are 16-byte aligned; no_ema != 0: the pair is copied where the others are averaged.  `chunks_dev`: n_chunks
 * pairs (item index, chunk index) of int32, one per nd_ema_chunk_elements elements of a tensor (the last chunk of a tensor may be short).
 * State in device memory: `step_dev` one int64, `initted_dev` one byte (a torch.bool), `plan_dev` 8 bytes owned by the caller, written by every
 * call: {int32 action; float weight}, action 0 skip, 1 copy, 2 lerp, 3 copy then lerp.  With s = *step_dev before the call (it is s + 1 after, in
 * every case):
 *   s % update_every != 0        skip: no tensor is touched;
 *   s <= update_after_step       copy: ema = src for every item;
 *   *initted_dev == 0            copy, *initted_dev = 1, then the lerp below (a no-op in value);
 *   otherwise                    lerp with weight = 1 - decay, e = s + 1 - update_after_step - 1,
 *                                decay = e <= 0 ? 0 : clamp(1 - (1 + e / inv_gamma)^-power, min_value, beta), in fp64, weight rounded to fp32 once;
 *                                per element, no contraction: w < 0.5 ? ema + w (src - ema) : src - (src - ema)(1 - w)   (torch.lerp's form).
 * Two launches (plan, apply); no reductions, no atomics: bitwise repeatable.  Null tables or state pointers, counts <= 0, beta outside [0, 1],
 * update_every < 1 or inv_gamma <= 0 return ND_E_BADARG and launch nothing.  noisediff_amd.train.EMA is the host side. */
typedef struct nd_ema_item {
    float*       ema;
    const float* src;
    int64_t      n;
    int32_t      vec4, no_ema;
} nd_ema_item;
int nd_ema_chunk_elements(void);
int nd_ema_update_f32(const nd_ema_item* items_dev, int n_items, const int32_t* chunks_dev, int n_chunks, int64_t* step_dev, uint8_t* initted_dev,
                      void* plan_dev, double beta, int64_t update_after_step, int64_t update_every, double inv_gamma, double power, double min_value,
                      void* stream);

/* ------------------------------------------------------------------ the two ends of a diffusion training step (diffusion_train.hip)
 * GaussianDiffusion.forward / p_losses (models/denoising_diffusion_pytorch.py:481-542) around the network: timestep, noising and target in
 * one launch; the weighted loss in two; its gradient in one.  All entries launch on the caller's stream and can be captured.
 *
 * Random numbers: Philox4x32-10, key = the 64-bit seed, counter = {index, global sample = first_sample + b, draw, block}.
 *   block 1 element noise: index = quad q of the sample's elements in NHWC order, four normals for four consecutive NHWC elements;
 *   block 2 offset noise: index = c >> 2, component c & 3, one normal per (sample, channel);
 *   block 3 timestep: index 0, word 0 = w, t = (uint64(w) * T) >> 32 -- a timestep's probability is off 1 / T by less than 2^-32, a relative
 *   bias below T / 2^32.  Block 0 is the sampler's, so sampling and training under one seed share no stream.  A sample's draws depend on
 *   (seed, global sample index, draw) only: not on the batch size, its row, or the rank that holds it.
 *
 * nd_diffusion_noising_f32.  x0 fp32 (B, C, H, W): NCHW-contiguous (x0_channels_last = 0) or NHWC memory (1); C % 4 == 0.  noise (NHWC memory,
 * x0's shape), offset [B][C] and t_in [B]: explicit values, or NULL to draw them; a t_in outside [0, T) is clamped (it lives in device memory).
 * Outputs: t_out [B] always; x_t and target in NHWC memory; noise_out (NHWC, the element noise before the offset is added) and offset_out
 * [B][C] when not NULL.  Per element, every operation rounded on its own, in the reference's order (:474-479, :490-492, :310-314, :539):
 *   x = 2 x0 - 1 (auto_normalize);  n = noise + offset_strength * offset (offset_strength > 0);  x_t = a x + b n,  a = sqrt_alphas_cumprod[t],
 *   b = sqrt_one_minus_alphas_cumprod[t];  target = n (objective 0), x (1), a n - b x (2).
 * With explicit noise, offset and t_in the outputs equal the reference's bit for bit.  rng ({seed, first_sample, draw} as three int64 in device
 * memory, or NULL) overrides the three scalars as nd_sampler_state.rng does: a captured graph draws anew on every replay once
 * nd_diffusion_train_advance (draw += 1, one thread) follows it.  All float pointers 16-byte aligned (ND_E_ALIGN), C % 4 != 0: ND_E_SHAPE. */
typedef struct nd_diffusion_noising {
    const float* x0;
    const float* noise;                             /* or NULL: drawn */
    const float* offset;                            /* or NULL: drawn when offset_strength > 0 or offset_out is set */
    const int64_t* t_in;                            /* or NULL: drawn */
    const float* sqrt_alphas_cumprod;               /* [T] */
    const float* sqrt_one_minus_alphas_cumprod;     /* [T] */
    const int64_t* rng;                             /* or NULL */
    int64_t* t_out;
    float* x_t;
    float* target;
    float* noise_out;                               /* or NULL */
    float* offset_out;                              /* or NULL */
    uint64_t seed;
    int64_t first_sample;
    int64_t draw;                                   /* the low 32 bits are the counter word */
    float offset_strength;
    int32_t B, C, H, W, T;
    int32_t objective, auto_normalize, x0_channels_last;
} nd_diffusion_noising;
int nd_diffusion_noising_f32(const nd_diffusion_noising* p, void* stream);
int nd_diffusion_train_advance(int64_t* rng, void* stream);
/* loss = mean_b( mean_elems((model_out - target)^2) * loss_weight[t_b] )  [+ mean_{b,c} |mean_hw(model_out) - mean_hw(target)| with x0_term,
 * :524-528] on NHWC tensors [B][HW][C].  Differences and squares in fp32, every sum in fp64 in a fixed order: a sample is cut into slices of
 * nd_diffusion_loss_slice_elements() elements, one workgroup each, whose partials go to `workspace`
 * (nd_diffusion_loss_workspace_bytes(B, C, HW) bytes, 16-byte aligned); a second launch of one workgroup adds a sample's slices in slice order
 * and the samples in a fixed tree.  TWO launches, no atomics and no arrival counter.  sample_loss [B] (optional) = mean_elems * loss_weight[t_b]:
 * its bits depend on neither the batch size nor the sample's row.  t outside [0, T) is clamped.  x0_term needs C a power of two <= 256 (ND_E_SHAPE)
 * and leaves the signs of the mean differences in the workspace, which nd_diffusion_loss_backward_f32 reads.  B <= 65535. */
int nd_diffusion_loss_slice_elements(void);
int64_t nd_diffusion_loss_workspace_bytes(int B, int C, int HW);
int nd_diffusion_loss_f32(const float* model_out, const float* target, const int64_t* t, const float* loss_weight, int B, int C, int HW, int T,
                          int x0_term, void* workspace, float* loss, float* sample_loss, void* stream);
/* grad_out = g * ( 2 loss_weight[t_b] / (B C HW) * (model_out - target) [+ sign_{b,c} / (B C HW)] ), one pass, formed in fp64 and rounded once.
 * g: the upstream gradient, one float in DEVICE memory (no host read).  workspace: the forward's (needed with x0_term only).  No gradient for target. */
int nd_diffusion_loss_backward_f32(const float* model_out, const float* target, const int64_t* t, const float* loss_weight, const float* g,
                                   const void* workspace, float* grad_out, int B, int C, int HW, int T, int x0_term, void* stream);

/* ------------------------------------------------------------------ the end of a denoiser training step (denoise_loss.hip)
 * models/trainer_denoising.py:66-76, 225-235: loss = mse_loss(out, target) * lambda_mse + l1_loss(out, target) * lambda_l1.
 * `out`: the network output, [B][C][HW] (ND_LAYOUT_NCHW, 1 <= C <= 16) or [B][HW][C] (ND_LAYOUT_NHWC, C = 4 only: LSID's head as it leaves the
 * 1x1 convolution); `target`: always [B][C][HW].  Anything else: ND_E_SHAPE.  d = fl(out - target) in fp32; |d| and d * d are formed and summed in
 * fp64 in an order defined over pixels and channels, not over memory: a sample's HW pixels are cut into slices of
 * nd_denoise_loss_slice_pixels() pixels, one workgroup each, whose two partials go to `workspace`
 * (nd_denoise_loss_workspace_bytes(B, C, HW) bytes, 16-byte aligned); a second launch of one workgroup adds a sample's slices in slice order and
 * the samples in a fixed tree.  TWO launches, no atomics.  Every output has the same bits for either layout of `out`, and a sample's terms depend on
 * neither the batch size nor the sample's row.
 *   terms [3]             = { (float)(lambda_mse S2 / N + lambda_l1 S1 / N), (float)(S1 / N), (float)(S2 / N) },  S1 = sum |d|, S2 = sum d^2, N = B C HW
 *   sample_terms [B][2]   = { (float)(S1_b / (C HW)), (float)(S2_b / (C HW)) }   (optional)
 * A negative or non-finite lambda, or both zero: ND_E_BADARG.  out, target, workspace (and grad below) 16-byte aligned: ND_E_ALIGN.  B <= 65535. */
enum nd_layout { ND_LAYOUT_NCHW = 0, ND_LAYOUT_NHWC = 1 };
int nd_denoise_loss_slice_pixels(void);
int64_t nd_denoise_loss_workspace_bytes(int B, int C, int HW);
int nd_denoise_loss_f32(const float* out, int out_layout, const float* target, int B, int C, int HW, double lambda_l1, double lambda_mse,
                        void* workspace, float* terms, float* sample_terms, void* stream);
/* grad = (float)(g lambda_l1 / N * sign(d) + g 2 lambda_mse / N * d), formed in fp64 and rounded once, sign(0) = 0; written in `out`'s layout, one
 * pass.  g: the upstream gradient, one float in DEVICE memory (no host read).  With lambda_mse = 0 every element is (float)(g / N) * sign(d)
 * exactly.  No gradient for target. */
int nd_denoise_loss_backward_f32(const float* out, int out_layout, const float* target, const float* g, float* grad, int B, int C, int HW,
                                 double lambda_l1, double lambda_mse, void* stream);

/* ------------------------------------------------------------------ HIP graph helpers */
int nd_stream_create(void** stream);
int nd_stream_destroy(void* stream);
int nd_stream_sync(void* stream);
int nd_graph_begin(void* stream);                 /* hipStreamBeginCapture (thread-local mode) */
int nd_graph_end(void* stream, void** graph_exec);
int nd_graph_launch(void* graph_exec, void* stream);
int nd_graph_destroy(void* graph_exec);
/* nd_graph_begin / _end / _launch make the STREAM's device current for the call (and restore the caller's): one host thread may drive the
 * step graphs of several GPUs round-robin -- GaussianDiffusion.sample under nn.DataParallel(device_ids=[...]), models/modules.py:73-83.
 * nd_stream_device: the device ordinal a stream was created on (-1: unknown). */
int nd_stream_device(void* stream);
/* timing on the library's own stream: HIP events are only meaningful on the stream they are
 * recorded on (torch.cuda.Event sees torch's current stream only). */
int nd_event_create(void** ev);
int nd_event_record(void* ev, void* stream);
int nd_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises `stop` */
int nd_event_destroy(void* ev);
/* cross-stream dependencies (the fork / join edges of the two-branch step graph: the shot-noise branch of NoiseDiffNet.forward,
 * Diffusion_arch.py:598-604, is independent of the U-Net until the final add :644): an event without timing, and "stream waits for event".
 * Recorded / waited on capturing streams they become edges of the captured graph. */
int nd_event_create_untimed(void** ev);
int nd_stream_wait_event(void* stream, void* ev);

#ifdef __cplusplus
}
#endif
#endif /* NOISEDIFF_HIP_H */
