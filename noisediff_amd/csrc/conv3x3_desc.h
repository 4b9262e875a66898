// What each conv3x3 forward kernel takes, stated once (host code only; no HIP call).  Every entry checks its descriptor in two parts.  The SHAPE part reads no
// pointer: B, H, W, cin, cout, ldo, of the source c0, c1, ld0, ld1, mode, upsample, unshuffle, map_blocked, for split-K `splits`.  It lives here, one function per
// kernel, and is the only place a kernel's limit is written: the entry runs it with its name prefix (refusal: message + code), nd_conv3x3_takes with `who` ==
// nullptr (a question: the code alone, nd_last_error untouched).  The POINTER part (null, alignment, p1 with c1, mad / map / gamma / beta present, stats with
// slot_count) stays with the entry.  So do the "grid too large" guards of the launch arithmetic: no tensor that fits a device's memory reaches them.
#pragma once
#include "nd_common.h"

constexpr int ND_W4_CHUNK = 16;          // F(4x4): channels per K chunk
constexpr int ND_W4_MAX_COUT = 2048;     // F(4x4): the whole bias vector (padded to cout tiles) lives in LDS

// ---------------------------------------------------------------- common to the four entries
static inline int nd_conv3x3_common_shape(const nd_conv3x3* d, const char* who) {
    const nd_src& s = d->src;
    ND_DESC_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->cin > 0 && d->cout > 0, ND_E_BADARG, "non-positive size");
    ND_DESC_REQUIRE(s.c0 + s.c1 == d->cin && s.c0 % 4 == 0 && s.c1 % 4 == 0 && s.c0 > 0, ND_E_SHAPE, "source channels %d+%d do not match cin=%d (multiples of 4)", s.c0, s.c1, d->cin);
    ND_DESC_REQUIRE(s.ld0 >= s.c0 && s.ld0 % 4 == 0 && (s.c1 == 0 || (s.ld1 >= s.c1 && s.ld1 % 4 == 0)), ND_E_ALIGN, "pixel strides must be >= channels and multiples of 4");
    return 0;
}

static inline int nd_conv3x3_common_ptrs(const nd_conv3x3* d, const char* who) {
    const nd_src& s = d->src;
    ND_DESC_REQUIRE(s.p0 && d->weight && d->out, ND_E_BADARG, "null tensor pointer");
    ND_DESC_REQUIRE((s.c1 == 0) == (s.p1 == nullptr), ND_E_BADARG, "p1/c1 mismatch");
    return 0;
}

// ---------------------------------------------------------------- direct, F(2x2) wino and wino2
// shape part of nd_conv3x3_nhwc_f32 and nd_conv3x3_wino_nhwc_f32, and the head of wino2's
static inline int nd_conv3x3_f2_shape(const nd_conv3x3* d, const char* who) {
    const nd_src& s = d->src;
    if (int e = nd_conv3x3_common_shape(d, who)) return e;
    ND_DESC_REQUIRE(d->cin % 8 == 0, ND_E_SHAPE, "cin=%d must be a multiple of 8", d->cin);
    ND_DESC_REQUIRE(d->ldo >= d->cout, ND_E_SHAPE, "ldo < cout");
    ND_DESC_REQUIRE(s.mode == ND_PRO_NONE || s.mode == ND_PRO_AFFINE_SILU || s.mode == ND_PRO_AFFINE_MAP_SILU || s.mode == ND_PRO_LEAKY ||
                    s.mode == ND_PRO_LEAKY_SECOND, ND_E_BADARG, "unsupported prologue %d", s.mode);
    ND_DESC_REQUIRE(!s.map_blocked, ND_E_BADARG, "the blocked map layout is read by nd_conv3x3_wino4_nhwc_f32 only");
    ND_DESC_REQUIRE(!s.upsample || (d->H % 2 == 0 && d->W % 2 == 0 && s.c1 == 0), ND_E_SHAPE, "upsample needs even H, W and one source");
    ND_DESC_REQUIRE(!s.unshuffle, ND_E_BADARG, "unshuffle is a pointwise-only addressing mode");
    return 0;
}

// pointer part of the same three entries (wino2 under W2_STAMP: no statistics operands)
static inline int nd_conv3x3_f2_ptrs(const nd_conv3x3* d, const char* who, bool stats = true) {
    const nd_src& s = d->src;
    if (int e = nd_conv3x3_common_ptrs(d, who)) return e;
    ND_DESC_REQUIRE(nd_aligned16(s.p0) && nd_aligned16(s.p1) && nd_aligned16(d->weight) && nd_aligned16(s.mad) && nd_aligned16(s.map), ND_E_ALIGN, "pointers must be 16-byte aligned");
    ND_DESC_REQUIRE((s.mode != ND_PRO_AFFINE_SILU && s.mode != ND_PRO_AFFINE_MAP_SILU) || s.mad, ND_E_BADARG, "affine prologue needs mad");
    ND_DESC_REQUIRE(s.mode != ND_PRO_AFFINE_MAP_SILU || s.map, ND_E_BADARG, "map prologue needs map");
    ND_DESC_REQUIRE(!stats || (d->stats == nullptr) == (d->slot_count == nullptr), ND_E_BADARG, "stats and slot_count go together");
    return 0;
}

static inline int nd_conv3x3_wino2_shape(const nd_conv3x3* d, const char* who) {
    const nd_src& s = d->src;
    if (int e = nd_conv3x3_f2_shape(d, who)) return e;
    ND_DESC_REQUIRE(!(s.mode == ND_PRO_AFFINE_MAP_SILU && s.upsample), ND_E_BADARG, "map prologue with upsample is not supported here (use nd_conv3x3_wino_nhwc_f32)");
    ND_DESC_REQUIRE((long)d->B * d->H * d->W < (1L << 24) && (long)(7 * d->W + 7) * d->ldo < (1L << 31), ND_E_SHAPE, "more than 2^24 pixels (use nd_conv3x3_wino_nhwc_f32)");
    const long px = (long)d->B * (d->H >> (s.upsample ? 1 : 0)) * (d->W >> (s.upsample ? 1 : 0));
    const long widest = s.mode == ND_PRO_AFFINE_MAP_SILU ? 2L * (s.c0 + s.c1) : 0;
    // (sources 64 KB below 2 GiB: pixel offset + channel offset + the 2^31 of an invalid channel quad stay below 2^32)
    ND_DESC_REQUIRE(px * s.ld0 * 4 < (1L << 31) - 65536 && px * s.ld1 * 4 < (1L << 31) - 65536 && px * widest * 4 < (1L << 31), ND_E_SHAPE,
                    "a source tensor of 2 GiB or more (use nd_conv3x3_wino_nhwc_f32)");
    ND_DESC_REQUIRE(s.c1 == 0 || s.c0 % 32 == 0, ND_E_SHAPE, "first concat source has %d channels; a 32-channel K chunk must not straddle the sources (use nd_conv3x3_wino_nhwc_f32)", s.c0);
    return 0;
}

// ---------------------------------------------------------------- F(4x4): the 16 x 32-region form (ntg = 2), the 16 x 16-region form (ntg = 1), split-K of either
static const char* const ND_W4_GENMAP_NEEDS = "the in-kernel map prologue needs silu(pos_emb) (map), mlp[1].weight (gamma) and mlp[1].bias (beta), 16-byte aligned, one source of whole "
    "16-channel chunks, no upsample addressing, the 16 x 32-region form";
static const char* const ND_W4_MAP_NEEDS = "the map prologue needs a 16-byte aligned map and no upsample addressing";

// `who`: "nd_conv3x3_wino4", under which all F(4x4) entries refuse what they share; `who_form`: the entry that speaks for the own conditions of the 16 x 16-region
// form (ntg == 1) and of split-K (`split`, with `splits` K ranges)
static inline int nd_conv3x3_wino4_shape(const nd_conv3x3* d, int ntg, bool split, int splits, const char* who, const char* who_form) {
    const nd_src& s = d->src;
    if (int e = nd_conv3x3_common_shape(d, who)) return e;
    ND_DESC_REQUIRE(d->cin % 4 == 0 && d->cout % 4 == 0 && d->cin > ND_W4_CHUNK && d->cout <= ND_W4_MAX_COUT, ND_E_SHAPE,
                    "cin=%d and cout=%d must be multiples of 4, cin > 16 (at least two K chunks), cout <= %d", d->cin, d->cout, ND_W4_MAX_COUT);
    ND_DESC_REQUIRE(d->ldo >= d->cout && d->ldo % 4 == 0, ND_E_SHAPE, "ldo must be >= cout and a multiple of 4");
    const bool aff = s.mode == ND_PRO_AFFINE_SILU || s.mode == ND_PRO_AFFINE_MAP_SILU || s.mode == ND_PRO_AFFINE_GENMAP_SILU;
    ND_DESC_REQUIRE(s.mode == ND_PRO_NONE || aff || s.mode == ND_PRO_LEAKY || s.mode == ND_PRO_LEAKY_SECOND, ND_E_BADARG, "unsupported prologue %d", s.mode);
    ND_DESC_REQUIRE(s.mode != ND_PRO_AFFINE_GENMAP_SILU || (ntg == 2 && !s.upsample && !s.map_blocked && s.c1 == 0 && s.c0 % ND_W4_CHUNK == 0), ND_E_BADARG, "%s", ND_W4_GENMAP_NEEDS);
    ND_DESC_REQUIRE(s.mode != ND_PRO_AFFINE_MAP_SILU || !s.upsample, ND_E_BADARG, "%s", ND_W4_MAP_NEEDS);
    ND_DESC_REQUIRE(s.mode != ND_PRO_AFFINE_MAP_SILU || (long)(d->B * (long)d->H + 2) * d->W * 2 * (s.c0 + s.c1) * 4 < (1L << 30) - 65536, ND_E_SHAPE, "a scale / shift map of 1 GiB or more");
    ND_DESC_REQUIRE(!s.map_blocked || (s.mode == ND_PRO_AFFINE_MAP_SILU && (s.c0 + s.c1) % 16 == 0), ND_E_BADARG, "map_blocked needs the map prologue and a channel count that is a multiple of 16");
    ND_DESC_REQUIRE(!s.unshuffle, ND_E_BADARG, "no unshuffle addressing");
    ND_DESC_REQUIRE(!s.upsample || (d->H % 2 == 0 && d->W % 2 == 0 && s.c1 == 0), ND_E_SHAPE, "nearest-x2 upsample addressing needs even H, W and a single source");
    ND_DESC_REQUIRE(s.c1 == 0 || s.c0 % ND_W4_CHUNK == 0, ND_E_SHAPE, "first concat source has %d channels; a 16-channel K chunk must not straddle the sources", s.c0);
    ND_DESC_REQUIRE(d->W <= 2048 && d->H <= 32768, ND_E_SHAPE, "image wider than 2048 (16-bit border table)");
    const long px = (long)(d->B) * (d->H >> (s.upsample ? 1 : 0)) * (d->W >> (s.upsample ? 1 : 0));
    // byte offsets (region base + relative pixel x stride + the out-of-range bias 0x7FFFFFF0) stay below 2^32, pixels below 2^24
    const long ext = px + (d->W >> (s.upsample ? 1 : 0)) + 2;
    ND_DESC_REQUIRE(ext * s.ld0 * 4 < (1L << 30) - 65536 && ext * s.ld1 * 4 < (1L << 30) - 65536 && ext < (1L << 24), ND_E_SHAPE, "a source tensor of 1 GiB or 16 M pixels or more");
    ND_DESC_REQUIRE((long)d->B * d->H * d->W * d->ldo * 4 < (1L << 32) - 65536, ND_E_SHAPE, "an output tensor of 4 GiB or more");
    if (who) who = who_form;
    ND_DESC_REQUIRE((!split && ntg == 2) || s.mode == ND_PRO_NONE || s.mode == ND_PRO_AFFINE_SILU, ND_E_BADARG, "plain or GroupNorm-affine + SiLU sources (no map / LeakyReLU prologue)");
    const int n_chunks = nd_cdiv(d->cin, ND_W4_CHUNK);
    ND_DESC_REQUIRE(!split || ((splits == 2 || splits == 4 || splits == 8) && d->cin % ND_W4_CHUNK == 0 && n_chunks % splits == 0 && n_chunks / splits >= 2), ND_E_SHAPE,
                    "splits=%d must be 2, 4 or 8 and divide cin=%d into ranges of at least two whole 16-channel chunks", splits, d->cin);
    ND_DESC_REQUIRE(!split || (long)splits * d->B * d->H * d->W * d->cout * 4 < (1L << 31), ND_E_SHAPE, "partial sums of 2 GiB or more");
    return 0;
}
