"""References and checkers for the 3x3 convolution kernels (conv3x3.hip, conv3x3_wino.hip, conv3x3_wino2.hip, conv3x3_wino4.hip): plain torch on the CPU.

``ref64``            the operator in float64: prologue, nn.Conv2d(3, padding=1) (zero padding AFTER the activation), bias.
``ref32_direct``     the same in fp32 as ONE sequential chain per output, in the direct kernel's order (conv3x3.hip: 32-channel chunks, nine taps per chunk, groups of
                     eight channels per tap, lane half h supplying channel 4 h + s at k-step s).  Not F.conv2d: torch's blocked summation is more accurate than any
                     MFMA chain and a bound taken from it would reject a correct kernel.
``ref32_winograd``   the fp32 Winograd formula F(m x m, 3 x 3), m = 2 / 4, with the matrices of the kernels' header comments: U = G g G^T, V = B^T d B, their product
                     summed over the channels as a chain, Y = A^T M A.  ``ranges`` cuts the channels as the split-K entries do (Y per range, added in range order).
``slot_stats``       per (sample, slot, channel) sum, M2 about the slot's mean and pixel count, two-pass, in the dtype of the tensor it is given.
``check_conv`` / ``check_stats``  pure functions of host tensors; every bound is ``util.derived`` on one of the fp32 references above, every guard element must still be NaN.

Tensors are NCHW going into the references (as nn.Conv2d takes them) and NHWC coming out (as the kernels write them).  ``inputs`` / ``references`` build and cache
the operands and references of a (case, prologue) pair so that the CPU and the GPU test files share them and compute each once.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from noisediff_amd import synth
from util import derived

F32, F64 = torch.float32, torch.float64

# (B, H, W, cin, cout): the smallest shapes that reach each code path (tests/test_conv3x3_float64.py runs every entry point on every case it accepts)
CASES = {
    "tiny": (2, 4, 4, 32, 20),               # image smaller than any tile; W < 16: the direct kernel's 8-wide tilings
    "one_over": (2, 17, 33, 24, 68),         # one pixel over a 4x4 tile, a 16-row tile and a 32-column region; cin = 16 + 8; one channel quad over a 64-cout tile
    "ragged": (2, 19, 37, 40, 20),           # cin = 32 + 8 (F(2x2): 32-channel chunks) = 2 x 16 + 8 (F(4x4)); cout = one wave's 16 + a quad of the next
    "second_trip": (3, 90, 150, 32, 180),    # 270 items of the 16 x 32 form, 540 of the 16 x 16 forms, ragged in y, x and cout: the persistent loops take a second trip
    "deep": (1, 16, 16, 512, 64),            # one region, 32 K chunks of F(4x4): the weight ring and the staging tables wrap many times
    "all_bias": (1, 16, 32, 32, 2048),       # F(4x4)'s MAX_COUT: the whole LDS bias vector
    "offset": (2, 19, 37, 40, 20),           # `ragged` with w ~ U(-0.05, 0.05), bias ~ 30 + U(-1, 1): output mean / std ~ 100, the conditioning case of the statistics
}
UPSAMPLE_TWIN = {"one_over": (2, 18, 34, 24, 68), "ragged": (2, 20, 36, 40, 20), "deep": (1, 16, 16, 512, 64)}   # even-sized twins for nearest-x2 addressing
PROLOGUES = ("none", "affine", "map", "map_blocked", "genmap", "leaky", "leaky_second", "concat", "upsample")

# Lavin & Gray; m = 4 as in conv3x3_wino4.hip's header comment, m = 2 as csrc/wino2x2.h's bt_* / at_coef
WINO = {
    4: ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
        [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
        [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
    2: ([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
        [[1, 1, 1, 0], [0, 1, -1, -1]]),
}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- operands

def inputs(case, pro="none", c0=0, shape=None):
    """The operands of one (case, prologue): a dict of fp32 CPU tensors.  ``c0`` = channels of the first source of a virtual concat (concat / leaky_second).
    M, A, D are drawn so that silu(D - M A) is far from 0: the border then tells padding before the activation from padding after it."""
    B, H, W, cin, cout = shape or (UPSAMPLE_TWIN[case] if pro == "upsample" else CASES[case])
    u = lambda name, shp, lo, hi: synth.uniform(23, f"c3.{case}.{name}", shp, lo, hi)
    hs, ws = (H // 2, W // 2) if pro == "upsample" else (H, W)
    x = u("x", (B, cin, hs, ws), -1.5, 1.5)
    inp = {"case": case, "pro": pro, "shape": (B, H, W, cin, cout), "c0": c0}
    if case == "offset":
        inp["w"], inp["b"] = u("w", (cout, cin, 3, 3), -0.05, 0.05), 30.0 + u("b", (cout,), -1.0, 1.0)
    else:
        inp["w"], inp["b"] = u("w", (cout, cin, 3, 3), -0.2, 0.2), u("b", (cout,), -1.0, 1.0)
    if pro in ("concat", "leaky_second"):
        assert 0 < c0 < cin
        inp["x"], inp["x2"] = x[:, :c0].contiguous(), x[:, c0:].contiguous()
    else:
        inp["x"] = x
    if pro in ("affine", "map", "map_blocked", "genmap"):
        inp["M"], inp["A"], inp["D"] = u("M", (B, cin), 0.5, 1.0), u("A", (B, cin), 0.5, 1.5), u("D", (B, cin), -1.0, -0.5)
    if pro in ("map", "map_blocked"):
        inp["sc"], inp["sh"] = u("sc", (B, cin, H, W), -0.5, 0.5), u("sh", (B, cin, H, W), -0.5, 0.5)
    if pro == "genmap":      # silu(pos_emb) [8 channels], mlp[1].weight [2 cin][8], mlp[1].bias [2 cin]
        inp["pe"], inp["gw"], inp["gb"] = u("pe", (B, 8, H, W), -2.0, 2.0), u("gw", (2 * cin, 8), -0.4, 0.4), u("gb", (2 * cin,), -0.3, 0.3)
    return inp


def activated(inp, dtype, pad_first=False):
    """The tensor the convolution sees, NCHW in ``dtype``, every step in that dtype.  ``pad_first`` (mutation tests only) returns it zero-padded by one pixel BEFORE the
    activation -- the wrong order."""
    pro = inp["pro"]
    x = inp["x"].to(dtype)
    if pad_first:
        x = F.pad(x, (1, 1, 1, 1))
    bc = lambda t: t.to(dtype)[:, :, None, None]
    if pro in ("affine", "map", "map_blocked", "genmap"):
        y = (x - bc(inp["M"])) * bc(inp["A"]) + bc(inp["D"])
        if pro in ("map", "map_blocked"):
            sc, sh = inp["sc"].to(dtype), inp["sh"].to(dtype)
        elif pro == "genmap":
            ss = F.conv2d(inp["pe"].to(dtype), inp["gw"].to(dtype)[:, :, None, None], inp["gb"].to(dtype))
            sc, sh = ss[:, : x.shape[1]], ss[:, x.shape[1]:]
        if pro != "affine":
            assert not pad_first
            y = y * (sc + 1.0) + sh
        return F.silu(y)
    if pro == "leaky":
        return F.leaky_relu(x, 0.2)
    if pro == "leaky_second":
        return torch.cat((x, F.leaky_relu(inp["x2"].to(dtype), 0.2)), 1)
    if pro == "concat":
        return torch.cat((x, inp["x2"].to(dtype)), 1)
    if pro == "upsample":
        return F.interpolate(x, scale_factor=2, mode="nearest")
    return x


class _chain_threads:
    """A chain is thousands of small element-wise steps: below a million elements a thread team costs more per step than it saves."""

    def __init__(self, t):
        self.n = 1 if t.numel() < (1 << 20) else None

    def __enter__(self):
        self.old = torch.get_num_threads()
        if self.n:
            torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        torch.set_num_threads(self.old)


def ref64(inp):
    """float64: prologue, F.conv2d(padding=1), bias.  NHWC."""
    return (F.conv2d(activated(inp, F64), inp["w"].double(), None, padding=1) + inp["b"].double()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()


def conv2d32(inp):
    """torch's own fp32 convolution: an 'other legitimate evaluation' for the admit tests, never a bound."""
    return F.conv2d(activated(inp, F32), inp["w"], inp["b"], padding=1).permute(0, 2, 3, 1).contiguous()


def ref32_direct(inp, taps_outer=False):
    """fp32, one sequential multiply-add chain per output in conv3x3.hip's order: `for cb in 0, 32, ..` (conv3x3_kernel's chunk loop), nine taps per chunk and
    groups of eight channels per tap (conv_chunk), k-steps s = 0..3 with lane half h supplying channel 4 h + s (header comment) -- the two halves of a
    v_mfma_f32_32x32x2_f32 in order.  ``taps_outer``: the taps outside the chunks, another legitimate chain (admit tests)."""
    B, H, W, cin, cout = inp["shape"]
    xp = F.pad(activated(inp, F32), (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    wt = inp["w"].permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous()
    acc = torch.zeros(B, H, W, cout)
    steps = [(cb, tap) for tap in range(9) for cb in range(0, cin, 32)] if taps_outer else [(cb, tap) for cb in range(0, cin, 32) for tap in range(9)]
    with _chain_threads(acc):
        for cb, tap in steps:
            xs = xp[:, tap // 3: tap // 3 + H, tap % 3: tap % 3 + W]
            for g0 in range(cb, min(cb + 32, cin), 8):
                for s in range(4):
                    for h in (0, 1):
                        c = g0 + 4 * h + s
                        acc.addcmul_(xs[..., c: c + 1], wt[tap, c])
    return acc + inp["b"]


def ref32_winograd(m, inp, dtype=F32, cols_first=False, u_from64=False, ranges=None):
    """Winograd F(m x m, 3 x 3) in ``dtype``: U = G g G^T, V = B^T d B (rows, then columns; ``cols_first`` the other way), M = the chain over the channels of V U,
    Y = A^T M A, + bias.  ``u_from64``: U formed in float64 and rounded once, as the packers do.  ``ranges``: [(lo, hi), ..] channel ranges, Y per range added in order
    (split-K: the partial tensors, then w4_splitk_reduce_kernel).  NHWC."""
    BT, G, AT = (torch.tensor(t, dtype=dtype) for t in WINO[m])
    B, H, W, cin, cout = inp["shape"]
    a, ty, tx = m + 2, cdiv(H, m), cdiv(W, m)
    xp = F.pad(activated(inp, dtype), (1, tx * m + 1 - W, 1, ty * m + 1 - H))
    d = xp.unfold(2, a, m).unfold(3, a, m)                                   # [B][C][ty][tx][a][a]
    if cols_first:
        V = torch.einsum("ip,bcyxpq->bcyxiq", BT, torch.einsum("bcyxpq,jq->bcyxpj", d, BT))
    else:
        V = torch.einsum("bcyxiq,jq->bcyxij", torch.einsum("ip,bcyxpq->bcyxiq", BT, d), BT)
    if u_from64:
        G6 = torch.tensor(WINO[m][1], dtype=F64)
        U = torch.einsum("ip,ocpq,jq->ocij", G6, inp["w"].double(), G6).to(dtype)
    else:
        U = torch.einsum("ocip,jp->ocij", torch.einsum("ip,ocpq->ociq", G, inp["w"].to(dtype)), G)
    N = B * ty * tx
    V = V.permute(1, 0, 2, 3, 4, 5).reshape(cin, N, a * a, 1).contiguous()
    U = U.permute(1, 2, 3, 0).reshape(cin, a * a, cout).contiguous()
    total = None
    for lo, hi in ranges or [(0, cin)]:
        M = torch.zeros(N, a * a, cout, dtype=dtype)
        with _chain_threads(M):
            for c in range(lo, hi):
                M.addcmul_(V[c], U[c])
        M = M.reshape(N, a, a, cout)
        if cols_first:
            Y = torch.einsum("ip,npjo->nijo", AT, torch.einsum("npqo,jq->npjo", M, AT))
        else:
            Y = torch.einsum("niqo,jq->nijo", torch.einsum("ip,npqo->niqo", AT, M), AT)
        total = Y if total is None else total + Y
    out = total.reshape(B, ty, tx, m, m, cout).permute(0, 1, 3, 2, 4, 5).reshape(B, ty * m, tx * m, cout)[:, :H, :W]
    return (out + inp["b"].to(dtype)).contiguous()


@functools.lru_cache(maxsize=32)
def _references(case, pro, c0, kind, ranges, shape):
    inp = inputs(case, pro, c0, shape)
    r32 = ref32_direct(inp) if kind == "direct" else ref32_winograd(int(kind), inp, ranges=list(ranges) if ranges else None)
    return inp, ref64(inp), r32


def references(case, pro, kind, c0=0, ranges=None, shape=None):
    """(operands, ref64, ref32) of a (case, prologue) for ``kind`` = "direct", 2 or 4.  Cached: computed once, shared, never modified by a caller."""
    return _references(case, pro, c0, str(kind), tuple(ranges) if ranges else None, shape)


# ---------------------------------------------------------------------------------------------------------------- F(4x4) packed weights

def wino4_U(g, dtype):
    """U = G g G^T of an OIHW operator ``g`` [cout][cin][3][3] in ``dtype`` -> [cout][cin][6][6].  float64: G's rationals 1/4, +-1/6, 1/24, +-1/12, 1 as float64
    literals (exact to 2^-53); fp32: G rounded to fp32, G g first, then G^T -- ref32_winograd's order."""
    G = torch.tensor(WINO[4][1], dtype=dtype)
    return torch.einsum("ocip,jp->ocij", torch.einsum("ip,ocpq->ociq", G, g.to(dtype)), G)


def _wino4_blocks(cin, cout):
    return 2 * cdiv(cdiv(cin, 8), 2), 4 * cdiv(cout, 64)              # whole 16-channel chunks of cin, whole 64-channel tiles of cout in groups of 16


def wino4_pack_layout(U, cin, cout):
    """``U`` [cout][cin][6][6] -> the flat buffer nd_pack_conv3x3_wino4_weight documents: blocks [cin / 8][coutP / 16][18 position pairs][64 lanes][4], lane
    (cout = l & 15, k = l >> 4) holding {U[2pp][ch 2k], U[2pp][ch 2k + 1], U[2pp + 1][ch 2k], U[2pp + 1][ch 2k + 1]} of its block, position = 6 xi + nu;
    padded channels zero."""
    n_c8, n_cg = _wino4_blocks(cin, cout)
    full = U.new_zeros(n_cg * 16, n_c8 * 8, 36)
    full[:cout, :cin] = U.reshape(cout, cin, 36)
    # [cg][col][c8][k][c][pp][ph] -> [c8][cg][pp][k][col][ph][c]
    return full.reshape(n_cg, 16, n_c8, 4, 2, 18, 2).permute(2, 0, 5, 3, 1, 6, 4).reshape(-1).contiguous()


def wino4_unpack(packed, cin, cout):
    """The inverse of ``wino4_pack_layout``: (U [cout][cin][6][6], the entries of the padded channels as one flat tensor)."""
    n_c8, n_cg = _wino4_blocks(cin, cout)
    assert packed.numel() == n_c8 * n_cg * 18 * 256
    full = packed.reshape(n_c8, n_cg, 18, 4, 16, 2, 2).permute(1, 4, 0, 3, 6, 2, 5).reshape(n_cg * 16, n_c8 * 8, 36)
    real = torch.zeros(n_cg * 16, n_c8 * 8, dtype=torch.bool)
    real[:cout, :cin] = True
    return full[:cout, :cin].reshape(cout, cin, 6, 6).contiguous(), full[~real].reshape(-1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- statistics

def _tiles(out, th, tw):
    """[B][ty][th][tx][tw][C] view of an NHWC tensor padded with zeros to whole tiles, and the inside-the-image mask [ty][th][tx][tw]."""
    B, H, W, C = out.shape
    ty, tx = cdiv(H, th), cdiv(W, tw)
    inside = F.pad(out.new_ones(H, W), (0, tx * tw - W, 0, ty * th - H)).reshape(ty, th, tx, tw)
    return F.pad(out, (0, 0, 0, tx * tw - W, 0, ty * th - H)).reshape(B, ty, th, tx, tw, C), inside


def slot_stats(out, tile=16):
    """Per (sample, slot, channel) {sum, M2 about the slot's mean} and per slot the pixel count of an NHWC tensor, two-pass in ITS dtype (float64: the reference;
    fp32: the fp32 evaluation whose error sets the bound).  One slot per ``tile`` x ``tile`` pixels, indexed ty * tiles_x + tx; ``tile=None``: the whole image."""
    B, H, W, C = out.shape
    t, inside = _tiles(out, *((H, W) if tile is None else (tile, tile)))
    ty, tx = inside.shape[0], inside.shape[2]
    cnt = inside.sum((1, 3)).reshape(ty * tx)                              # the ragged tiles: zeros join the sums, never the counts
    s = t.sum((2, 4))
    dv = (t - (s / cnt.reshape(1, ty, tx, 1))[:, :, None, :, None]) * inside[None, :, :, :, :, None]
    return s.reshape(B, ty * tx, C), (dv * dv).sum((2, 4)).reshape(B, ty * tx, C), cnt.double()


def slot_stats_pivoted(out, th, tw):
    """The same partials in the ONE-PASS order of the Winograd kernels' epilogues, in the dtype of ``out``: about a pivot p = the slot's first pixel,
    S = sum (v - p), Q = sum (v - p)^2, sum = S + n p, M2 = Q - S^2 / n -- conv3x3_wino4.hip's epilogue ("one pivot per cout for the whole 16x16 tile: its first
    pixel", "sum = S + n p, M2 = Q - S^2 / n") and w4_splitk_reduce_stats_kernel with 16 x 16 slots, conv3x3_wino2.hip's ("shifted sums: sum = S + cnt*p,
    M2 = Q - S^2/cnt", pivot = Y0[0] of the wave's 8 x 16 half tile).  A legitimate order whose conditioning depends on how far the first pixel is from the
    slot's mean; the direct kernel and conv3x3_wino.hip take M2 two-pass in registers (``slot_stats``)."""
    B, H, W, C = out.shape
    t, inside = _tiles(out, th, tw)
    ty, tx = inside.shape[0], inside.shape[2]
    cnt = inside.sum((1, 3)).reshape(1, ty, tx, 1)
    p = t[:, :, 0, :, 0]                                                   # [B][ty][tx][C]
    dv = ((t - p[:, :, None, :, None]) * inside[None, :, :, :, :, None]).permute(0, 1, 3, 5, 2, 4).reshape(B, ty, tx, C, th * tw // 32, 32)
    # a lane's shifted sums are chains, not torch's blocked sums: 32 values per chain (wino2: f32x2 halves of a lane's 64 pixels, `sS2 += dv`; wino4: `sum2 += dv` over
    # the lane's 4 x 16 pixels), the chains then added (`sS2[0] + sS2[1]`, __shfl_xor)
    S, Q = dv.new_zeros(B, ty, tx, C, th * tw // 32), dv.new_zeros(B, ty, tx, C, th * tw // 32)
    for k in range(32):
        S += dv[..., k]
        Q.addcmul_(dv[..., k], dv[..., k])
    S, Q = S.sum(-1), Q.sum(-1)
    return (S + cnt * p).reshape(B, ty * tx, C), (Q - S * S / cnt).clamp(min=0).reshape(B, ty * tx, C), cnt.reshape(ty * tx).double()


def slot_stats64(out64, tile=16):
    assert out64.dtype == F64
    return slot_stats(out64, tile)


def merge_slots64(st, cnt):
    """Pools partials {sum, M2} [B][slots][C][2] with counts [slots] over the slots, in float64, with the exact pairwise formula:
    M2 = sum_i M2_i + sum_i n_i (mean_i - mean)^2.  -> sum [B][C], M2 [B][C], n."""
    st, n = st.double(), cnt.double()
    live = (n > 0)[None, :, None]                    # a slot behind no pixel holds nothing: nd_groupnorm_finalize_f32 skips it (norm.hip, `ok = ni[u] > 0.0f`)
    zero = torch.zeros((), dtype=F64)
    s_i, m_i = torch.where(live, st[..., 0], zero), torch.where(live, st[..., 1], zero)
    tot, N = s_i.sum(1), n.sum()
    m2 = m_i.sum(1) + (n[None, :, None] * (s_i / n.clamp(min=1)[None, :, None] - (tot / N)[:, None]) ** 2 * live).sum(1)
    return tot, m2, N


# ---------------------------------------------------------------------------------------------------------------- checkers

def only_nan_outside(buffer, region, what):
    """Every element of ``buffer`` outside ``region`` (a tuple of slices) is still NaN."""
    g = buffer.clone()
    g[region] = float("nan")
    bad = int((~torch.isnan(g)).sum())
    assert bad == 0, f"{what}: {bad} guard elements were written (the first at flat index {int((~torch.isnan(g)).reshape(-1).nonzero()[0])})"


def check_conv(got, out_buffer, r64, r32, what=""):
    """``got``: the [B][H][W][cout] region of the host copy ``out_buffer`` [1 + B H + 1][W][ldo] of the output allocation (one guard image row in front and behind,
    ldo - cout guard columns).  Bound: util.derived against ``r64`` with the fp32 reference ``r32``; the region finite; every guard element still NaN."""
    B, H, W, cout = got.shape
    assert out_buffer.shape[0] == B * H + 2 and out_buffer.shape[1] == W
    only_nan_outside(out_buffer, (slice(1, -1), slice(None), slice(0, cout)), what + " output")
    return derived(got, r64, r32, what)


def check_stats(st, sc, st_buffer, sc_buffer, guard, r64, r32, per_slot, what="", pivot=None):
    """``st`` [B][slots][cout][2] and ``sc`` [slots] as the kernel left them, inside the flat host copies ``st_buffer`` / ``sc_buffer`` with ``guard`` NaN floats in front and
    behind.  ``per_slot`` (F(4x4) forms: one slot per 16 x 16 tile, ty * tiles_x + tx): sum, M2 and count slot by slot; otherwise the slots' pixel sets are not part
    of the interface: the partials are pooled in float64 (merge_slots64) and compared over the whole image, the counts must be whole numbers >= 0 that add up to H W.
    Sum, M2 and count each go through util.derived with their own fp32 reference: the fp32 two-pass sum and M2 of the fp32 reference output ``r32`` -- or, for the
    kernels whose epilogue takes them one-pass about a pivot, ``pivot`` = their slot (rows, columns): the fp32 partials of ``slot_stats_pivoted`` (pooled in float64
    like the kernel's own where the slots are pooled).  Slots behind no pixel are not looked at: their consumer skips them."""
    B, H, W, cout = r64.shape
    for buf, n, name in ((st_buffer, st.numel(), "statistics"), (sc_buffer, sc.numel(), "slot_count")):
        assert buf.numel() == n + 2 * guard
        only_nan_outside(buf, (slice(guard, guard + n),), f"{what} {name}")
    assert torch.isfinite(sc).all() and torch.isfinite(st[:, sc > 0]).all(), f"{what}: non-finite statistics"
    tile = 16 if per_slot else None
    s64, m64, n64 = slot_stats(r64, tile)
    if pivot is None:
        s32, m32, _ = slot_stats(r32, tile)
    else:
        s32, m32, n32 = slot_stats_pivoted(r32, *pivot)
        if not per_slot:
            s32, m32, _ = merge_slots64(torch.stack((s32, m32), -1), n32)
    if per_slot:
        assert st.shape[1] == s64.shape[1], f"{what}: {st.shape[1]} slots for {s64.shape[1]} tiles"
        assert torch.equal(sc.double(), n64), f"{what}: slot_count {sc.tolist()} != {n64.tolist()}"
        gs, gm, gn = st[..., 0], st[..., 1], sc
    else:
        assert bool((sc >= 0).all()) and torch.equal(sc, sc.round()) and float(sc.double().sum()) == H * W, f"{what}: slot_count {sc.tolist()} does not partition {H} x {W} pixels"
        gs, gm, gn = merge_slots64(st, sc)
        gn = gn.reshape(1)
    derived(gs, s64, s32, what + " sum")
    derived(gm, m64, m32, what + " M2")
    derived(gn, n64, n64.float(), what + " count")
    return True
