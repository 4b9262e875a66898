"""The 1x1 GEMM and chain kernels (pointwise.hip, pwchain.hip) against float64 at their edge shapes: nd_pointwise_gemm_nhwc_f32 (narrow, large-tile, pipelined and
generic bodies), nd_pointwise_gemm_split_nhwc_f32, nd_pointwise_narrow_fold_nhwc_f32, nd_pointwise_chain_nhwc_f32, nd_pointwise_chain_split_nhwc_f32 and
nd_pointwise_chain_tail_split_nhwc_f32, each through its own packer, called directly through ctypes.

Every bound is util.derived on an fp32 reference of tests/pointwise_ref.py in the body's own accumulation order; no tolerance is a literal.  Every case runs twice and
must give the same bits.

Buffers (hiputil.Guarded): every image operand has a pixel stride wider than its channels -- ld0 = c0 + 8, ld1 = c1 + 16, ldo = cout + 4, ldr0 = cout + 8,
ldr1 = cout + 12, ldt = cout + 4 (cout rounded up to 4 first where it is 6 or 10: strides are multiples of 4) -- with NaN in the unused columns and a NaN block of
pixels before and after; bias, vec, M | A | D, gamma, beta, rowstats and every packed weight are flat with 64 NaN floats on each side.  After each call every guard
element of every buffer is still NaN and the written region is finite.

Each GEMM row names the body and tile it is written for, by pw_run's rules as they stand in pointwise.hip (the library has no call that reports which body ran, so
the name is the row's intent and not an assertion: nothing notices if a change to pw_run or another CU count moves a row to another body).  Shapes whose threshold depends on the CU count are computed from it.

cout % 4 != 0 (rows g_cout6, g_cout10) runs without per-sample epilogue operands only, or with vec at B = 1 (row g_cout6_vec): pw_epilogue reads vec + b cout and M | A | D + b 3 cout
as 16-byte quads, which are aligned for every sample only where cout % 4 == 0.  No caller passes that combination and no row runs it.

Out of scope, on purpose: the MB == 2 instantiations (128-pixel tiles of the generic and pipelined kernels) are reachable only through the ND_PW_MB knob, which the
library reads once per process -- no row runs them.  The pixel-shuffle scatter and the pixel-unshuffle addressing of the generic kernel have no row here; they stay
with tests/test_hip_kernels.py and the LSID tests.

Refusals are enumerated in ``REFUSALS``: each returns non-zero and leaves its message and the NaN output untouched.  A table row that refuses fails its test.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import pointwise_ref as R
from conv3x3_ref import only_nan_outside
from hiputil import Guarded, nan_like
from noisediff_amd import _lib as L
from util import derived

MODES = {"none": L.PRO_NONE, "silu": L.PRO_SILU, "leaky": L.PRO_LEAKY, "affine": L.PRO_AFFINE_SILU, "ln": L.PRO_LAYERNORM}
ACTS = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "silu": L.ACT_SILU}


@pytest.fixture(scope="module")
def ctx():
    import hiputil
    return hiputil.Ctx()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def pad_to(c, extra):
    """Columns to add to ``c`` channels: up to a multiple of 4, then ``extra`` unused ones."""
    return (-c) % 4 + extra


def img(t, extra):
    """(B, HW, C) host tensor -> Guarded with a NaN block of pixels on each side (the largest divisor of the pixel count up to 64) and ``extra`` NaN columns."""
    P, Cc = t.shape[0] * t.shape[1], t.shape[2]
    wg = max(d for d in range(1, min(P, 64) + 1) if P % d == 0)
    g = Guarded(t.reshape(1, P // wg, wg, Cc), pad_to(Cc, extra))
    g.orig = t
    return g


def flat(t):
    """A flat operand: 64 NaN floats on each side."""
    g = Guarded(t)
    g.orig = t
    return g


def intact(bufs, what):
    """Every read-only operand after a call: its guards still NaN, and its own values -- where the test holds the original -- unchanged."""
    for g in bufs:
        if getattr(g, "is_out", False):
            continue
        buf = g.host()
        only_nan_outside(buf, g.region, what + ": a read-only operand")
        if getattr(g, "orig", None) is not None:
            assert torch.equal(g.tensor(buf), g.orig.reshape(g.shape)), f"{what}: a read-only operand was written"


def pack(ctx, name, w, *args):
    """W through packer ``name`` into a guarded buffer; the packing fills its whole region (padding zeros included) and nothing else."""
    cout, cin = w.shape
    wd, wp = Guarded(w), nan_like((getattr(ctx.lib, name + "_floats")(cin, cout, *args[:1] if "chain" in name else ()),))
    L.call(name, wd.ptr, wp.ptr, cin, cout, *args, ctx.stream)
    ctx.sync()
    buf = wp.host()
    only_nan_outside(buf, wp.region, name)
    assert torch.isfinite(wp.tensor(buf)).all(), f"{name}: the packing left part of its region unwritten"
    return wp


def finish(ctx, rc, what):
    msg = ctx.lib.nd_last_error().decode() if rc else ""
    try:
        ctx.sync()
    except L.HipError as e:
        rc, msg = 1, str(e)
    if rc > 0:          # a HIP error, not a refusal (those are negative): the device may have faulted -- nothing more runs on it from this file
        pytest.exit(f"{what}: HIP error {rc}: {msg}", returncode=3)
    return rc, msg


# ================================================================================================================ the GEMM entries

def row(body, tile, B, HW, cin, cout, c0=0, pro="none", act="none", ep="b", svec=False, why=""):
    return dict(body=body, tile=tile, B=B, HW=HW, cin=cin, cout=cout, c0=c0, pro=pro, act=act, ep=ep, svec=svec, why=why)


# body / tile: what pw_run (pointwise.hip) chooses by its rules; B / HW may be functions of the CU count; ep: b = bias, v = vec, 0 = res0, 1 = res1, g = gn_t + gn_mad
GEMM = {
    # ---- generic: pointwise_kernel.  pw_pipe_takes says no (cin % 32 != 0 or cin < 64, or LayerNorm without rowstats)
    "g_cin4": row("generic", (1, 1), 2, 37, 4, 16, why="cinP = 8: ng = 1, half of the only K group is padding (`cvalid`, `min(g, ng - 1)`)"),
    "g_cin8_cout96": row("generic", (1, 1), 2, 37, 8, 96, act="gelu", ep="b0", why="one K group; cout = 64 + 32: the second 64-wide tile is ragged (`nvalid`)"),
    "g_cin24": row("generic", (1, 1), 2, 37, 24, 16, pro="silu", ep="b01", why="ng = 3 (`if (g < ng)` branch of the MFMA loop)"),
    "g_cin48_ln": row("generic", (1, 1), 2, 37, 48, 32, pro="ln", svec=True, act="gelu", ep="bv", why="in-kernel row statistics (`nd_row16_sum`), 12 of 16 lanes valid"),
    "g_cin80_cat": row("generic", (1, 1), 2, 37, 80, 24, c0=36, ep="b", why="two chunks, ng = 2 in the second; concat 36 + 44 inside the first chunk"),
    "g_cin80_ln": row("generic", (1, 1), 2, 37, 80, 24, pro="ln", svec=True, ep="b0", why="LayerNorm from rowstats in the generic kernel: cin > 64 and cin % 32 != 0"),
    "g_cin80_affine": row("generic", (1, 1), 2, 37, 80, 24, pro="affine", ep="bg", why="affine prologue over two chunks (`tM / tA / tD` per chunk)"),
    "g_cout4_vec": row("generic", (1, 1), 2, 37, 16, 4, ep="bv", why="cout = 4 with vec: pw_run's narrow test has `!d->vec`, the MFMA tile is 60 / 64 padding"),
    "g_cout6": row("generic", (1, 1), 2, 37, 16, 6, act="silu", ep="b01", why="cout % 4 != 0 without per-sample operands: pw_epilogue's scalar tail"),
    "g_cout6_vec": row("generic", (1, 1), 1, 37, 16, 6, ep="bv", why="cout = 6 with vec at B = 1: quad 0 reads vec + 0 aligned, the quad at n = 4 takes the scalar tail"),
    "g_cout10": row("generic", (1, 1), 1, 37, 16, 10, ep="b0", why="two whole quads on the 16-byte path and a scalar tail of 2"),
    "g_hw1": row("generic", (1, 1), 3, 1, 24, 16, ep="bv0", why="HW = 1: every staging row but one clamped to `HW - 1`"),
    "g_hw65": row("generic", (1, 1), 2, 65, 8, 16, ep="b0", why="one row over a 64-pixel tile: the slow epilogue path (`p0 + BM <= HW` fails)"),
    "g_12": row("generic", (1, 2), 1, 64 * 511 + 37, 24, 128, ep="b0", why="launch<1,2>: cout % 128 == 0 and count(1, 2) = 512 workgroups, the last pixel tile ragged"),
    # ---- pipe: pointwise_pipe_kernel.  cin % 32 == 0, cin >= 64; not big (cout % 128 != 0, cin % 64 != 0, or fewer 128-pixel tiles than CUs)
    "p_cin64": row("pipe", (1, 1), 2, 70, 64, 32, pro="silu", ep="b0", why="n_chunks = 2: the `n_chunks - c == 2` tail with c = 0"),
    "p_cin96_cat": row("pipe", (1, 1), 2, 70, 96, 96, c0=40, pro="leaky", ep="b01", why="n_chunks = 3: one trip of the unrolled loop, the odd tail; concat inside chunk 1"),
    "p_cin128_ln": row("pipe", (1, 1), 2, 70, 128, 64, pro="ln", svec=True, act="gelu", ep="bv0", why="n_chunks = 4: the loop, then the two-chunk tail; rowstats"),
    "p_cin64_affine": row("pipe", (1, 1), 2, 70, 64, 32, pro="affine", ep="bv01g", why="affine prologue, all five epilogue operands"),
    "p_cin64_none": row("pipe", (1, 1), 2, 64, 64, 32, ep="bv01g", why="no prologue; HW = 64: the fast epilogue path with every operand"),
    "p_12": row("pipe", (1, 2), 1, 64 * 255 + 21, 96, 256, ep="b0", why="launch_pipe<1,2>: 256 pixel tiles x 2 = 512 workgroups; cin % 64 != 0 keeps it off the big kernel"),
    # ---- big: pointwise_big_kernel.  cin % 64 == 0, cin >= 128, cout % 128 == 0, B ceil(HW / 128) (cout / 128) >= CUs (pw_big_tiles)
    "b_cin128_affine": row("big", (2, 2), 1, lambda n: 128 * n + 50, 128, 128, pro="affine", ep="bv01g", why="CUs + 1 tiles, the last ragged; affine; five epilogue operands"),
    "b_cin192_cat": row("big", (2, 2), lambda n: n // 2 + 1, 178, 192, 128, c0=64, pro="leaky", ep="b0", why="three chunks (weight ring wraps), concat at 64, every sample's second tile ragged"),
    "b_cin128_ln": row("big", (2, 2), 1, lambda n: 128 * n + 50, 128, 128, pro="ln", svec=True, act="gelu", ep="bv", why="LayerNorm from rowstats"),
    "b_cin128_none": row("big", (2, 2), 1, lambda n: 128 * n + 50, 128, 128, ep="b0", why="launch_big's `default:` instantiation <2, ND_PRO_NONE>, the form of most wide layers; CUs + 1 tiles, the last ragged"),
    "b_cin128_silu": row("big", (2, 2), 1, lambda n: 128 * n, 128, 128, pro="silu", ep="b", why="exactly one tile per CU (tiles >= CUs holds with equality), no ragged tile"),
    # ---- narrow: pointwise_narrow_kernel.  cout 4 / 8, no prologue, no vec / gn
    "n_cin4": row("narrow4", (0, 0), 2, 37, 4, 4, ep="b", why="nq = 1: three of a pixel's four lanes have no channel quad"),
    "n_cin24_cat": row("narrow8", (0, 0), 2, 37, 24, 8, c0=8, act="silu", ep="b01", why="concat 8 + 16 (`r1 = p1 + pc ld1 - c0`), activation and two residuals"),
    "n_cin1024": row("narrow8", (0, 0), 1, 37, 1024, 8, ep="b", why="the whole 32 KB LDS weight image (`wl[256 * 8 * 4]`)"),
    "n_trip": row("narrow4", (0, 0), 1, lambda n: 64 * 8 * n + 37, 8, 4, ep="b0", why="grid = 8 CUs blocks: the first 37-pixel block of a second grid-stride trip"),
}
# ---- the split entry: pointwise_split_kernel (pw_split_shape: cin % 32 == 0, cin >= 64, cout % 128 == 0)
SPLIT = {
    "s_cin64": row("split", None, 2, 130, 64, 128, ep="b", why="two chunks; HW = 130: a second 128-pixel tile of 2 rows"),
    "s_cin96_cat": row("split", None, 2, 130, 96, 128, c0=32, pro="silu", ep="b0", why="three chunks (`cbn` re-stage, `min(.., last_ks)`), concat at 32"),
    "s_cin64_ln": row("split", None, 2, 130, 64, 128, pro="ln", svec=True, act="gelu", ep="bv", why="LayerNorm from rowstats"),
    "s_cin64_gn": row("split", None, 2, 130, 64, 256, ep="b01g", why="two cout tiles; the GroupNorm tail and both residuals in the epilogue"),
}


def resolve(r):
    n = cus()
    f = lambda v: v(n) if callable(v) else v
    return f(r["B"]), f(r["HW"])


@functools.lru_cache(maxsize=2)
def gemm_case(name, B, HW):
    r = {**GEMM, **SPLIT}[name]
    cin, cout, c0, ep = r["cin"], r["cout"], r["c0"], r["ep"]
    u = lambda n, shp, lo=-1.0, hi=1.0: R.U(f"{name}.{n}", shp, lo, hi)
    x = u("x", (B, HW, cin), -1.5, 1.5)
    inp = {"pro": r["pro"], "act": r["act"], "w": u("w", (cout, cin), -0.3, 0.3)}
    if c0:
        inp["x"], inp["x2"] = x[..., :c0].contiguous(), x[..., c0:].contiguous()
    else:
        inp["x"] = x
    if r["pro"] == "affine":
        inp["mad"] = u("mad", (B, 3, cin), 0.5, 1.5)
    if r["pro"] == "ln":
        inp["gamma"], inp["beta"] = u("g", (cin,), 0.5, 1.5), u("be", (cin,))
        if r["svec"]:
            inp["svec"] = u("sv", (B, cin))
    for key, nm, shp in (("b", "b", (cout,)), ("v", "vec", (B, cout)), ("0", "res0", (B, HW, cout)), ("1", "res1", (B, HW, cout))):
        if key in ep:
            inp[nm] = u(nm, shp)
    if "g" in ep:
        inp["gn_t"], inp["gn_mad"] = u("t", (B, HW, cout), -2, 2), u("gmad", (B, 3, cout), 0.5, 1.5)
    body = r["body"]
    gemm = R.gemm32_split if body == "split" else R.gemm32_narrow if body.startswith("narrow") else R.gemm32_mfma
    return inp, R.operator(inp, R.F64), R.operator(inp, R.F32, gemm)


def gemm_desc(ctx, r, inp, B, HW, split=False):
    """nd_pointwise of a case on guarded buffers -> (descriptor, output Guarded, every buffer)."""
    cin, cout = r["cin"], r["cout"]
    d, keep = L.Pointwise(), []
    g = lambda t, extra=None: keep.append(flat(t) if extra is None else img(t, extra)) or keep[-1]
    s = d.src
    x = g(inp["x"], 8)
    s.p0, s.c0, s.ld0 = x.ptr, inp["x"].shape[-1], x.ld
    if "x2" in inp:
        x2 = g(inp["x2"], 16)
        s.p1, s.c1, s.ld1 = x2.ptr, inp["x2"].shape[-1], x2.ld
    s.mode = MODES[inp["pro"]]
    if "mad" in inp:
        s.mad = g(inp["mad"]).ptr
    if inp["pro"] == "ln":
        s.gamma, s.beta = g(inp["gamma"]).ptr, g(inp["beta"]).ptr
        if "svec" in inp:
            s.vec = g(inp["svec"]).ptr
        if cin > 64 or split:
            s.rowstats = g(R.rowstats(inp)).ptr
    wp = pack(ctx, "nd_pack_pointwise_weight_split", inp["w"]) if split else pack(ctx, "nd_pack_pointwise_weight", inp["w"], 0)
    keep.append(wp)
    out = img(torch.full((B, HW, cout), float("nan")), 4)
    out.is_out = True
    d.weight, d.out, d.ldo = wp.ptr, out.ptr, out.ld
    d.B, d.HW, d.W, d.cin, d.cout, d.act = B, HW, HW, cin, cout, ACTS[inp["act"]]
    if "b" in inp:
        d.bias = g(inp["b"]).ptr
    if "vec" in inp:
        d.vec = g(inp["vec"]).ptr
    if "res0" in inp:
        r0 = g(inp["res0"], 8)
        d.res0, d.ldr0 = r0.ptr, r0.ld
    if "res1" in inp:
        r1 = g(inp["res1"], 12)
        d.res1, d.ldr1 = r1.ptr, r1.ld
    if "gn_t" in inp:
        t = g(inp["gn_t"], 4)
        d.gn_t, d.ldt, d.gn_mad = t.ptr, t.ld, g(inp["gn_mad"]).ptr
    return d, out, keep


def run_twice(ctx, call, out, shape, r64, r32, keep, what):
    rc, msg = finish(ctx, call(), what)
    assert rc == 0, f"{what}: refused ({rc}: {msg}) but not listed in REFUSALS"
    buf = out.host()
    only_nan_outside(buf, out.region, what)
    got = out.tensor(buf).reshape(shape)
    derived(got, r64, r32, what)
    intact(keep, what)
    rc, msg = finish(ctx, call(), what)
    assert rc == 0
    assert torch.equal(out.host().nan_to_num(1e30), buf.nan_to_num(1e30)), f"{what}: a repeated call gave other bits"
    return got


@pytest.mark.parametrize("name", list(GEMM))
def test_gemm_bodies(ctx, name):
    r = GEMM[name]
    B, HW = resolve(r)
    inp, r64, r32 = gemm_case(name, B, HW)
    d, out, keep = gemm_desc(ctx, r, inp, B, HW)
    assert ctx.lib.nd_pointwise_gemm_takes(C.byref(d)) == 1
    run_twice(ctx, lambda: ctx.lib.nd_pointwise_gemm_nhwc_f32(C.byref(d), ctx.stream), out, (B, HW, r["cout"]), r64, r32, keep, f"{r['body']} {name}")


@pytest.mark.parametrize("name", list(SPLIT))
def test_split_gemm(ctx, name):
    r = SPLIT[name]
    B, HW = resolve(r)
    inp, r64, r32 = gemm_case(name, B, HW)
    d, out, keep = gemm_desc(ctx, r, inp, B, HW, split=True)
    assert ctx.lib.nd_pointwise_gemm_split_takes(C.byref(d)) == 1
    run_twice(ctx, lambda: ctx.lib.nd_pointwise_gemm_split_nhwc_f32(C.byref(d), ctx.stream), out, (B, HW, r["cout"]), r64, r32, keep, f"split {name}")


# ================================================================================================================ the folded narrow kernel

@pytest.mark.parametrize("cout", [4, 8])
def test_narrow_fold_second_trip(ctx, cout):
    """pointwise_narrow_fold_kernel's grid-stride loop (`base += gridDim.x * 128`, grid = 8 CUs): B = 3 samples, the pixel count just above 128 x 8 x CUs and not a
    multiple of 128, d = 16, distinct M | A | D per sample, res0.  The folded weight is nd_pack_narrow_fold's own, read back for the references: this test pins the KERNEL on the weight it is
    given.  The fold itself (Wf Wr and Wf br + bf in fp64, rounded once) is pinned bit for bit in tests/test_fused_ends.py
    (test_narrow_fold_weights_are_the_fp64_product_rounded_once), and the folded kernel against the UNFOLDED two-layer formula in float64 there too
    (test_narrow_fold_matches_the_unfolded_layers_in_float64)."""
    d_, B = 16, 3
    HW = 128 * 8 * cus() // 3 + 13
    HW += (B * HW) % 128 == 0
    assert B * HW > 128 * 8 * cus() and (B * HW) % 128
    u = lambda n, shp, lo=-1.0, hi=1.0: R.U(f"nf{cout}.{n}", shp, lo, hi)
    wf, bf, wr, br = u("wf", (cout, d_), -0.3, 0.3), u("bf", (cout,)), u("wr", (d_, 2 * d_), -0.3, 0.3), u("br", (d_,))
    hw = [Guarded(t) for t in (wf, bf, wr, br)]
    wp, bp = nan_like((ctx.lib.nd_pack_narrow_fold_floats(3 * d_, cout),)), nan_like((cout,))
    L.call("nd_pack_narrow_fold", hw[0].ptr, hw[1].ptr, hw[2].ptr, hw[3].ptr, wp.ptr, bp.ptr, 2 * d_, d_, cout, ctx.stream)
    ctx.sync()
    wbuf, bbuf = wp.host(), bp.host()
    only_nan_outside(wbuf, wp.region, "nd_pack_narrow_fold weight")
    only_nan_outside(bbuf, bp.region, "nd_pack_narrow_fold bias")
    W = wp.tensor(wbuf).reshape(3 * d_ // 4, cout, 4).permute(1, 0, 2).reshape(cout, 3 * d_).contiguous()
    inp = {"x": u("xp", (B, HW, d_), -1.5, 1.5), "x2": u("x0", (B, HW, d_), -1.5, 1.5), "t": u("t", (B, HW, d_), -2, 2), "mad": u("mad", (B, 3, d_), 0.5, 1.5),
           "w": W, "b": bp.tensor(bbuf).clone(), "res0": u("res", (B, HW, cout))}
    r64, r32 = R.narrow_fold(inp, R.F64), R.narrow_fold(inp, R.F32, lambda x, w: R.gemm32_narrow(x, w, [d_, d_, d_]))
    x, x2, t, res, mad = img(inp["x"], 8), img(inp["x2"], 16), img(inp["t"], 4), img(inp["res0"], 8), flat(inp["mad"])
    out = img(torch.full((B, HW, cout), float("nan")), 4)
    out.is_out = True
    nf = L.NarrowFold()
    nf.p0, nf.p1, nf.t, nf.mad, nf.weight, nf.bias, nf.res0, nf.out = x.ptr, x2.ptr, t.ptr, mad.ptr, wp.ptr, bp.ptr, res.ptr, out.ptr
    nf.B, nf.HW, nf.c0, nf.c1, nf.c2, nf.ld0, nf.ld1, nf.ldt, nf.cout, nf.ldo, nf.ldr0 = B, HW, d_, d_, d_, x.ld, x2.ld, t.ld, cout, out.ld, res.ld
    run_twice(ctx, lambda: ctx.lib.nd_pointwise_narrow_fold_nhwc_f32(C.byref(nf), ctx.stream), out, (B, HW, cout), r64, r32, [x, x2, t, res, mad, wp, bp],
              f"narrow fold cout={cout} second trip")


# ================================================================================================================ the chains

# every row of nd_pointwise_chain_supported's table (pwchain.hip) = every row of chain_run's split list with K0 rounded up to 16: real widths -> (K0, N1, N2, N3)
CHAINS = {
    "8_24_16": ([8, 24, 16], 4),           # {8, 32, 32, 0} / split {16, 32, 32, 0}: two sources 4 + 4 (split: the TWO form), ragged stage widths
    "16_16_16": ([16, 16, 16], 0),         # {16, 32, 32, 0}
    "16_32_16_16": ([16, 32, 16, 16], 0),  # {16, 32, 32, 32}
    "32_32_32": ([32, 32, 32], 0),         # {32, 32, 32, 0}
    "32_32_32_32": ([32, 32, 32, 32], 0),  # {32, 32, 32, 32}
    "32_64_32_32": ([32, 64, 32, 32], 0),  # {32, 64, 32, 32}
    "8_64_64": ([8, 64, 64], 4),           # {8, 64, 64, 0} / split {16, 64, 64, 0}: shot_mlp1's cat[clean_img, x]
    "48_48_48": ([48, 48, 48], 0),         # {48, 64, 64, 0}
    "48_96_48_48": ([48, 96, 48, 48], 0),  # {48, 96, 64, 64}
    "64_64_64": ([64, 64, 64], 0),         # {64, 64, 64, 0}
    "64_128_64_64": ([64, 128, 64, 64], 0),  # {64, 128, 64, 64}: 768 threads (chain_threads)
    "64_64_4": ([64, 64, 4], 0),           # {64, 64, 32, 0}
    "48_48_4": ([48, 48, 4], 0),           # {48, 64, 32, 0}
}
ENTRY = {"fp32": ("nd_pack_chain_weight", "nd_pointwise_chain_nhwc_f32", R.gemm32_mfma), "split": ("nd_pack_chain_weight_split", "nd_pointwise_chain_split_nhwc_f32", R.gemm32_split),
         "tail": ("nd_pack_chain_weight_split", "nd_pointwise_chain_tail_split_nhwc_f32", R.gemm32_split)}


@functools.lru_cache(maxsize=2)
def chain_inputs(name, B, HW, tail=False, ln=None):
    """Mlp (two stages: fc2(GELU(fc1(x)))) or AttnBlock tail (three: LayerNorm(x + v), GELU, + x + v, + x); ``ln`` forces the prologue and vec on a two-stage chain."""
    widths, c0 = CHAINS[name]
    n, cin = len(widths) - 1, widths[0]
    u = lambda nm, shp, lo=-1.0, hi=1.0: R.U(f"ch.{name}.{nm}", shp, lo, hi)
    x = u("x", (B, HW, cin), -1.5, 1.5)
    inp = {"ws": [u(f"w{i}", (widths[i + 1], widths[i]), -0.3, 0.3) for i in range(n)], "bs": [u(f"b{i}", (widths[i + 1],)) for i in range(n)]}
    if c0:
        inp["x"], inp["x2"] = x[..., :c0].contiguous(), x[..., c0:].contiguous()
    else:
        inp["x"] = x
    if tail:
        inp.update(tail=True, mad=u("mad", (B, 3, cin), 0.5, 1.5), r0=u("r0", (B, HW, cin), -2, 2), r1=u("r1", (B, HW, cin), -2, 2))
    elif n == 3 or ln:
        inp.update(pro="ln", svec=u("v", (B, cin)), gamma=u("g", (cin,), 0.5, 1.5), beta=u("be", (cin,)))
        if n == 3:
            inp["res"] = (0, 1, 2)
    return inp, R.chain(inp, R.F64)


def chain_desc(ctx, form, name, inp, B, HW):
    widths, _ = CHAINS[name]
    n, keep = len(widths) - 1, []
    g = lambda t, extra=None: keep.append(flat(t) if extra is None else img(t, extra)) or keep[-1]
    dt = L.ChainTail()
    d = dt.chain
    for i in range(n):
        wp = pack(ctx, ENTRY[form][0], inp["ws"][i], int(i == 0))
        keep.append(wp)
        d.st[i].weight, d.st[i].bias, d.st[i].cin, d.st[i].cout = wp.ptr, g(inp["bs"][i]).ptr, widths[i], widths[i + 1]
        d.st[i].act = ACTS[inp.get("acts", ("gelu", "none", "none"))[i]]
        d.st[i].res = inp.get("res", (0, 0, 0))[i]
    s = d.src
    x = g(inp["x"], 8)
    s.p0, s.c0, s.ld0 = x.ptr, inp["x"].shape[-1], x.ld
    if "x2" in inp:
        x2 = g(inp["x2"], 16)
        s.p1, s.c1, s.ld1 = x2.ptr, inp["x2"].shape[-1], x2.ld
    if inp.get("pro") == "ln":
        s.mode, s.gamma, s.beta, s.vec = L.PRO_LAYERNORM, g(inp["gamma"]).ptr, g(inp["beta"]).ptr, g(inp["svec"]).ptr
    if inp.get("tail"):
        r0, r1 = g(inp["r0"], 8), g(inp["r1"], 12)
        dt.mad, dt.r0, dt.ldr0, dt.r1, dt.ldr1 = g(inp["mad"]).ptr, r0.ptr, r0.ld, r1.ptr, r1.ld
    out = img(torch.full((B, HW, widths[-1]), float("nan")), 4)
    out.is_out = True
    d.out, d.n_stages, d.B, d.HW, d.ldo = out.ptr, n, B, HW, out.ld
    return dt, out, keep


def chain_call(ctx, form, dt):
    fn = getattr(ctx.lib, ENTRY[form][1])
    return (lambda: fn(C.byref(dt), ctx.stream)) if form == "tail" else (lambda: fn(C.byref(dt.chain), ctx.stream))


@pytest.mark.parametrize("form", ["fp32", "split"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_every_instantiated_width(ctx, name, form):
    """2 x 64 pixels: four tiles, one per wave.  Two-source rows at cin = 8; three-stage rows with LayerNorm + vec + both residual kinds."""
    B, HW = 2, 64
    widths, _ = CHAINS[name]
    assert ctx.lib.nd_pointwise_chain_supported(widths[0], widths[1], widths[2], widths[3] if len(widths) == 4 else 0)
    assert ctx.lib.nd_pointwise_chain_takes(HW, widths[0], widths[1], widths[2], widths[3] if len(widths) == 4 else 0)
    inp, r64 = chain_inputs(name, B, HW)
    r32 = R.chain(inp, R.F32, ENTRY[form][2])
    dt, out, keep = chain_desc(ctx, form, name, inp, B, HW)
    run_twice(ctx, chain_call(ctx, form, dt), out, (B, HW, widths[-1]), r64, r32, keep, f"chain {form} {name}")


@pytest.mark.parametrize("name", ["64_64_4", "48_48_4"])
def test_chain_tail_widths(ctx, name):
    B, HW = 2, 64
    widths, _ = CHAINS[name]
    inp, r64 = chain_inputs(name, B, HW, tail=True)
    r32 = R.chain(inp, R.F32, R.gemm32_split)
    dt, out, keep = chain_desc(ctx, "tail", name, inp, B, HW)
    run_twice(ctx, chain_call(ctx, "tail", dt), out, (B, HW, widths[-1]), r64, r32, keep, f"chain tail {name}")


@pytest.mark.parametrize("form,name", [("fp32", "16_16_16"), ("split", "16_16_16"), ("fp32", "64_64_4"), ("split", "64_64_4"), ("tail", "64_64_4")])
def test_chain_second_trip(ctx, form, name):
    """The persistent loop's second and third trips (pwchain.hip `for (int t = t_begin; t < t_end; ++t)`): HW = 96 is three tiles per sample and B is chosen so that
    n_tiles ~ 2.5 x 16 waves x CUs, so every wave holds two or three tiles and most cross a sample boundary: the `b != b_cur` reloads of the vec and M | A | D
    stashes, the SPLIT form's prefetch_rows(t + 1) and the reload behind the last tile.  LayerNorm + a distinct vec per sample (fp32, split), distinct M | A | D (tail).
    Then the same output, bit for bit, from launches of at most CUs tiles each -- one tile per wave, the path every other test runs.
    (d = 64: 327 k pixels x 64 channels on 256 CUs; the fp32 reference's sequential chain over them is what takes this case's seconds.)"""
    HW = 96
    B = -(-(5 * 16 * cus() // 2) // 3)
    widths, _ = CHAINS[name]
    assert 3 * B > 2 * 16 * cus()
    inp, r64 = chain_inputs(name, B, HW, tail=form == "tail", ln=form != "tail")
    r32 = R.chain(inp, R.F32, ENTRY[form][2])
    dt, out, keep = chain_desc(ctx, form, name, inp, B, HW)
    got = run_twice(ctx, chain_call(ctx, form, dt), out, (B, HW, widths[-1]), r64, r32, keep, f"chain {form} {name} second trip")
    # in pieces of whole samples, at most CUs tiles per launch
    out2 = img(torch.full((B, HW, widths[-1]), float("nan")), 4)
    step, d, s, cin = max(cus() // 3, 1), dt.chain, dt.chain.src, widths[0]
    base = {"p0": s.p0, "vec": s.vec, "mad": dt.mad, "r0": dt.r0, "r1": dt.r1}
    for b0 in range(0, B, step):
        px = 4 * b0 * HW
        s.p0, d.out, d.B = base["p0"] + px * s.ld0, out2.ptr + px * d.ldo, min(step, B - b0)
        if base["vec"]:
            s.vec = base["vec"] + 4 * b0 * cin
        if form == "tail":
            dt.mad, dt.r0, dt.r1 = base["mad"] + 4 * b0 * 3 * cin, base["r0"] + px * dt.ldr0, base["r1"] + px * dt.ldr1
        assert 3 * d.B <= cus()
        rc = chain_call(ctx, form, dt)()
        assert rc == 0, ctx.lib.nd_last_error()
    finish(ctx, 0, "pieces")
    buf2 = out2.host()
    only_nan_outside(buf2, out2.region, "pieces")
    assert torch.equal(out2.tensor(buf2).reshape(B, HW, -1), got), f"chain {form} {name}: the persistent loop and one tile per wave give different bits"


# ================================================================================================================ refusals

def _small(name):
    r = dict({**GEMM, **SPLIT}[name])
    B, HW = resolve(r)
    inp = dict(gemm_case(name, B, HW)[0])
    return r, inp, B, HW


def _set(path, value):
    def f(d):
        obj = d
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value(obj) if callable(value) else value)
    return f


# name -> (base row, split entry, descriptor mutation, fragment of the message).  Rows of OPERANDS are refused for an operand that is given (its stride): the
# entry's pointer part; every other row is refused by the shape part, which the question of the entry answers too.
OPERANDS = {"ldr0_below_cout", "ldr1_not_a_multiple_of_4", "ldt_below_cout"}
REFUSALS = {
    "ln_cin_above_1024": ("ln1028", False, None, "C <= 1024"),
    "ln_wide_without_rowstats": ("g_cin80_ln", False, _set("src.rowstats", None), "needs src.rowstats"),
    "ln_two_sources": ("g_cin48_ln", False, lambda d: (_set("src.c0", 24)(d), _set("src.c1", 24)(d), _set("src.p1", d.src.p0)(d), _set("src.ld1", d.src.ld0)(d)), "LayerNorm needs gamma/beta, one source"),
    "affine_two_sources": ("g_cin80_affine", False, lambda d: (_set("src.c0", 40)(d), _set("src.c1", 40)(d), _set("src.p1", d.src.p0)(d), _set("src.ld1", d.src.ld0)(d)), "affine prologue needs mad, one source"),
    "ld0_below_channels": ("g_cin24", False, _set("src.ld0", 20), "ld < channels"),
    "ld0_not_a_multiple_of_4": ("g_cin24", False, _set("src.ld0", 26), "pixel strides must be multiples of 4"),
    "ldo_below_cout": ("g_cin24", False, _set("ldo", 12), "ldo < cout"),
    "ldo_not_a_multiple_of_4": ("g_cin24", False, _set("ldo", 18), "strides must be multiples of 4"),
    "ldr0_below_cout": ("g_cin24", False, _set("ldr0", 12), "ldr0 < cout"),
    "ldr1_not_a_multiple_of_4": ("g_cin24", False, _set("ldr1", 30), "strides must be multiples of 4"),
    "ldt_below_cout": ("g_cin80_affine", False, _set("ldt", 20), "ldt >= cout"),
    "split_cin_48": ("g_cin48_ln", True, None, "not a layer of the split kernel"),
    "split_cout_96": ("p_cin96_cat", True, None, "not a layer of the split kernel"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gemm_refusals(ctx, name):
    base, split, mutate, why = REFUSALS[name]
    if base == "ln1028":
        r = row("generic", (1, 1), 1, 5, 1028, 16, pro="ln", ep="b")
        x = R.U("ln1028.x", (1, 5, 1028))
        inp = {"pro": "ln", "act": "none", "x": x, "w": R.U("ln1028.w", (16, 1028)), "b": R.U("ln1028.b", (16,)), "gamma": R.U("ln1028.g", (1028,)), "beta": R.U("ln1028.be", (1028,))}
        B, HW = 1, 5
    else:
        r, inp, B, HW = _small(base)
    d, out, keep = gemm_desc(ctx, r, inp, B, HW, split=False)          # (a refused call reads no weight: the plain packing stands in for the split one)
    if callable(mutate):
        mutate(d)
    fn = ctx.lib.nd_pointwise_gemm_split_nhwc_f32 if split else ctx.lib.nd_pointwise_gemm_nhwc_f32
    takes = ctx.lib.nd_pointwise_gemm_split_takes if split else ctx.lib.nd_pointwise_gemm_takes
    rc, msg = finish(ctx, fn(C.byref(d), ctx.stream), name)
    assert rc < 0 and why in msg, f"{name}: expected a refusal with '{why}', got rc {rc} '{msg}'"
    assert msg.startswith("nd_pointwise_gemm_split: " if "split kernel" in why else "nd_pointwise: "), msg
    assert torch.isnan(out.host()).all(), f"{name}: a refused call wrote to the output"
    assert takes(C.byref(d)) == (1 if name in OPERANDS else 0), f"{name}: the question and the entry disagree"


CHAIN_REFUSALS = {
    "hw_not_a_multiple_of_32": ("fp32", "16_16_16", lambda dt: setattr(dt.chain, "HW", 40), "multiple of 32"),
    "widths_not_instantiated": ("fp32", "16_16_16", lambda dt: (setattr(dt.chain.st[0], "cout", 160), setattr(dt.chain.st[1], "cin", 160)), "not instantiated"),
    "split_widths_not_instantiated": ("split", "16_16_16", lambda dt: (setattr(dt.chain.st[0], "cout", 160), setattr(dt.chain.st[1], "cin", 160)), "not instantiated"),
    "split_two_sources_cin_32": ("split", "32_32_32", lambda dt: (setattr(dt.chain.src, "c0", 16), setattr(dt.chain.src, "c1", 16), setattr(dt.chain.src, "p1", dt.chain.src.p0),
                                                                  setattr(dt.chain.src, "ld1", dt.chain.src.ld0)), "two sources only with cin <= 16"),
    "tail_with_vec": ("tail", "64_64_4", lambda dt: setattr(dt.chain.src, "vec", dt.mad), "one plain source"),
    "tail_widths_not_instantiated": ("tail", "64_64_64", None, "not instantiated"),
}


@pytest.mark.parametrize("name", list(CHAIN_REFUSALS))
def test_chain_refusals(ctx, name):
    form, base, mutate, why = CHAIN_REFUSALS[name]
    B, HW = 2, 64
    inp, _ = chain_inputs(base, B, HW, tail=form == "tail")
    dt, out, keep = chain_desc(ctx, form, base, inp, B, HW)
    if mutate:
        mutate(dt)
    rc, msg = finish(ctx, chain_call(ctx, form, dt)(), name)
    assert rc < 0 and why in msg, f"{name}: expected a refusal with '{why}', got rc {rc} '{msg}'"
    assert torch.isnan(out.host()).all(), f"{name}: a refused call wrote to the output"
    if form != "tail" and ("multiple of 32" in why or "not instantiated" in why):      # what nd_pointwise_chain_takes answers for: pixel tiles and widths
        ch = dt.chain
        assert ctx.lib.nd_pointwise_chain_takes(ch.HW, ch.src.c0 + ch.src.c1, ch.st[0].cout, ch.st[1].cout, ch.st[2].cout if ch.n_stages == 3 else 0) == 0


def test_the_library_instantiates_no_chain_the_list_lacks(ctx):
    """CHAINS is this file's own list of the instantiated widths; the library's table (one X-macro in pwchain.hip) has no further row on a grid around it."""
    up = lambda v, m: -(-v // m) * m
    listed = {(up(w[0], 8), up(w[1], 32), up(w[2], 32), up(w[3], 32) if len(w) == 4 else 0) for w, _ in CHAINS.values()}
    assert len(listed) == len(CHAINS) == 13
    grid = [(k0, n1, n2, n3) for k0 in range(8, 89, 8) for n1 in range(32, 193, 32) for n2 in range(32, 193, 32) for n3 in range(0, 193, 32)]
    assert {g for g in grid if ctx.lib.nd_pointwise_chain_supported(*g)} == listed
    assert {g for g in grid if ctx.lib.nd_pointwise_chain_takes(64, *g)} == listed and not any(ctx.lib.nd_pointwise_chain_takes(48, *g) for g in listed)


# ================================================================================================================ packers

def test_transposed_and_batched_packers_equal_the_plain_packer_bit_for_bit(ctx):
    """nd_pack_pointwise_weight_t of W^T and each item of nd_pack_pointwise_weights_batch == nd_pack_pointwise_weight of W, padding zeros included, guards intact.  Three
    shapes in one batch: cin and cout below their padding units, a ragged cin over several 64-cout blocks, and one item transposed."""
    shapes = [(20, 12), (130, 72), (64, 100)]              # (cout, cin)
    ws = [R.U(f"pk.{i}", s) for i, s in enumerate(shapes)]
    plain = [pack(ctx, "nd_pack_pointwise_weight", w, 0) for w in ws]
    for w, p in zip(ws, plain):
        assert torch.equal(p.tensor(), R.pack_layout(w)), "nd_pack_pointwise_weight: not [cinP / 4][coutP][4] with zero padding"
    # transposed
    for w, p in zip(ws, plain):
        cout, cin = w.shape
        wt, out = Guarded(w.T.contiguous()), nan_like((ctx.lib.nd_pack_pointwise_weight_floats(cin, cout),))
        L.call("nd_pack_pointwise_weight_t", wt.ptr, out.ptr, cin, cout, ctx.stream)
        ctx.sync()
        buf = out.host()
        only_nan_outside(buf, out.region, "nd_pack_pointwise_weight_t")
        assert torch.equal(out.tensor(buf), p.tensor())
    # batch: item 1 transposed
    srcs = [Guarded(w.T.contiguous() if i == 1 else w) for i, w in enumerate(ws)]
    outs = [nan_like((ctx.lib.nd_pack_pointwise_weight_floats(w.shape[1], w.shape[0]),)) for w in ws]
    items = (L.PackItem * 3)()
    for i, w in enumerate(ws):
        items[i].w, items[i].packed, items[i].cin, items[i].cout, items[i].transposed = srcs[i].ptr, outs[i].ptr, w.shape[1], w.shape[0], int(i == 1)
    import hiputil as hu
    table = hu.dev(torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8))
    L.call("nd_pack_pointwise_weights_batch", table.data_ptr(), 3, ctx.stream)
    ctx.sync()
    for o, p in zip(outs, plain):
        buf = o.host()
        only_nan_outside(buf, o.region, "nd_pack_pointwise_weights_batch")
        assert torch.equal(o.tensor(buf), p.tensor())
