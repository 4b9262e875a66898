"""Downsample (pixel-unshuffle + 1x1) on the streaming kernels: nd_pointwise_downsample_nhwc_f32.

The GPU cases run the entry against float64 of unshuffle + 1x1 (Diffusion_arch.py:80-81: 'b c (h p1) (w p2) -> b (c p1 p2) h w', then the conv): 128 -> 128 on the
split kernel's unshuffled instance, 256 -> 64 on the pipelined kernel's; outputs of 8 x 12 pixels (a partial tile of either kernel) and 16 x 16 (two 128-pixel tiles,
four 64-pixel ones), B = 2, each route once with a source stride of c0 / 4 + 4.  Bound: util.derived on the fp32 reference of tests/pointwise_ref.py in the route's own
accumulation order over the kernel's K order (p1 p2 c).  The question and the refusals need the library only, no GPU."""
import ctypes as C

import pytest
import torch

import pointwise_ref as R
from noisediff_amd import _lib as L
from noisediff_amd import synth
from util import derived


@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(41, "down." + name, shape, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("cs,cout,h,w,pad", [(32, 128, 8, 12, 0), (32, 128, 16, 16, 4), (64, 64, 8, 12, 4), (64, 64, 16, 16, 0)])
def test_downsample_entry_matches_unshuffle_and_1x1_in_float64(ctx, cs, cout, h, w, pad):
    import hiputil as hu
    B, cin, split = 2, 4 * cs, cout % 128 == 0
    case = f"{cs}.{cout}.{h}x{w}"
    x = U(case + ".x", (B, 2 * h, 2 * w, cs), -1.5, 1.5)
    wt, bias = U(f"w.{cs}.{cout}", (cout, cin), -0.3, 0.3), U(f"b.{cout}", (cout,))
    # torch order (c p1 p2) for the float64 reference; the kernel's K order (p1 p2 c) for the fp32 one
    sub = x.view(B, h, 2, w, 2, cs).permute(0, 1, 3, 2, 4, 5).reshape(B, h * w, 4, cs)         # [b][pixel][p1 p2][c]
    ref64 = sub.permute(0, 1, 3, 2).reshape(B, h * w, cin).double() @ wt.double().T + bias.double()
    xk, wk = sub.reshape(B * h * w, cin), wt.view(cout, cs, 4).permute(0, 2, 1).reshape(cout, cin).contiguous()
    ref32 = ((R.gemm32_split if split else R.gemm32_mfma)(xk, wk) + bias).view(B, h * w, cout)

    wd = hu.dev(wt)
    if split:
        wp = hu.full((ctx.lib.nd_pack_pointwise_weight_split_floats(cin, cout),))
        L.call("nd_pack_pointwise_weight_split_unshuffle", wd.data_ptr(), wp.data_ptr(), cin, cout, cs, ctx.stream)
        ctx.sync()
        assert torch.isfinite(wp).all()
    else:
        wp = hu.pack_pw(ctx, wt, unshuffle_c=cs)
    buf = torch.full((B, 2 * h, 2 * w, cs + pad), float("nan"))                              # NaN in the pad columns: a read past c0 / 4 poisons the output
    buf[..., :cs] = x
    xd, bd = hu.dev(buf), hu.dev(bias)
    ldo = cout + 4
    out = hu.full((B * h * w + 3, ldo))
    d = L.pointwise(L.src(xd, None, L.PRO_NONE, cin, cs + pad, unshuffle=1), wp, bd, out, B, h * w, w, cin, cout, ldo=ldo)
    assert ctx.lib.nd_pointwise_downsample_takes(C.byref(d))
    L.call("nd_pointwise_downsample_nhwc_f32", C.byref(d), ctx.stream)
    ctx.sync()
    got = out.cpu()
    assert torch.isnan(got[B * h * w:]).all() and torch.isnan(got[:B * h * w, cout:]).all(), "the kernel wrote outside its output"
    assert derived(got[:B * h * w, :cout].reshape(B, h * w, cout), ref64, ref32, f"downsample {'split' if split else 'pipe'} {case} pad={pad}")
    L.call("nd_pointwise_downsample_nhwc_f32", C.byref(d), ctx.stream)
    ctx.sync()
    assert torch.equal(out.cpu()[:B * h * w, :cout], got[:B * h * w, :cout])


def _down(cs=32, cout=128, ld0=None, ldo=None, HW=32, W=8, **kw):
    """nd_pointwise_downsample_takes on a one-sample descriptor of 32 output pixels (rows of 8); ``kw``: further fields of the descriptor or of its source."""
    d = L.Pointwise(B=1, HW=HW, W=W, cin=4 * cs, cout=cout, ldo=cout if ldo is None else ldo)
    d.src.c0, d.src.ld0, d.src.unshuffle = 4 * cs, cs if ld0 is None else ld0, 1
    for k, v in kw.items():                                              # (`vec` names the epilogue's operand here; the source's belongs to LayerNorm)
        setattr(d.src if hasattr(d.src, k) and k != "vec" else d, k, v)
    return bool(L.load().nd_pointwise_downsample_takes(C.byref(d)))


def test_downsample_question_answers_on_both_sides_of_each_limit():
    assert _down() and _down(cs=64, cout=64) and _down(cs=128, cout=256)
    assert not _down(unshuffle=0, ld0=128)                                                     # a plain source is the other entries'
    assert not _down(cs=16) and not _down(cs=48) and _down(cs=96) and not _down(cs=33)         # (c0 / 4) % 32
    assert _down(cout=64) and _down(cout=192) and not _down(cout=32) and not _down(cout=96) and not _down(cout=0)
    assert _down(ld0=36) and not _down(ld0=28) and not _down(ld0=34)
    assert _down(ldo=132) and not _down(ldo=124) and not _down(ldo=130)
    assert not _down(c1=32, ld1=32) and not _down(mode=L.PRO_SILU) and not _down(upsample=1)
    assert not _down(shuffle_c=32, shuffle_h=8, shuffle_w=16, ldo=32)
    assert _down(bias=16) and _down(act=L.ACT_SILU) and not _down(act=3)
    for operand in ("res0", "res1", "gn_t", "vec"):                                            # given or not is all the question reads of a pointer
        assert not _down(**{operand: 16}), operand
    assert not _down(W=5) and not _down(HW=0) and _down(HW=35, W=7)
    assert L.load().nd_pointwise_downsample_takes(None) == 0


def test_a_refused_downsample_question_is_not_a_failure_and_the_entry_refuses_with_a_message():
    lib = L.load()
    assert lib.nd_conv3x3_wino_nhwc_f32(None, None) == -1               # a host-only refusal: returns before any HIP call
    said = lib.nd_last_error()
    assert not _down(cs=16) and not _down(cout=96) and not _down(res0=16) and not _down(mode=L.PRO_SILU) and not _down(ld0=28)
    assert lib.nd_last_error() == said
    # the entry itself refuses the same shapes before any HIP call, and says why
    d = L.Pointwise(B=1, HW=32, W=8, cin=64, cout=128, ldo=128)
    d.src.p0 = d.weight = d.out = 0x1000
    d.src.c0, d.src.ld0, d.src.unshuffle = 64, 16, 1
    assert lib.nd_pointwise_downsample_nhwc_f32(C.byref(d), None) == -2 and b"nd_pointwise_downsample_takes" in lib.nd_last_error()
    assert lib.nd_pointwise_downsample_nhwc_f32(None, None) == -1 and b"null" in lib.nd_last_error()
    assert lib.nd_pack_pointwise_weight_split_unshuffle(0x1000, 0x1000, 128, 128, 16, None) == -2
