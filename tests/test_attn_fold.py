"""The tail of a wide AttnBlock as one GEMM: ff.net.2 and proj_out have only additions between them, so

    y = Wp (W2 h1 + b2 + x + cb) + bp + x = [Wp W2 | Wp + I] [h1; x] + (Wp b2 + bp) + Wp cb.

  * nd_pack_attn_tail_fold -- the folded weight and bias are the float64 result rounded ONCE to fp32: equal to torch's float64 product rounded to fp32, except
    where that float64 sum sits on an fp32 rounding boundary (two orders of a C-term float64 sum differ by a few float64 ulps): there the neighbouring fp32 value
    is accepted, and only there (``rounded_once``);
  * the folded launch (nd_pointwise_gemm_split_nhwc_f32 over (h1, x) with vec = Wp cb + bias) against float64 of the UNFOLDED formula; bound: util.derived on the
    fp32 evaluation of the folded formula in the split kernel's accumulation order (tests/pointwise_ref.py);
  * the plans: engine.FOLD_ATTN / engine.DOWN_FAST on against both off."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import pointwise_ref as R
from noisediff_amd import _lib as L
from noisediff_amd import synth
from util import close, derived, state_dict

NET_TOL = 2e-4          # tests/test_hip_net.py's
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(37, "attn_fold." + name, shape, lo, hi)


def _strided(t, ld):
    """Device copy of (rows..., C) with pixel stride ld >= C; the pad columns hold NaN (a kernel that reads them poisons its output)."""
    import hiputil as hu
    buf = torch.full(t.shape[:-1] + (ld,), float("nan"))
    buf[..., :t.shape[-1]] = t
    return hu.dev(buf)


@pytest.fixture(scope="module")
def weights():
    """Per width: W2 (C, 2C), b2, Wp (C, C), bp and their fold in float64 -- computed once, shared, never written."""
    out = {}
    for Cc in (128, 256):
        w2, b2 = U(f"w2.{Cc}", (Cc, 2 * Cc), -0.1, 0.1), U(f"b2.{Cc}", (Cc,))
        wp, bp = U(f"wp.{Cc}", (Cc, Cc), -0.1, 0.1), U(f"bp.{Cc}", (Cc,))
        w64 = torch.cat((wp.double() @ w2.double(), wp.double() + torch.eye(Cc, dtype=torch.float64)), 1)
        b64 = wp.double() @ b2.double() + bp.double()
        # how far two orders of the same float64 sum can lie apart: 2 C ulps of the sum of the terms' magnitudes
        w_slack = torch.cat((2 * Cc * 2.0 ** -53 * (wp.double().abs() @ w2.double().abs()), torch.full((Cc, Cc), 2.0 ** -52, dtype=torch.float64)), 1)
        b_slack = 2 * Cc * 2.0 ** -53 * (wp.double().abs() @ b2.double().abs() + bp.double().abs())
        out[Cc] = dict(w2=w2, b2=b2, wp=wp, bp=bp, w64=w64, b64=b64, w_slack=w_slack, b_slack=b_slack)
    return out


def _fold(ctx, w):
    """nd_pack_attn_tail_fold on the device -> (w_out (C, 3C), b_out (C,)) device tensors; nothing written past them."""
    import hiputil as hu
    Cc = w["wp"].shape[0]
    n = ctx.lib.nd_pack_attn_tail_fold_floats(Cc)
    assert n == 3 * Cc * Cc
    wo, bo = hu.full((n + 8,)), hu.full((Cc + 4,))
    keep = [hu.dev(w[k]) for k in ("w2", "b2", "wp", "bp")]
    L.call("nd_pack_attn_tail_fold", keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), wo.data_ptr(), bo.data_ptr(), Cc, ctx.stream)
    ctx.sync()
    assert torch.isnan(wo[n:]).all() and torch.isnan(bo[Cc:]).all()
    return wo[:n].view(Cc, 3 * Cc), bo[:Cc], keep


def rounded_once(got, ref64, slack, what):
    """``got`` (fp32) is ``ref64`` rounded once: equal to ref64.float(), or its fp32 neighbour where ref64 lies within ``slack`` of the midpoint of the two."""
    ref = ref64.float()
    off = got != ref
    if off.any():
        g, r = got[off], ref[off]
        assert torch.equal(torch.nextafter(r, g), g), f"{what}: more than one ulp from the float64 result"
        assert ((ref64[off] - (g.double() + r.double()) / 2).abs() <= slack[off]).all(), f"{what}: off by an ulp away from a rounding boundary"
    assert int(off.sum()) <= max(1, got.numel() // 10000), f"{what}: {int(off.sum())} of {got.numel()} values on a rounding boundary is no accident"


@pytest.mark.parametrize("Cc", [128, 256])
def test_fold_is_the_float64_product_rounded_once(ctx, weights, Cc):
    w = weights[Cc]
    wo, bo, _ = _fold(ctx, w)
    got_w, got_b = wo.cpu(), bo.cpu()            # from here on no GPU is needed
    rounded_once(got_w, w["w64"], w["w_slack"], f"w_out C={Cc}")
    rounded_once(got_b, w["b64"], w["b_slack"], f"b_out C={Cc}")
    # the identity is IN the weight: the last C columns are Wp with 1 added on the diagonal (one exact float64 addition: no boundary case here)
    assert torch.equal(got_w[:, 2 * Cc:], (w["wp"].double() + torch.eye(Cc, dtype=torch.float64)).float())


@pytest.mark.parametrize("B,H,W,Cc", [(2, 12, 20, 128), (1, 8, 16, 256)])
def test_folded_launch_matches_the_unfolded_formula_in_float64(ctx, weights, B, H, W, Cc):
    """(2, 12 x 20, 128): one whole 128-pixel tile and a partial one per sample, two samples whose cb differ.  (1, 8 x 16, 256): two cout tiles, the concat on a
    32-channel boundary (h1 ends at channel 512).  Strides wider than the channels, NaN in the pad columns and around the output; a second launch gives the same bits."""
    import hiputil as hu
    w = weights[Cc]
    HW = H * W
    h1, x, cb = U(f"h1.{Cc}", (B, HW, 2 * Cc), -1.5, 1.5), U(f"x.{Cc}", (B, HW, Cc), -1.5, 1.5), U(f"cb.{Cc}", (B, Cc))
    w2, b2, wp, bp = (w[k].double() for k in ("w2", "b2", "wp", "bp"))
    x2 = F.linear(h1.double(), w2, b2) + x.double() + cb.double()[:, None]
    ref64 = F.linear(x2, wp, bp) + x.double()
    # the folded formula in fp32, in the split kernel's order: the folded weight and bias rounded once, vec = Wp cb + bias as an fp32 Linear
    wf, bf = w["w64"].float(), w["b64"].float()
    folded = {"x": h1, "x2": x, "w": wf, "vec": F.linear(cb, w["wp"], bf)}
    ref32 = R.operator(folded, R.F32, R.gemm32_split)
    assert float((R.operator(folded, R.F64) - ref64).abs().max()) < 1e-5          # the fold is the same map (up to its one rounding)

    wo, bo, keep = _fold(ctx, w)
    ws = hu.full((ctx.lib.nd_pack_pointwise_weight_split_floats(3 * Cc, Cc),))
    L.call("nd_pack_pointwise_weight_split", wo.data_ptr(), ws.data_ptr(), 3 * Cc, Cc, ctx.stream)
    cbd, cbf, wpp = hu.dev(cb), hu.full((B, Cc)), hu.pack_pw(ctx, w["wp"])          # as the plan forms it: proj_out over the rows of cb, the folded bias
    dv = L.pointwise(L.src(cbd), wpp, bo, cbf, 1, B, B, Cc, Cc)
    L.call("nd_pointwise_gemm_nhwc_f32", C.byref(dv), ctx.stream)
    h1d, xd = _strided(h1, 2 * Cc + 8), _strided(x, Cc + 4)
    ldo = Cc + 4
    out = hu.full((B * HW + 3, ldo))
    d = L.pointwise(L.src(h1d, xd, L.PRO_NONE, 2 * Cc, 2 * Cc + 8, 0, Cc, Cc + 4), ws, None, out, B, HW, W, 3 * Cc, Cc, ldo=ldo, vec=cbf)
    assert ctx.lib.nd_pointwise_gemm_split_takes(C.byref(d))
    L.call("nd_pointwise_gemm_split_nhwc_f32", C.byref(d), ctx.stream)
    ctx.sync()
    got = out.cpu()
    assert torch.isnan(got[B * HW:]).all() and torch.isnan(got[:B * HW, Cc:]).all(), "the kernel wrote outside its output"
    assert derived(got[:B * HW, :Cc].reshape(B, HW, Cc), ref64, ref32, f"folded AttnBlock tail C={Cc} B={B} {H}x{W}")
    L.call("nd_pointwise_gemm_split_nhwc_f32", C.byref(d), ctx.stream)
    ctx.sync()
    assert torch.equal(out.cpu()[:B * HW, :Cc], got[:B * HW, :Cc])


def _names(plan):
    return [op[2] for op in plan.step_ops]


def test_folded_plan_equals_the_unfolded_plan_with_five_launches_fewer(monkeypatch):
    """d = 64, 64 x 64, B = 2: one step's model_out with FOLD_ATTN / DOWN_FAST on against both off, within the net parity tolerance.  The five wide AttnBlocks
    (downs.2.2, downs.3.2, ups.0.2, ups.1.2, ups.2.2) lose one launch each; the three Downsample layers keep their count and change their entry; a debug plan
    records the plain plan's launches (it taps the blocks' outputs, not x2) with the trunk's end and the shot branch unfused, as before."""
    from types import SimpleNamespace
    from noisediff_amd import NoiseDiffNet
    from noisediff_amd import engine as E
    dim, B, H = 64, 2, 64
    net = NoiseDiffNet(SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False, mid_attn=False))
    net.load_state_dict(state_dict(dim), strict=True)
    eng = net.to(DEV).eval().hip_engine(DEV)
    cond = {k: (v if k == "iso_ratio_idx" else v.to(DEV)) for k, v in synth.make_condition(B, H, seed=1).items()}
    x, t = synth.make_noise(2, "net.x", B, 4, H).to(DEV), torch.tensor([17, 640])
    monkeypatch.setattr(E, "FOLD_ATTN", True)
    monkeypatch.setattr(E, "DOWN_FAST", True)
    fast = eng.plan(B, H, H)
    fast.set_condition(cond)
    y_f = fast.forward(x, t).cpu()
    dbg = eng.plan(B, H, H, debug=True)
    monkeypatch.setattr(E, "FOLD_ATTN", False)
    monkeypatch.setattr(E, "DOWN_FAST", False)
    plain = eng.plan(B, H, H, tag=1)
    plain.set_condition(cond)
    y_u = plain.forward(x, t).cpu()
    assert torch.isfinite(y_f).all() and float(y_f.abs().max()) > 1e-3
    assert close(y_f.numpy(), y_u.numpy(), NET_TOL)
    nf, nu, nd = _names(fast), _names(plain), _names(dbg)
    layers = lambda plan: [str(op[3].get("layer", "")) for op in plan.step_ops if op[3]]
    assert "nd_pointwise_downsample_nhwc_f32" not in nu and not any(n.endswith(".tail_fold") for n in layers(plain)) and not plain.cbf
    assert sum(n.endswith(".2.proj_out") for n in layers(plain)) == 5 and sum(n.endswith(".2.ff.net.2") for n in layers(plain)) == 5
    assert [n for n in layers(dbg) if n.endswith(".tail_fold")] == [n for n in layers(fast) if n.endswith(".tail_fold")] and "downs.2.2" in dbg.taps
    assert nd.count("nd_pointwise_downsample_nhwc_f32") == 3
    assert len(nu) - len(nf) == 5
    assert nf.count("nd_pointwise_downsample_nhwc_f32") == 3
    folded = [op[3]["layer"] for op in fast.step_ops if op[3] and str(op[3].get("layer", "")).endswith(".tail_fold")]
    assert folded == [f"{n}.tail_fold" for n in ("downs.2.2", "downs.3.2", "ups.0.2", "ups.1.2", "ups.2.2")]
    assert len(plain.cond_ops) + 5 == len(fast.cond_ops)                       # the per-sample vectors are formed with the condition, not per step
