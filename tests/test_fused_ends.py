"""The step's two full-resolution block tails folded into their per-pixel consumers:

  * nd_pointwise_narrow_fold_nhwc_f32 -- final_conv(res_conv(cat(xp, x0)) + silu(GN(c2))) + shot as one narrow dot product with the folded weight
    [Wf Wr | Wf] (nd_pack_narrow_fold: the mid-term sums in fp64, rounded once);
  * nd_pointwise_chain_tail_split_nhwc_f32 -- shot_mlp3(shot_time(s2) + r) with the ResnetBlock tail as the split chain's prologue;
  * the plans that record them (engine.FOLD_FINAL / engine.SHOT_TAIL), against the same plans with both knobs off.

References are float64 on the CPU; the bounds are tests/util.py's ``derived`` (4 x the error of the unfused formula in fp32 torch + one ulp) and ``close``."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from noisediff_amd import _lib as L
from noisediff_amd import synth
from util import close, derived, state_dict

TOL = 2e-5
NET_TOL = 2e-4
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(31, name, shape, lo, hi)


def _strided(t, ld):
    """Device copy of (rows..., C) with pixel stride ld >= C; the pad columns hold NaN (a kernel that reads them poisons its output)."""
    import hiputil as hu
    buf = torch.full(t.shape[:-1] + (ld,), float("nan"))
    buf[..., :t.shape[-1]] = t
    return hu.dev(buf)


def _canary_out(B, HW, cout, ldo, extra_rows=3):
    """NaN-filled output of B * HW + extra_rows rows x ldo columns: the kernel may write [:B * HW, :cout] and nothing else."""
    import hiputil as hu
    return hu.full((B * HW + extra_rows, ldo))


def _check_canary(buf, rows, cout):
    got = buf.cpu()
    assert torch.isnan(got[rows:]).all() and torch.isnan(got[:rows, cout:]).all(), "the kernel wrote outside its output"
    return got[:rows, :cout]


def _mad(name, B, Cc):
    """Distinct M | A | D per sample, [B][3][C] as nd_groupnorm_finalize_f32 writes it."""
    return torch.stack((U(name + ".M", (B, Cc), -0.5, 0.5), U(name + ".A", (B, Cc), 0.5, 1.5), U(name + ".D", (B, Cc), -0.5, 0.5)), 1).contiguous()


def _affine_silu(t, mad):
    return F.silu((t - mad[:, None, 0]) * mad[:, None, 1] + mad[:, None, 2])


# ====================================================================================================== 1. the folded narrow kernel
def _fold(ctx, wf, bf, wr, br):
    """nd_pack_narrow_fold on the device -> (weight [cin/4][cout][4], bias [cout]) device tensors."""
    import hiputil as hu
    cout, mid = wf.shape
    cin_r = wr.shape[1]
    n = ctx.lib.nd_pack_narrow_fold_floats(cin_r + mid, cout)
    assert n == (cin_r + mid) * cout
    wp, bp = hu.full((n + 8,)), hu.full((cout + 4,))
    keep = [hu.dev(wf), hu.dev(bf), hu.dev(wr), hu.dev(br)]
    L.call("nd_pack_narrow_fold", keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), wp.data_ptr(), bp.data_ptr(),
           cin_r, mid, cout, ctx.stream)
    ctx.sync()
    assert torch.isnan(wp[n:]).all() and torch.isnan(bp[cout:]).all()
    return wp, bp


@pytest.mark.parametrize("cout", [4, 8])
@pytest.mark.parametrize("d", [16, 48, 64])
def test_narrow_fold_weights_are_the_fp64_product_rounded_once(ctx, d, cout):
    wf, bf = U(f"fold.wf.{d}.{cout}", (cout, d), -0.3, 0.3), U(f"fold.bf.{cout}", (cout,))
    wr, br = U(f"fold.wr.{d}", (d, 2 * d), -0.3, 0.3), U(f"fold.br.{d}", (d,))
    wp, bp = _fold(ctx, wf, bf, wr, br)
    n = 3 * d * cout
    got_w = wp[:n].cpu().view(3 * d // 4, cout, 4).permute(1, 0, 2).reshape(cout, 3 * d)       # [cin/4][cout][4] -> (cout, cin)
    ref_w = torch.cat(((wf.double() @ wr.double()).float(), wf), 1)
    ref_b = (wf.double() @ br.double() + bf.double()).float()
    assert torch.equal(got_w, ref_w)
    assert torch.equal(bp[:cout].cpu(), ref_b)


@pytest.mark.parametrize("cout", [4, 8])
@pytest.mark.parametrize("d", [16, 48, 64])
def test_narrow_fold_matches_the_unfolded_layers_in_float64(ctx, d, cout):
    """B = 3, HW = 185: 555 pixels, a ragged last block; distinct M | A | D per sample; with and without res0; strides wider than the channel counts; a repeated
    launch is bitwise equal.  Reference: the UNFOLDED formula in float64; bound: the two-layer formula in fp32 torch (``derived``)."""
    import hiputil as hu
    B, HW = 3, 185
    xp, x0, t = U(f"nf.xp.{d}", (B, HW, d), -1.5, 1.5), U(f"nf.x0.{d}", (B, HW, d), -1.5, 1.5), U(f"nf.t.{d}", (B, HW, d), -2, 2)
    mad = _mad(f"nf.mad.{d}", B, d)
    wf, bf = U(f"fold.wf.{d}.{cout}", (cout, d), -0.3, 0.3), U(f"fold.bf.{cout}", (cout,))
    wr, br = U(f"fold.wr.{d}", (d, 2 * d), -0.3, 0.3), U(f"fold.br.{d}", (d,))
    res = U(f"nf.res.{cout}", (B, HW, cout))
    wp, bp = _fold(ctx, wf, bf, wr, br)

    def formula(dt):
        c = lambda v: v.to(dt)
        xf = F.linear(torch.cat((c(xp), c(x0)), -1), c(wr), c(br)) + _affine_silu(c(t), c(mad))
        return F.linear(xf, c(wf), c(bf))
    ref64, ref32 = formula(torch.float64), formula(torch.float32)
    for ld_pad, with_res in ((0, False), (0, True), (4, True)):
        srcs = [_strided(v, d + ld_pad) for v in (xp, x0, t)]
        rd = _strided(res, cout + ld_pad) if with_res else None
        ldo = cout + 4
        out = _canary_out(B, HW, cout, ldo)
        nf = L.NarrowFold()
        madd = hu.dev(mad)
        nf.p0, nf.p1, nf.t, nf.mad = srcs[0].data_ptr(), srcs[1].data_ptr(), srcs[2].data_ptr(), madd.data_ptr()
        nf.weight, nf.bias, nf.out = wp.data_ptr(), bp.data_ptr(), out.data_ptr()
        nf.B, nf.HW, nf.c0, nf.c1, nf.c2, nf.ld0, nf.ld1, nf.ldt, nf.cout, nf.ldo = B, HW, d, d, d, d + ld_pad, d + ld_pad, d + ld_pad, cout, ldo
        if with_res:
            nf.res0, nf.ldr0 = rd.data_ptr(), cout + ld_pad
        L.call("nd_pointwise_narrow_fold_nhwc_f32", C.byref(nf), ctx.stream)
        ctx.sync()
        got = _check_canary(out, B * HW, cout).view(B, HW, cout)
        add64, add32 = (res.double(), res) if with_res else (0.0, 0.0)
        assert derived(got, ref64 + add64, ref32 + add32, f"narrow fold d={d} cout={cout} pad={ld_pad} res={with_res}")
        first = out.clone()
        torch.cuda.synchronize()
        L.call("nd_pointwise_narrow_fold_nhwc_f32", C.byref(nf), ctx.stream)
        ctx.sync()
        assert torch.equal(out[:B * HW, :cout], first[:B * HW, :cout])
    # shapes the kernel does not take are refused, not approximated
    assert not ctx.lib.nd_pointwise_narrow_fold_takes(d, d, d, 16) and not ctx.lib.nd_pointwise_narrow_fold_takes(d, d, d + 2, cout)
    nf.cout = 16
    assert ctx.lib.nd_pointwise_narrow_fold_nhwc_f32(C.byref(nf), ctx.stream) != 0
    assert b"not a shape" in ctx.lib.nd_last_error()


# ====================================================================================================== 2. the chain's tail prologue
def _chain_desc(ctx, case, widths, keep):
    import hiputil as hu
    ws = [U(f"{case}.w{i}", (widths[i + 1], widths[i]), -0.3, 0.3) for i in range(2)]
    bs = [U(f"{case}.b{i}", (widths[i + 1],)) for i in range(2)]
    d = L.Chain()
    for i in range(2):
        wd = hu.dev(ws[i])
        wp = hu.full((ctx.lib.nd_pack_chain_weight_split_floats(widths[i], widths[i + 1], int(i == 0)),))
        L.call("nd_pack_chain_weight_split", wd.data_ptr(), wp.data_ptr(), widths[i], widths[i + 1], int(i == 0), ctx.stream)
        bd = hu.dev(bs[i])
        keep += [wd, wp, bd]
        d.st[i].weight, d.st[i].bias, d.st[i].cin, d.st[i].cout = wp.data_ptr(), bd.data_ptr(), widths[i], widths[i + 1]
    d.st[0].act = L.ACT_GELU
    ctx.sync()
    return d, ws, bs


@pytest.mark.parametrize("with_r1", [True, False])
@pytest.mark.parametrize("widths", [[64, 64, 4], [48, 48, 4]])
def test_chain_tail_prologue_matches_float64_and_the_two_launches(ctx, widths, with_r1):
    """B = 3, HW = 96: three 32-pixel tiles per sample, nine in all: on any part with two or more CUs every wave holds at most one tile, so each stashes M | A | D once (a wave
    that crosses a sample boundary and reloads the stash: tests/test_pointwise_float64.py, the chain's second trip); inputs in +-2.  References:
    fc2(gelu(fc1(silu(affine(t)) + r0 + r1))) in float64, and nd_affine_silu_add_f32 followed by the split chain on the same inputs."""
    import hiputil as hu
    B, HW, Cc = 3, 96, widths[0]
    case = f"ct.{Cc}"
    t, r0, r1 = U(case + ".t", (B, HW, Cc), -2, 2), U(case + ".r0", (B, HW, Cc), -2, 2), U(case + ".r1", (B, HW, Cc), -2, 2)
    mad = _mad(case + ".mad", B, Cc)
    keep = []
    d, ws, bs = _chain_desc(ctx, case, widths, keep)
    row64 = _affine_silu(t.double(), mad.double()) + r0.double() + (r1.double() if with_r1 else 0.0)
    ref64 = F.linear(F.gelu(F.linear(row64, ws[0].double(), bs[0].double())), ws[1].double(), bs[1].double())
    td, r0d, r1d, madd = _strided(t, Cc + 4), _strided(r0, Cc + 8), _strided(r1, Cc) if with_r1 else None, hu.dev(mad)
    ldo = widths[-1] + 4
    out = _canary_out(B, HW, widths[-1], ldo)
    d.src = hu.src(td)
    d.src.c0, d.src.ld0 = Cc, Cc + 4
    d.out, d.n_stages, d.B, d.HW, d.ldo = out.data_ptr(), 2, B, HW, ldo
    dt = L.ChainTail()
    dt.chain, dt.mad, dt.r0, dt.ldr0 = d, madd.data_ptr(), r0d.data_ptr(), Cc + 8
    if with_r1:
        dt.r1, dt.ldr1 = r1d.data_ptr(), Cc
    L.call("nd_pointwise_chain_tail_split_nhwc_f32", C.byref(dt), ctx.stream)
    ctx.sync()
    got = _check_canary(out, B * HW, widths[-1]).view(B, HW, widths[-1])
    assert close(got.numpy(), ref64.numpy(), TOL)
    first = out.clone()
    torch.cuda.synchronize()
    L.call("nd_pointwise_chain_tail_split_nhwc_f32", C.byref(dt), ctx.stream)
    ctx.sync()
    assert torch.equal(out[:B * HW, :widths[-1]], first[:B * HW, :widths[-1]])
    # the two launches it replaces, on the same inputs
    s3 = hu.full((B, HW, Cc))
    L.call("nd_affine_silu_add_f32", td.data_ptr(), Cc + 4, madd.data_ptr(), r0d.data_ptr(), Cc + 8, r1d.data_ptr() if with_r1 else None, Cc, s3.data_ptr(), Cc,
           B, HW, Cc, ctx.stream)
    out2 = hu.full((B, HW, widths[-1]))
    d2 = L.Chain.from_buffer_copy(d)
    d2.src = hu.src(s3)
    d2.out, d2.ldo = out2.data_ptr(), widths[-1]
    L.call("nd_pointwise_chain_split_nhwc_f32", C.byref(d2), ctx.stream)
    ctx.sync()
    assert close(out2.cpu().numpy(), ref64.numpy(), TOL)
    assert close(got.numpy(), out2.cpu().double().numpy(), TOL)


def test_chain_tail_refuses_widths_it_does_not_instantiate(ctx):
    import hiputil as hu
    B, HW, widths = 2, 32, [32, 32, 4]
    assert not ctx.lib.nd_pointwise_chain_tail_takes(32, 32, 4, 0) and not ctx.lib.nd_pointwise_chain_tail_takes(64, 128, 64, 64)
    assert ctx.lib.nd_pointwise_chain_tail_takes(64, 64, 4, 0) and ctx.lib.nd_pointwise_chain_tail_takes(48, 48, 4, 0)
    keep = []
    d, _, _ = _chain_desc(ctx, "ct.refuse", widths, keep)
    t, r0, mad, out = hu.dev(U("ct.refuse.t", (B, HW, 32))), hu.dev(U("ct.refuse.r", (B, HW, 32))), hu.dev(_mad("ct.refuse.mad", B, 32)), hu.full((B, HW, 4))
    d.src = hu.src(t)
    d.out, d.n_stages, d.B, d.HW, d.ldo = out.data_ptr(), 2, B, HW, 4
    dt = L.ChainTail()
    dt.chain, dt.mad, dt.r0, dt.ldr0 = d, mad.data_ptr(), r0.data_ptr(), 32
    assert ctx.lib.nd_pointwise_chain_tail_split_nhwc_f32(C.byref(dt), ctx.stream) != 0
    assert b"not instantiated" in ctx.lib.nd_last_error()
    ctx.sync()
    assert torch.isnan(out).all()


# ====================================================================================================== 3. the plans
def _make_net(dim):
    from types import SimpleNamespace
    from noisediff_amd import NoiseDiffNet
    net = NoiseDiffNet(SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False, mid_attn=False))
    net.load_state_dict(state_dict(dim), strict=True)
    return net.to(DEV).eval()


def _to_dev(cond):
    return {k: (v if k == "iso_ratio_idx" else v.to(DEV)) for k, v in cond.items()}


def _names(plan):
    return [op[2] for op in plan.step_ops]


FUSED = ("nd_pointwise_narrow_fold_nhwc_f32", "nd_pointwise_chain_tail_split_nhwc_f32")


@pytest.mark.parametrize("dim", [16, 64])
def test_fused_plan_equals_the_unfused_plan_and_debug_plans_keep_every_tap(dim, monkeypatch):
    """32 x 32, B = 2: the fused plan against the same plan with both knobs off (NET_TOL); the recorded launches differ as expected (one launch fewer per end: at d = 64
    both ends, at d = 16 the trunk's -- the chain prologue has no 16-wide instance); a debug plan records the unfused launches and all taps."""
    from noisediff_amd import engine as E
    B, H = 2, 32
    net = _make_net(dim)
    eng = net.hip_engine(DEV)
    cond = _to_dev(synth.make_condition(B, H, seed=1))
    x, t = synth.make_noise(2, "net.x", B, 4, H).to(DEV), torch.tensor([17, 640])
    fused = eng.plan(B, H, H)
    fused.set_condition(cond)
    y_f = fused.forward(x, t).cpu()
    dbg = eng.plan(B, H, H, debug=True)
    monkeypatch.setattr(E, "FOLD_FINAL", False)
    monkeypatch.setattr(E, "SHOT_TAIL", False)
    plain = eng.plan(B, H, H, tag=1)
    plain.set_condition(cond)
    y_u = plain.forward(x, t).cpu()
    assert torch.isfinite(y_f).all() and float(y_f.abs().max()) > 1e-3
    assert close(y_f.numpy(), y_u.numpy(), NET_TOL)
    nf, nu, nd = _names(fused), _names(plain), _names(dbg)
    assert not any(n in FUSED for n in nu) and not any(n in FUSED for n in nd) and nd == nu
    assert nf.count(FUSED[0]) == 1 and nf.count(FUSED[1]) == (1 if dim == 64 else 0)
    assert len(nu) - len(nf) == (2 if dim == 64 else 1)
    assert nu.count("nd_affine_silu_add_f32") - nf.count("nd_affine_silu_add_f32") == (1 if dim == 64 else 0)
    assert nu.count("nd_pointwise_gemm_nhwc_f32") - nf.count("nd_pointwise_gemm_nhwc_f32") == 2
    for tap in ("shot_time", "final_res_block", "shot_noise", "pos_block2", "shot_mlp2"):
        assert tap in dbg.taps, tap
    # the layer each fused launch reports (what bench.py and the tools key on)
    metas = {op[2]: op[3] for op in fused.step_ops if op[2] in FUSED}
    for m in metas.values():
        assert {"layer", "B", "HW", "cin", "cout"} <= set(m) and m["B"] == B and m["HW"] == H * H


def test_fused_plan_graph_replay_equals_eager_and_a_sample_does_not_depend_on_its_batch():
    from noisediff_amd import GaussianDiffusion
    dim, B, H = 64, 2, 32
    net = _make_net(dim)
    gd = GaussianDiffusion(net, image_size=H, timesteps=6, beta_schedule="sigmoid2").to(DEV)
    cond = _to_dev(synth.make_condition(B, H, seed=1))
    ref = gd.sample(batch_size=B, condition=cond, seed=11).cpu()
    loop = next(iter(gd._loop_cache.values()))
    assert any(n in FUSED for n in _names(loop.plan))
    eager = loop.run(x_T=None, step_noise=None, seed=11, first_sample=0, use_graph=False).cpu()
    assert torch.equal(ref, eager)
    # rows 1..2 of a batch of 5 == the same two samples as a batch of their own, bit for bit
    cond5 = synth.make_condition(5, H, seed=1)
    x5, t5 = synth.make_noise(2, "net.x", 5, 4, H), torch.tensor([3, 321, 640, 999, 17])
    with torch.inference_mode():
        y5 = net(x5.to(DEV), t5.to(DEV), _to_dev(cond5)).cpu()
        y2 = net(x5[1:3].to(DEV), t5[1:3].to(DEV), _to_dev({k: v[1:3] for k, v in cond5.items()})).cpu()
    assert torch.equal(y5[1:3], y2)
