"""Training the attention modules on the HIP library (noisediff_amd/csrc/attn_train.hip, train.attention_core / linear_attention_core / rms_norm):
every forward and gradient against the reference's own formulas (models/attend.py:101-116, models/archs/Diffusion_arch.py:84-90, 218-235) restated here in
float64 on the CPU under autograd, at the smallest shapes where each kernel can go wrong; the raw C ABI with padded rows; bitwise repeatability,
independence of a sample from its batch, graph capture, and the wiring in TrainableNoiseDiffNet.

Bound: util.derived -- kernel error <= 4 x the error of the same formula in fp32 torch on the CPU + one ulp of the scale."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from noisediff_amd import GaussianDiffusion, TrainableNoiseDiffNet, synth, train, trainable
from noisediff_amd import _lib as L
from util import derived, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DH = 32
CL = torch.channels_last


# ---- the reference, restated ------------------------------------------------------------------------------------------------------------
def _full_formula(qkv, heads):
    """Attention.forward's core with Attend's explicit path (Diffusion_arch.py:260-265, attend.py:101-116)."""
    b, _, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, DH, h * w).transpose(-1, -2) for t in qkv.chunk(3, dim=1))          # b h (x y) c
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * (DH ** -0.5)
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
    return out.transpose(-1, -2).reshape(b, heads * DH, h, w)


def _linear_formula(qkv, heads):
    """LinearAttention.forward's core (Diffusion_arch.py:223-234)."""
    b, _, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, DH, h * w) for t in qkv.chunk(3, dim=1))                            # b h c (x y)
    q = q.softmax(dim=-2)
    k = k.softmax(dim=-1)
    q = q * (DH ** -0.5)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", context, q).reshape(b, heads * DH, h, w)


def _rms_formula(x, g, res=None):
    """RMSNorm.forward (Diffusion_arch.py:89-90) (+ the residual of the per-stage wiring)."""
    y = F.normalize(x, dim=1) * g * (x.shape[1] ** 0.5)
    return y if res is None else y + res


def _core_reference(formula, qkv, dout, heads, dtype):
    x = qkv.detach().to(dtype, copy=True).requires_grad_(True)            # (a copy: the cached inputs stay plain tensors, so what the GPU runs on is a leaf)
    out = formula(x, heads)
    (g,) = torch.autograd.grad(out, x, dout.to(dtype))
    return (out.detach(),) + tuple(g.chunk(3, dim=1))


FORMULA = {"full": _full_formula, "linear": _linear_formula}
CORE = {"full": train.attention_core, "linear": train.linear_attention_core}


@functools.lru_cache(maxsize=None)
def _core_case(kind, shape, boost):
    """(qkv, dout, float64 reference, fp32 reference) of one case, computed once; ``boost``: the factor on q (full) or on q and k (linear)."""
    B, heads, H, W = shape
    hid = heads * DH
    qkv = synth.normal(11, f"attn_train.{kind}.qkv.{shape}", (B, 3 * hid, H, W))
    dout = synth.normal(11, f"attn_train.{kind}.dout.{shape}", (B, hid, H, W))
    if boost != 1:
        qkv = qkv.clone()
        qkv[:, :hid if kind == "full" else 2 * hid] *= boost
    return qkv, dout, _core_reference(FORMULA[kind], qkv, dout, heads, torch.float64), _core_reference(FORMULA[kind], qkv, dout, heads, torch.float32)


def _run_core(kind, qkv, dout, heads):
    """(out, dq, dk, dv) of the library operator, on the CPU."""
    x = qkv.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    out = CORE[kind](x, heads)
    (g,) = torch.autograd.grad(out, x, dout.to(DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    return (out.detach().cpu(),) + tuple(g.cpu().chunk(3, dim=1))


def _check_core(kind, shape, boost):
    qkv, dout, ref64, ref32 = _core_case(kind, shape, boost)
    got = _run_core(kind, qkv, dout, shape[1])
    for name, a, r64, r32 in zip(("out", "dq", "dk", "dv"), got, ref64, ref32):
        assert a.shape == r64.shape
        derived(a, r64, r32, f"{kind} attention {shape} x{boost}: {name}")


# (B, heads, H, W): N = 16 below one key tile; 64 one key tile; 100 partial key and query tiles; 129 one query in the second 128-query group, one head;
# 160; 1024 config 4's own mid-block shape -- and the peaked set (q x 8) at N = 100 and 1024
FULL_CASES = [((1, 4, 4, 4), 1), ((2, 4, 8, 8), 1), ((2, 4, 10, 10), 1), ((1, 1, 3, 43), 1), ((1, 4, 10, 16), 1), ((2, 4, 32, 32), 1),
              ((2, 4, 10, 10), 8), ((2, 4, 32, 32), 8)]
# N = 16; 100; 2048 one context chunk exactly; 2304 a partial second chunk; 65536 stage 0 of a 256 x 256 step -- and q, k x 4 at N = 100 and 2304
LINEAR_CASES = [((1, 4, 4, 4), 1), ((2, 4, 10, 10), 1), ((2, 4, 32, 64), 1), ((2, 4, 48, 48), 1), ((1, 4, 256, 256), 1),
                ((2, 4, 10, 10), 4), ((2, 4, 48, 48), 4)]


@pytest.mark.parametrize("shape,boost", FULL_CASES)
def test_full_attention_forward_and_gradients_equal_float64_autograd(shape, boost):
    _check_core("full", shape, boost)


@pytest.mark.parametrize("shape,boost", LINEAR_CASES)
def test_linear_attention_forward_and_gradients_equal_float64_autograd(shape, boost):
    _check_core("linear", shape, boost)


# ---- RMSNorm ----------------------------------------------------------------------------------------------------------------------------
def _rms_inputs(tokens, Cc, zero_pixel):
    x = synth.normal(12, f"attn_train.rms.x.{tokens}.{Cc}", (2, Cc, tokens // 2, 1))
    if zero_pixel:
        x = x.clone()
        x[1, :, 3, 0] = 0.0
    g = 1.0 + 0.25 * synth.normal(12, f"attn_train.rms.g.{Cc}", (1, Cc, 1, 1))
    res = synth.normal(12, f"attn_train.rms.res.{tokens}.{Cc}", tuple(x.shape))
    dy = synth.normal(12, f"attn_train.rms.dy.{tokens}.{Cc}", tuple(x.shape))
    return x, g, res, dy


def _rms_reference(x, g, res, dy, dtype):
    x, g = x.to(dtype, copy=True).requires_grad_(True), g.to(dtype, copy=True).requires_grad_(True)
    r = None if res is None else res.to(dtype, copy=True).requires_grad_(True)
    y = _rms_formula(x, g, r)
    grads = torch.autograd.grad(y, (x, g) if r is None else (x, g, r), dy.to(dtype))
    return (y.detach(),) + tuple(grads)


def _rms_run(x, g, res, dy):
    xd, gd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True), g.to(DEV).requires_grad_(True)
    rd = None if res is None else res.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    y = train.rms_norm(xd, gd, rd)
    dyd = dy.to(DEV).contiguous(memory_format=CL)
    grads = torch.autograd.grad(y, (xd, gd) if rd is None else (xd, gd, rd), dyd)
    torch.cuda.synchronize()
    if rd is not None:
        assert torch.equal(grads[2], dyd)                                    # the residual's gradient is dy itself
    return (y.detach().cpu(),) + tuple(t.cpu() for t in grads)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("tokens,Cc,zero_pixel", [(16, 16, False), (200, 64, False), (4096, 128, False), (2048, 1024, False), (200, 64, True)])
def test_rms_norm_forward_and_gradients_equal_float64_autograd(tokens, Cc, zero_pixel, with_res):
    """``zero_pixel``: one pixel is all zeros -- the clamp of F.normalize makes its norm a constant; the gradient must be finite and autograd's."""
    x, g, res, dy = _rms_inputs(tokens, Cc, zero_pixel)
    res = res if with_res else None
    ref64, ref32 = _rms_reference(x, g, res, dy, torch.float64), _rms_reference(x, g, res, dy, torch.float32)
    got = _rms_run(x, g, res, dy)
    for name, a, r64, r32 in zip(("y", "dx", "dg", "dres"), got, ref64, ref32):
        assert a.shape == r64.shape
        derived(a, r64, r32, f"rms_norm ({tokens}, {Cc}) zero={zero_pixel} res={with_res}: {name}")
    if zero_pixel:           # the clamped pixel's dx (~1e13) sets the scale of the bound above: the other pixels once more, on their own scale
        keep = torch.ones(x.shape[0], 1, x.shape[2], 1, dtype=torch.bool)
        keep[1, :, 3, 0] = False
        rest = lambda t: t.masked_select(keep)
        derived(rest(got[1]), rest(ref64[1]), rest(ref32[1]), f"rms_norm ({tokens}, {Cc}) zero={zero_pixel} res={with_res}: dx without the zero pixel")


# ---- the raw C ABI ------------------------------------------------------------------------------------------------------------------------
POISON = 12345.0


def _padded(t_nchw, ld):
    """NHWC rows of ``ld`` floats on the GPU: the tensor's channels, then poison."""
    B, Cc, H, W = t_nchw.shape
    buf = torch.full((B, H * W, ld), POISON, device=DEV)
    buf[:, :, :Cc] = t_nchw.permute(0, 2, 3, 1).reshape(B, H * W, Cc).to(DEV)
    return buf


def _unpad(buf, Cc, B, H, W):
    assert bool((buf[:, :, Cc:] == POISON).all()), "the padding of a row was written"
    return buf[:, :, :Cc].reshape(B, H, W, Cc).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("kind", ["full", "linear"])
@pytest.mark.parametrize("shape", [(2, 4, 10, 10), (2, 4, 32, 32)])
def test_c_abi_with_padded_rows_leaves_the_padding_and_equals_the_operator(kind, shape):
    """ld_qkv = 3 hid + 16, ld_out = hid + 8, ld_dqkv = 3 hid + 16 with poisoned padding: the padding comes back unchanged, all 3 hid channels of every token
    are written, and the results are the bits of the train.* operator on dense rows; nd_attention_train_forward_f32's out is nd_attention_mfma_f32's."""
    import hiputil
    ctx = hiputil.Ctx()
    B, heads, H, W = shape
    hid, N = heads * DH, H * W
    qkv, dout, _, _ = _core_case(kind, shape, 1)
    want = _run_core(kind, qkv, dout, heads)
    ldq, ldo = 3 * hid + 16, hid + 8
    qb, gb = _padded(qkv, ldq), _padded(dout, ldo)
    ob = torch.full((B, N, ldo), POISON, device=DEV)
    db = torch.full((B, N, ldq), POISON, device=DEV)
    torch.cuda.synchronize()
    if kind == "full":
        lse = torch.empty((B, heads, N), device=DEV)
        ws = torch.empty(int(ctx.lib.nd_attention_backward_workspace_floats(B, N, heads)), device=DEV)
        L.call("nd_attention_train_forward_f32", qb.data_ptr(), ldq, ob.data_ptr(), ldo, lse.data_ptr(), B, N, heads, DH, ctx.stream)
        L.call("nd_attention_backward_f32", qb.data_ptr(), ldq, ob.data_ptr(), ldo, gb.data_ptr(), ldo, lse.data_ptr(), db.data_ptr(), ldq, ws.data_ptr(),
               B, N, heads, DH, ctx.stream)
        ob2 = torch.full((B, N, ldo), POISON, device=DEV)
        torch.cuda.synchronize()
        L.call("nd_attention_mfma_f32", qb.data_ptr(), ldq, ob2.data_ptr(), ldo, B, N, heads, DH, ctx.stream)
        ctx.sync()
        assert torch.equal(ob, ob2), "the training forward's out is not the inference entry's"
    else:
        fws = torch.empty(int(ctx.lib.nd_linear_attention_workspace_floats(B, N, heads)), device=DEV)
        ws = torch.empty(int(ctx.lib.nd_linear_attention_backward_workspace_floats(B, N, heads)), device=DEV)
        L.call("nd_linear_attention_f32", qb.data_ptr(), ldq, ob.data_ptr(), ldo, fws.data_ptr(), B, N, heads, DH, ctx.stream)
        L.call("nd_linear_attention_backward_f32", qb.data_ptr(), ldq, gb.data_ptr(), ldo, fws.data_ptr(), db.data_ptr(), ldq, ws.data_ptr(),
               B, N, heads, DH, ctx.stream)
    ctx.sync()
    assert torch.equal(qb[:, :, 3 * hid:], torch.full_like(qb[:, :, 3 * hid:], POISON))
    out = _unpad(ob, hid, B, H, W)
    dq, dk, dv = _unpad(db, 3 * hid, B, H, W).chunk(3, dim=1)
    for name, a, b in zip(("out", "dq", "dk", "dv"), (out, dq, dk, dv), want):
        assert torch.isfinite(a).all() and torch.equal(a, b), name


def test_c_abi_refuses_a_head_width_other_than_32():
    import hiputil
    ctx = hiputil.Ctx()
    B, N, heads, dh = 1, 16, 8, 16                                             # the same 384 / 128 floats per row
    hid = heads * dh
    qb, ob, gb, db = (torch.zeros((B, N, c), device=DEV) for c in (3 * hid, hid, hid, 3 * hid))
    lse, ws = torch.zeros((B, heads, N), device=DEV), torch.zeros(1 << 16, device=DEV)
    torch.cuda.synchronize()
    lib = ctx.lib
    assert lib.nd_attention_train_forward_f32(qb.data_ptr(), 3 * hid, ob.data_ptr(), hid, lse.data_ptr(), B, N, heads, dh, ctx.stream) == -2      # ND_E_SHAPE
    assert lib.nd_attention_backward_f32(qb.data_ptr(), 3 * hid, ob.data_ptr(), hid, gb.data_ptr(), hid, lse.data_ptr(), db.data_ptr(), 3 * hid, ws.data_ptr(),
                                         B, N, heads, dh, ctx.stream) == -2
    assert lib.nd_linear_attention_backward_f32(qb.data_ptr(), 3 * hid, gb.data_ptr(), hid, ws.data_ptr(), db.data_ptr(), 3 * hid, ws.data_ptr(),
                                                B, N, heads, dh, ctx.stream) == -2
    with pytest.raises(ValueError):
        train.attention_core(torch.zeros((1, 3 * 4 * 16, 4, 4), device=DEV), heads=4)
    ctx.sync()


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("full", (2, 4, 10, 10)), ("full", (2, 4, 32, 32)), ("linear", (2, 4, 10, 10)), ("linear", (2, 4, 48, 48))])
def test_cores_are_bitwise_repeatable_and_a_sample_does_not_depend_on_its_batch(kind, shape):
    qkv, dout, _, _ = _core_case(kind, shape, 1)
    a = _run_core(kind, qkv, dout, shape[1])
    b = _run_core(kind, qkv, dout, shape[1])
    alone = _run_core(kind, qkv[1:], dout[1:], shape[1])
    for name, x, y, z in zip(("out", "dq", "dk", "dv"), a, b, alone):
        assert torch.equal(x, y), f"{name}: two calls differ"
        assert torch.equal(x[1:], z), f"{name}: the second sample of the batch is not the sample alone"


def test_rms_norm_is_bitwise_repeatable():
    x, g, res, dy = _rms_inputs(4096, 128, False)
    a, b = _rms_run(x, g, res, dy), _rms_run(x, g, res, dy)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "linear"])
def test_forward_and_backward_replay_from_one_captured_graph(kind):
    """Forward and backward at N = 100 captured in one torch.cuda.graph (after a warm-up on a side stream) and replayed equal the eager result bitwise.
    The gradient accumulates into the leaf's ``.grad`` through ``backward()``, as a training step's does."""
    shape = (2, 4, 10, 10)
    qkv, dout, _, _ = _core_case(kind, shape, 1)
    x = qkv.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    gd = dout.to(DEV).contiguous(memory_format=CL)
    assert x.is_leaf

    def step():
        x.grad = None
        out = CORE[kind](x, shape[1])
        out.backward(gd)
        return out.detach()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            want_out = step().clone()
        want_grad = x.grad.clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        got_out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_out, want_out) and torch.equal(x.grad, want_grad)


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,expected", [(dict(mid_attn=True), dict(attention_core=1, rms_norm=1, linear_attention_core=0)),
                                         (dict(stage_attn=True), dict(attention_core=2, rms_norm=14, linear_attention_core=6))])
def test_the_attention_modules_of_a_hip_network_run_on_the_library(monkeypatch, kw, expected):
    """One forward + backward of TrainableNoiseDiffNet(dim=16, mid_attn / stage_attn).hip() on a 32 x 32 batch of 2: the three operators are called the
    expected number of times, neither F.scaled_dot_product_attention nor F.normalize is, FALLBACKS stays free of attention / RMSNorm entries, and the
    loss is the PyTorch path's."""
    Bn, Hn = 2, 32
    x0 = synth.uniform(5, "train.x0", (Bn, 4, Hn, Hn), -1.0, 1.0).to(DEV)
    noise = synth.make_noise(5, "train.noise", Bn, 4, Hn).to(DEV)
    t = torch.tensor([3, 777], dtype=torch.long, device=DEV)
    cond = {k: (v if k == "iso_ratio_idx" else v.to(DEV)) for k, v in synth.make_condition(Bn, Hn, seed=1).items()}
    net = TrainableNoiseDiffNet(SimpleNamespace(dim=16, **kw)).to(DEV).train()
    gd = GaussianDiffusion(net, image_size=Hn, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(DEV)
    net.hip(False)
    with torch.no_grad():
        want = float(gd.p_losses(x0, t, cond, noise=noise.clone()))

    def refuse(*a, **k):
        raise AssertionError("a PyTorch attention / normalize op ran in a .hip() network")

    monkeypatch.setattr(F, "scaled_dot_product_attention", refuse)
    monkeypatch.setattr(F, "normalize", refuse)
    counts = {}
    for name in expected:
        def counted(*a, _fn=getattr(train, name), _name=name, **k):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(train, name, counted)
    trainable.FALLBACKS.clear()
    net.hip()
    loss = gd.p_losses(x0, t, cond, noise=noise.clone())
    loss.backward()
    torch.cuda.synchronize()
    assert {k: counts.get(k, 0) for k in expected} == expected
    assert not [k for k in trainable.FALLBACKS if k[1] in ("attention", "linear_attention", "rms_norm")], trainable.FALLBACKS
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in net.named_parameters()
               if n.startswith(("mid_attn.", "down_attns.", "up_attns.")))
    assert rel_err(float(loss.detach()), want) < 2e-4
