"""The two ends of a diffusion training step on the HIP library (noisediff_amd/csrc/diffusion_train.hip, train.diffusion_noising / diffusion_loss,
GaussianDiffusion.use_device_rng / hip_losses): the numpy restatement (tests/diffusion_train_ref.py) is pinned to the reference's golden values on the
CPU; the kernels are held to it on the GPU -- bit for bit where the contract says so, under util.derived for the fp64 sums.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from torch import nn

import diffusion_train_ref as R
from noisediff_amd import _lib as L, synth, train
from noisediff_amd.diffusion import GaussianDiffusion, make_betas, make_buffers
from util import derived

T = 1000
OBJECTIVES = ["pred_v", "pred_noise", "pred_x0"]
GB, GH = 2, 32                                  # the golden inputs: tests/test_training.py::_inputs()
SEED_T = 1                                      # under this seed the 65 536 draws below leave no timestep out (counts 40 .. 95, expected 65.5)
DRAW_SHAPES = [(1, 4, 2, 2), (3, 4, 24, 40), (2, 8, 8, 8)]


@functools.lru_cache(None)
def buffers(objective="pred_v"):
    return {k: v.numpy() for k, v in make_buffers(make_betas("sigmoid2", T), objective).items()}


def golden_inputs():
    return (synth.uniform(5, "train.x0", (GB, 4, GH, GH), -1.0, 1.0), synth.make_noise(5, "train.noise", GB, 4, GH), torch.tensor([3, 777], dtype=torch.long))


def schedule(objective="pred_v"):
    b = buffers(objective)
    return b["sqrt_alphas_cumprod"], b["sqrt_one_minus_alphas_cumprod"]


class PlugNet(nn.Module):
    """One 1x1 convolution with the reference's plug-in surface: three parameters (weight, bias, a gain on the timestep)."""
    channels = out_dim = 4
    self_condition = False
    random_or_learned_sinusoidal_cond = False

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.weight = nn.Parameter(torch.randn(4, 4, 1, 1, generator=g) * 0.5)
        self.bias = nn.Parameter(torch.randn(4, generator=g) * 0.1)
        self.tgain = nn.Parameter(torch.tensor(0.3))

    def forward(self, x, time, condition):
        y = torch.nn.functional.conv2d(x, self.weight, self.bias)
        return y * (1 + self.tgain * (time.to(x.dtype) / T))[:, None, None, None]


def plug_gd(objective="pred_v", size=16, **kw):
    net = PlugNet()
    return net, GaussianDiffusion(net, image_size=size, timesteps=T, beta_schedule="sigmoid2", objective=objective, **kw)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_restatement_matches_the_reference_noising_bit_for_bit(golden):
    x0, noise, t = golden_inputs()
    x_t, v = R.noising(x0.numpy(), noise.numpy(), None, t.numpy(), *schedule(), "pred_v")
    assert np.array_equal(x_t, golden("training", "train.x_t"))
    assert np.array_equal(v, golden("training", "train.v_target"))


@pytest.mark.parametrize("objective,strength,key", [("pred_v", 0.0, "train.loss.pred_v"), ("pred_noise", 0.0, "train.loss.pred_noise"),
                                                    ("pred_x0", 0.0, "train.loss.pred_x0"), ("pred_v", 0.1, "train.loss.pred_v.offset0.1")])
def test_restatement_matches_the_reference_losses(golden, objective, strength, key):
    from test_training import _gd, _inputs
    x0, noise, t, cond = _inputs()
    offset = synth.uniform(5, "train.offset", (GB, 4), -1.0, 1.0).numpy()
    b = buffers(objective)
    x_t, target = R.noising(x0.numpy(), noise.numpy(), offset, t.numpy(), b["sqrt_alphas_cumprod"], b["sqrt_one_minus_alphas_cumprod"], objective,
                            strength=strength)
    _, gd = _gd(objective)
    with torch.no_grad():
        out = gd.model(torch.from_numpy(x_t), t, cond).numpy()
    loss, sample = R.loss64(out, target, t.numpy(), b["loss_weight"], x0_term=objective == "pred_x0")
    assert float(loss) == pytest.approx(float(golden("training", key)), rel=2e-5)
    assert sample.shape == (GB,)


def test_restated_timestep_draw_is_in_range_exact_and_covers_every_timestep():
    n = 65536
    w = R.draw_t_words(SEED_T, np.arange(n), 0)
    t = R.draw_t(SEED_T, np.arange(n), 0, T)
    assert t.min() >= 0 and t.max() < T
    assert t.tolist() == [(int(x) * T) >> 32 for x in w.tolist()]            # floor(w T / 2^32) in exact integers
    assert np.bincount(t, minlength=T).min() >= 1
    assert not np.array_equal(t, R.draw_t(SEED_T, np.arange(n), 1, T))       # another draw, another stream


def test_use_device_rng_bookkeeping_on_a_cpu_wrapper(monkeypatch):
    _, gd = plug_gd()
    seen = []
    monkeypatch.setattr(gd, "p_losses", lambda *a, **k: seen.append(1) or torch.tensor(0.0))
    assert gd.train_rng is None
    gd(torch.zeros(1, 4, 16, 16), None)
    assert seen == [1]                                                       # unset: forward still reaches p_losses
    assert gd.use_device_rng(2 ** 64 - 3, first_sample=6, draw=9) is gd
    assert gd.train_rng.dtype == torch.int64 and gd.train_rng.tolist() == [-3, 6, 9]
    twin = copy.deepcopy(gd)
    twin.train_rng[2] = 100
    assert gd.train_rng.tolist() == [-3, 6, 9] and twin.train_rng.tolist() == [-3, 6, 100]
    assert "train_rng" in gd.__getstate__() and gd.__getstate__()["_loop_cache"] == {}
    with pytest.raises(L.HipError, match="no CPU path"):                     # no fallback once switched on
        gd(torch.zeros(1, 4, 16, 16), None)
    assert seen == [1]
    gd.use_device_rng(None)
    gd(torch.zeros(1, 4, 16, 16), None)
    assert seen == [1, 1] and gd.train_rng is None


# ---------------------------------------------------------------------------------------------------------------- GPU, through the C ABI
@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def abi_noising(ctx, x0, objective="pred_v", layout="nchw", auto=False, strength=0.0, seed=0, first=0, draw=0, noise=None, offset=None, t=None, rng=None,
                want_draws=True):
    """nd_diffusion_noising_f32 on CPU tensors (NCHW-shaped): dict of CPU results, the images back in NCHW."""
    import hiputil as hu
    B, Cc, H, W = x0.shape
    sa, sb = (hu.dev(torch.from_numpy(v)) for v in schedule(objective))
    p = L.DiffusionNoising()
    keep = [hu.dev(x0) if layout == "nchw" else hu.nhwc(x0), sa, sb]
    p.x0, p.sqrt_alphas_cumprod, p.sqrt_one_minus_alphas_cumprod = (k.data_ptr() for k in keep)
    for name, val in (("noise", None if noise is None else hu.nhwc(noise)), ("offset", None if offset is None else hu.dev(offset)),
                      ("t_in", None if t is None else hu.dev(t)), ("rng", None if rng is None else hu.dev(rng))):
        if val is not None:
            keep.append(val)
            setattr(p, name, val.data_ptr())
    out = {"t": hu._settle(torch.full((B,), -1, dtype=torch.int64, device=hu.DEV)), "x_t": hu.full((B, H, W, Cc)), "target": hu.full((B, H, W, Cc))}
    if want_draws:
        out["noise"], out["offset"] = hu.full((B, H, W, Cc)), hu.full((B, Cc))
        p.noise_out, p.offset_out = out["noise"].data_ptr(), out["offset"].data_ptr()
    p.t_out, p.x_t, p.target = out["t"].data_ptr(), out["x_t"].data_ptr(), out["target"].data_ptr()
    p.seed, p.first_sample, p.draw, p.offset_strength = seed, first, draw, strength
    p.B, p.C, p.H, p.W, p.T = B, Cc, H, W, T
    p.objective, p.auto_normalize, p.x0_channels_last = L.OBJECTIVES[objective], int(auto), int(layout != "nchw")
    L.call("nd_diffusion_noising_f32", C.byref(p), ctx.stream)
    ctx.sync()
    return {k: (hu.nchw(v) if v.dim() == 4 else v.cpu()) for k, v in out.items()}


def abi_loss(ctx, out, target, t, objective, g=None):
    """nd_diffusion_loss_f32 (and, with g, the backward) on CPU NCHW tensors: (loss, sample_loss, grad NCHW or None)."""
    import hiputil as hu
    B, Cc, H, W = out.shape
    x0_term = int(objective == "pred_x0")
    o, tg, td, lw = hu.nhwc(out), hu.nhwc(target), hu.dev(t), hu.dev(torch.from_numpy(buffers(objective)["loss_weight"]))
    nbytes = ctx.lib.nd_diffusion_loss_workspace_bytes(B, Cc, H * W)
    assert nbytes > 0
    ws = hu._settle(torch.empty(nbytes, dtype=torch.uint8, device=hu.DEV))
    loss, sample = hu.full((1,)), hu.full((B,))
    L.call("nd_diffusion_loss_f32", o.data_ptr(), tg.data_ptr(), td.data_ptr(), lw.data_ptr(), B, Cc, H * W, T, x0_term, ws.data_ptr(), loss.data_ptr(),
           sample.data_ptr(), ctx.stream)
    grad = None
    if g is not None:
        gd_, grad = hu.dev(torch.tensor([g], dtype=torch.float32)), hu.full((B, H, W, Cc))
        L.call("nd_diffusion_loss_backward_f32", o.data_ptr(), tg.data_ptr(), td.data_ptr(), lw.data_ptr(), gd_.data_ptr(), ws.data_ptr(), grad.data_ptr(),
               B, Cc, H * W, T, x0_term, ctx.stream)
    ctx.sync()
    return loss.cpu()[0], sample.cpu(), None if grad is None else hu.nchw(grad)


def ref32_loss(out, target, t, objective, g):
    """The reference's expressions (:514-528) in fp32 torch on the CPU: (loss, sample_loss, grad for the upstream gradient g)."""
    o = out.clone().requires_grad_(True)
    lw = torch.from_numpy(buffers(objective)["loss_weight"])
    sample = torch.nn.functional.mse_loss(o, target, reduction="none").flatten(1).mean(dim=1) * lw.gather(-1, t)
    loss = sample.mean()
    if objective == "pred_x0":
        loss = loss + (o.mean(dim=(2, 3)) - target.mean(dim=(2, 3))).abs().mean()
    loss.backward(torch.tensor(g))
    return loss.detach(), sample.detach(), o.grad


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_noising_with_given_draws_is_the_reference_bit_for_bit(ctx, golden, layout):
    x0, noise, t = golden_inputs()
    r = abi_noising(ctx, x0, "pred_v", layout, noise=noise, t=t, want_draws=False)
    assert torch.equal(r["t"], t)
    assert np.array_equal(r["x_t"].numpy(), golden("training", "train.x_t"))
    assert np.array_equal(r["target"].numpy(), golden("training", "train.v_target"))
    offset = synth.uniform(5, "train.offset", (GB, 4), -1.0, 1.0)
    for objective in OBJECTIVES:
        for auto, strength in ((False, 0.0), (True, 0.0), (True, 0.1)):
            r = abi_noising(ctx, x0, objective, layout, auto=auto, strength=strength, noise=noise, offset=offset, t=t, want_draws=False)
            x_t, target = R.noising(x0.numpy(), noise.numpy(), offset.numpy(), t.numpy(), *schedule(objective), objective, auto, strength)
            assert np.array_equal(r["x_t"].numpy(), x_t), (objective, auto, strength)
            assert np.array_equal(r["target"].numpy(), target), (objective, auto, strength)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DRAW_SHAPES)
def test_drawn_timesteps_noise_and_offset_match_the_restatement(ctx, shape):
    B, Cc, H, W = shape
    seed, first, draw = 0x1234567890ABCDEF, 5, 7
    x0 = synth.uniform(3, "dt.x0", shape, -1.0, 1.0)
    r = abi_noising(ctx, x0, "pred_v", strength=0.1, seed=seed, first=first, draw=draw)
    assert np.array_equal(r["t"].numpy(), R.draw_t(seed, first + np.arange(B), draw, T))
    for b in range(B):
        np.testing.assert_allclose(r["noise"][b].numpy(), R.draw_noise(seed, first + b, draw, Cc, H, W), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(r["offset"][b].numpy(), R.draw_offset(seed, first + b, draw, Cc), atol=2e-5, rtol=1e-4)
    again = abi_noising(ctx, x0, "pred_v", strength=0.1, noise=r["noise"], offset=r["offset"], t=r["t"])
    assert torch.equal(again["x_t"], r["x_t"]) and torch.equal(again["target"], r["target"])
    x_t, target = R.noising(x0.numpy(), r["noise"].numpy(), r["offset"].numpy(), r["t"].numpy(), *schedule(), "pred_v", strength=0.1)
    assert np.array_equal(r["x_t"].numpy(), x_t) and np.array_equal(r["target"].numpy(), target)
    # the device state overrides the three scalars
    dev_rng = abi_noising(ctx, x0, "pred_v", strength=0.1, seed=1, first=0, draw=0, rng=torch.tensor([seed, first, draw], dtype=torch.int64))
    assert all(torch.equal(dev_rng[k], r[k]) for k in r)


@pytest.mark.gpu
def test_draws_do_not_depend_on_the_batch_or_the_shard(ctx):
    shape = (3, 4, 24, 40)
    x0 = synth.uniform(3, "dt.x0", shape, -1.0, 1.0)
    kw = dict(strength=0.1, seed=99, draw=4)
    whole = abi_noising(ctx, x0, "pred_v", first=5, **kw)
    same = abi_noising(ctx, x0, "pred_v", first=5, **kw)
    assert all(torch.equal(whole[k], same[k]) for k in whole)
    stand_in = synth.uniform(3, "dt.out", shape, -1.0, 1.0)                  # a model output to score against the target
    _, sample, _ = abi_loss(ctx, stand_in, whole["target"], whole["t"], "pred_v")
    for i in range(3):
        one = abi_noising(ctx, x0[i:i + 1], "pred_v", first=5 + i, **kw)
        for k in whole:
            assert torch.equal(one[k], whole[k][i:i + 1]), (i, k)
        _, s1, _ = abi_loss(ctx, stand_in[i:i + 1], one["target"], one["t"], "pred_v")
        assert torch.equal(s1, sample[i:i + 1])
    for other in (dict(kw, draw=5), dict(kw, seed=100)):
        d = abi_noising(ctx, x0, "pred_v", first=5, **other)
        assert not torch.equal(d["noise"], whole["noise"]) and not torch.equal(d["offset"], whole["offset"]) and not torch.equal(d["t"], whole["t"])


def loss_shapes():
    S = 4096                                    # asserted against nd_diffusion_loss_slice_elements() in the test
    return [(2, 4, 1, S // 4 - 1), (2, 4, 1, S // 4), (2, 4, 1, S // 4 + 1)] + DRAW_SHAPES


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("shape", loss_shapes())
def test_loss_and_gradient_against_float64(ctx, shape, objective):
    assert ctx.lib.nd_diffusion_loss_slice_elements() == 4096
    B = shape[0]
    out, target = synth.uniform(4, "dl.out", shape, -1.5, 1.5), synth.uniform(4, "dl.target", shape, -1.0, 1.0)
    t = torch.tensor([3, 777, 412][:B], dtype=torch.long)
    g = 0.37
    loss, sample, grad = abi_loss(ctx, out, target, t, objective, g=g)
    x0_term = objective == "pred_x0"
    l64, s64 = R.loss64(out.numpy(), target.numpy(), t.numpy(), buffers(objective)["loss_weight"], x0_term)
    g64 = R.grad64(out.numpy(), target.numpy(), t.numpy(), buffers(objective)["loss_weight"], x0_term, g=float(np.float32(g)))
    l32, s32, g32 = ref32_loss(out, target, t, objective, g)
    derived(loss, l64, l32, "loss")
    derived(sample, s64, s32, "sample_loss")
    derived(grad, g64, g32, "grad_out")
    # the upstream gradient scales the result: doubling it is exact
    _, _, g1 = abi_loss(ctx, out, target, t, objective, g=1.0)
    _, _, g2 = abi_loss(ctx, out, target, t, objective, g=2.0)
    assert torch.equal(g2, 2 * g1) and float(g1.abs().max()) > 0


@pytest.mark.gpu
def test_argument_checks_return_the_library_codes_and_launch_nothing(ctx):
    import hiputil as hu
    lib = ctx.lib
    assert lib.nd_diffusion_noising_f32(None, ctx.stream) == -1                                      # ND_E_BADARG
    assert lib.nd_diffusion_loss_workspace_bytes(0, 4, 16) == -1
    assert lib.nd_diffusion_loss_workspace_bytes(1, 6, 16) == -2                                     # ND_E_SHAPE
    buf = hu.full((2 * 6 * 4 * 4 + 8,), 0.0)
    tt = hu._settle(torch.zeros(2, dtype=torch.int64, device=hu.DEV))
    sa, sb = (hu.dev(torch.from_numpy(v)) for v in schedule())

    def block(Cc, shift=0):
        p = L.DiffusionNoising()
        p.x0, p.x_t, p.target, p.t_out = buf.data_ptr(), buf.data_ptr() + shift, buf.data_ptr(), tt.data_ptr()
        p.sqrt_alphas_cumprod, p.sqrt_one_minus_alphas_cumprod = sa.data_ptr(), sb.data_ptr()
        p.B, p.C, p.H, p.W, p.T, p.objective = 2, Cc, 4, 4, T, 2
        return p
    assert lib.nd_diffusion_noising_f32(C.byref(block(6)), ctx.stream) == -2
    assert lib.nd_diffusion_noising_f32(C.byref(block(4, shift=4)), ctx.stream) == -3                # ND_E_ALIGN
    assert b"aligned" in lib.nd_last_error()
    assert lib.nd_diffusion_train_advance(None, ctx.stream) == -1
    assert lib.nd_diffusion_loss_f32(buf.data_ptr(), buf.data_ptr(), tt.data_ptr(), sa.data_ptr(), 2, 6, 16, T, 0, buf.data_ptr(), buf.data_ptr(), None,
                                     ctx.stream) == -2
    assert lib.nd_diffusion_loss_f32(buf.data_ptr(), buf.data_ptr(), tt.data_ptr(), sa.data_ptr(), 2, 12, 16, T, 1, buf.data_ptr(), buf.data_ptr(), None,
                                     ctx.stream) == -2                                               # the x0 term: C a power of two
    ctx.sync()
    assert float(buf.abs().max()) == 0.0 and tt.tolist() == [0, 0]                                   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- GPU, through the Python layer
DEV = torch.device("cuda", 0)


@pytest.mark.gpu
def test_python_layer_raises_where_it_does_not_run():
    x = torch.zeros(1, 4, 8, 8)
    sa, sb = (torch.from_numpy(v) for v in schedule())
    with pytest.raises(L.HipError, match="no CPU path"):
        train.diffusion_noising(x, sa, sb, objective="pred_v")
    with pytest.raises(L.HipError, match="no CPU path"):
        train.diffusion_loss(x, x, torch.zeros(1, dtype=torch.long), sa)
    xd = x.to(DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        train.diffusion_noising(torch.zeros(1, 6, 8, 8, device=DEV), sa.to(DEV), sb.to(DEV), objective="pred_v")
    with pytest.raises(ValueError, match="fp32"):
        train.diffusion_loss(xd.double(), xd.double(), torch.zeros(1, dtype=torch.long, device=DEV), sa.to(DEV))
    with pytest.raises(ValueError, match="no gradient is produced for target"):
        train.diffusion_loss(xd, xd.clone().requires_grad_(True), torch.zeros(1, dtype=torch.long, device=DEV), sa.to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_forward_under_device_rng_matches_p_losses_on_the_same_draws(objective, monkeypatch):
    B, S = 3, 16
    net, gd = plug_gd(objective, S, auto_normalize=True)
    gd = gd.to(DEV).use_device_rng(7, first_sample=2, draw=5)
    assert gd.train_rng.device.type == "cuda"
    img = synth.uniform(8, "wire.img", (B, 4, S, S), 0.0, 1.0).to(DEV)
    t_out, x_t, _target, noise_out, _ = train.diffusion_noising(img, gd.sqrt_alphas_cumprod, gd.sqrt_one_minus_alphas_cumprod, objective=objective,
                                                               auto_normalize=True, rng=gd.train_rng.clone(), return_draws=True)
    assert x_t.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(t_out.cpu().numpy(), R.draw_t(7, 2 + np.arange(B), 5, T))
    loss = gd(img, None)
    loss.backward()
    torch.cuda.synchronize()
    assert gd.train_rng.tolist() == [7, 2, 6] and torch.equal(gd.last_t, t_out)                      # one draw per call
    got = [loss.detach().cpu()] + [p.grad.cpu() for p in net.parameters()]
    # the PyTorch path on the same draws: fp32 and float64 on the CPU
    spy = []
    real = GaussianDiffusion.p_losses
    monkeypatch.setattr(GaussianDiffusion, "p_losses", lambda self, *a, **k: spy.append(1) or real(self, *a, **k))
    gd.use_device_rng(None)
    refs = []
    for dtype in (torch.float32, torch.float64):
        ref = copy.deepcopy(gd).cpu().to(dtype)
        ref.zero_grad(set_to_none=True)
        l = ref.p_losses(ref.normalize(img.cpu().to(dtype)), t_out.cpu(), None, noise=noise_out.cpu().to(dtype))
        l.backward()
        refs.append([l.detach()] + [p.grad for p in ref.model.parameters()])
    for name, a, r32, r64 in zip(["loss", "weight", "bias", "tgain"], got, *refs):
        derived(a, r64, r32, name)
    n = len(spy)
    torch.manual_seed(0)
    assert torch.isfinite(gd(img, None)) and len(spy) == n + 1 and gd.train_rng is None              # switched back: forward reaches p_losses


@pytest.mark.gpu
def test_a_step_of_the_hip_network_repeats_from_the_same_rng_state():
    from types import SimpleNamespace
    from noisediff_amd import TrainableNoiseDiffNet
    B, S = 2, 32
    net = TrainableNoiseDiffNet(SimpleNamespace(dim=16)).to(DEV).hip(True)
    gd = GaussianDiffusion(net, image_size=S, timesteps=T, beta_schedule="sigmoid2", objective="pred_v", offset_noise_strength=0.1).to(DEV)
    cond = {k: v.to(DEV) for k, v in synth.make_condition(B, S, seed=1).items()}
    img = synth.uniform(7, "img", (B, 4, S, S), -1.0, 1.0).to(DEV)
    losses = []
    for _ in range(2):
        gd.use_device_rng(21, first_sample=4, draw=3)
        net.zero_grad(set_to_none=True)
        loss = gd(img, cond)
        loss.backward()
        losses.append(loss.detach().cpu())
        assert gd.train_rng.tolist() == [21, 4, 4]
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def _small_step_setup(img):
    net, gd = plug_gd("pred_v", 16)
    gd = gd.to(DEV).use_device_rng(7)
    opt = train.Adam(net.parameters(), lr=1e-2, capturable=True)

    def one():
        opt.zero_grad(set_to_none=True)
        loss = gd(img, None)
        loss.backward()
        opt.step()
        return loss.detach()
    return gd, opt, one


@pytest.mark.gpu
def test_a_captured_step_draws_anew_on_every_replay():
    img = synth.uniform(8, "cap.img", (2, 4, 16, 16), -1.0, 1.0).to(DEV)
    side = torch.cuda.Stream()
    # eager: three steps at draw 0, 1, 2
    gd, _opt, one = _small_step_setup(img)
    eager = []
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            loss = one()
            eager.append((loss.cpu(), gd.last_t.cpu()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert gd.train_rng.tolist() == [7, 0, 3]
    assert not torch.equal(eager[1][1], eager[2][1])
    # one eager step, then the same step captured at draw k = 1 and replayed twice
    gd, opt, one = _small_step_setup(img)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss = gd(img, None)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert gd.train_rng.tolist() == [7, 0, 1]                                                        # capturing ran nothing
    for k in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach().cpu(), eager[k][0]) and torch.equal(gd.last_t.cpu(), eager[k][1]), k
    assert gd.train_rng.tolist() == [7, 0, 3]
