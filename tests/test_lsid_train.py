"""noisediff_amd.TrainableLSID: the reference's denoiser (models/archs/SID_arch.py:49-175) trained without the reference tree (train_denoising.py,
script.sh:17: L1 loss, Adam).

CPU: parameter names / shapes are the reference's, and the PyTorch path reproduces the reference's loss and parameter gradients
(tests/golden/lsid_train.npz, captured from the reference's own LSID by tests/golden/capture_lsid_train.py).
GPU: ``.hip()`` -- one autograd Function over the HIP library, forward and backward -- matches the same fixture, a float64 run of the network at
the training size, PyTorch's max-pool tie rule, repeats itself bit for bit, runs no ATen convolution / max-pool kernel, trains weights that the
inference LSID takes as they are, and captures into one CUDA graph with the optimizer."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from noisediff_amd import synth
from noisediff_amd.spec import lsid_param_spec
from util import rel_err, sub

CASES = [("l1", 2, 64, 64), ("mse", 2, 64, 64), ("l1", 1, 36, 44), ("mse", 1, 36, 44)]
LOSSES = {"l1": F.l1_loss, "mse": F.mse_loss}
NET_TOL = 2e-4


def _net():
    from noisediff_amd import TrainableLSID
    net = TrainableLSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    return net


def _data(B, H, W):
    return (synth.uniform(11, f"lsid_train.x.{H}x{W}", (B, 4, H, W), 0.0, 1.0), synth.uniform(11, f"lsid_train.y.{H}x{W}", (B, 4, H, W), 0.0, 1.0))


def _check_against_golden(golden, key, net, loss, loss_rel, grad_tol, sq_rel):
    assert float(loss.detach()) == pytest.approx(float(golden("lsid_train", f"{key}.loss")), rel=loss_rel)
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert sum(1 for g in grads.values() if g is not None) == int(golden("lsid_train", f"{key}.n_params_with_grad"))
    for k, g in grads.items():
        ref = golden("lsid_train", f"{key}.grad.{k}")
        got = sub(g.detach().cpu(), 2048)
        assert np.abs(got - ref).max() <= grad_tol * max(1.0, np.abs(ref).max()), (key, k)
    sq = sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None)
    assert sq == pytest.approx(float(golden("lsid_train", f"{key}.grad_sq_norm")), rel=sq_rel)


# ------------------------------------------------------------------------------------------------------------------------------ CPU
def test_parameter_names_and_shapes_follow_the_spec_and_load_into_lsid():
    from noisediff_amd import LSID, TrainableLSID
    net = TrainableLSID()
    spec = [(p.name, tuple(p.shape)) for p in lsid_param_spec()]
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == spec
    assert [(k, tuple(v.shape)) for k, v in LSID(None).state_dict().items()] == spec
    assert all(p.requires_grad for p in net.parameters())
    LSID(None).load_state_dict(net.state_dict(), strict=True)
    w = net.state_dict()["conv5_2.weight"]
    assert float(w.std()) == pytest.approx((2.0 / (9 * 512)) ** 0.5, rel=0.05)        # SID_arch.py:96-103: N(0, sqrt(2 / (k k out)))
    assert float(net.state_dict()["conv5_2.bias"].abs().max()) == 0.0


@pytest.mark.parametrize("loss_name,B,H,W", CASES)
def test_torch_path_loss_and_gradients_match_the_reference(golden, loss_name, B, H, W):
    x, y = _data(B, H, W)
    net = _net()
    loss = LOSSES[loss_name](net(x), y)
    loss.backward()
    _check_against_golden(golden, f"{loss_name}.{H}x{W}", net, loss, 2e-5, 2e-5, 1e-4)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
DEV = torch.device("cuda", 0)


def _hip_net():
    return _net().to(DEV).hip()


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name,B,H,W", CASES)
def test_hip_loss_and_gradients_match_the_reference(golden, loss_name, B, H, W):
    x, y = _data(B, H, W)
    net = _hip_net()
    loss = LOSSES[loss_name](net(x.to(DEV)), y.to(DEV))
    loss.backward()
    _check_against_golden(golden, f"{loss_name}.{H}x{W}", net, loss, 2e-5, 2e-5, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 36, 44), (1, 33, 47)])
def test_hip_forward_on_the_inference_kernels_is_the_inference_lsid_bit_for_bit(monkeypatch, B, H, W):
    """Training runs the launch list the inference LSID records (lsid.lsid_forward_hip): with the F(4x4) forward kernels allowed, as inference
    has them, the outputs are equal bit for bit.  At 64 x 64 the stages cover wino4, wino2 and direct."""
    from noisediff_amd import LSID, lsid, lsid_train
    monkeypatch.setattr(lsid_train, "WINO4_FORWARD", True)
    monkeypatch.setattr(lsid, "WINO4", True)
    net = _hip_net()
    inference = LSID(None)
    inference.load_state_dict(net.state_dict(), strict=True)
    inference = inference.to(DEV).eval()
    x = _data(B, H, W)[0].to(DEV)
    with torch.no_grad():
        assert torch.equal(net(x), inference(x))


def _check_float64_gradients(x, y):
    """The L1 loss's gradient at the float64 output fed to both runs: every parameter gradient within 1e-4 of its max |g| of float64 PyTorch."""
    ref = _net().to(DEV).double()
    out64 = ref(x.double())
    gy = torch.sign(out64.detach() - y.double()) / out64.numel()                  # d l1_loss / d out
    out64.backward(gy)
    net = _hip_net()
    net(x).backward(gy.float())
    got = dict(net.named_parameters())
    errs = {}
    for k, p in ref.named_parameters():
        g, r = got[k].grad.double(), p.grad
        scale = float(r.abs().max())
        assert scale > 0, k
        errs[k] = float((g - r).abs().max()) / scale
    bad = {k: e for k, e in errs.items() if not e <= 1e-4}                        # (a NaN error is bad too)
    worst = max(errs, key=lambda k: float("inf") if errs[k] != errs[k] else errs[k])
    assert not bad, f"{len(bad)} parameter(s) past 1e-4 of their max |g|; worst {worst}: {errs[worst]:.3e}"


@pytest.mark.gpu
def test_hip_gradients_at_the_training_size_match_float64():
    """B = 4, 256 x 256 (script.sh:17's crop and batch).  (2e-5 is out of reach of fp32 here: PyTorch's own fp32 path is 6.3e-5 away on its worst
    parameter, the HIP path 5.2e-5 -- 18 convolutions deep, the rounding of the forward reaches every weight gradient.)"""
    B, H = 4, 256
    x = synth.uniform(12, "lsid_train.big.x", (B, 4, H, H), 0.0, 1.0).to(DEV)
    y = synth.uniform(12, "lsid_train.big.y", (B, 4, H, H), 0.0, 1.0).to(DEV)
    _check_float64_gradients(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(1, 33, 47), (2, 17, 9)])
def test_hip_gradients_at_odd_sizes_match_float64(B, H, W):
    """Odd at full and at half resolution: the crops of every ConvTranspose (up9, up8, ...) and the clamped pooling windows of the early stages."""
    x = synth.uniform(12, f"lsid_train.odd.x.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    y = synth.uniform(12, f"lsid_train.odd.y.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    _check_float64_gradients(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (9, 11), (5, 6), (3, 3)])
def test_the_gradient_join_routes_tied_maxima_as_pytorch_does(H, W):
    """nd_leaky_grad_join_f32 on a map of exact ties (values from {-1, 0, 1}), full and ceil-mode partial windows: dz equals the autograd of
    leaky_relu -> max_pool2d(ceil_mode=True) plus a direct consumer, with the direct gradient read from a channel slice of a wider tensor."""
    from noisediff_amd import _lib as L
    B, Cc = 2, 8
    g = torch.Generator().manual_seed(H * 100 + W)
    z = torch.randint(-1, 2, (B, H, W, Cc), generator=g).float()
    z[0, :2, :2, :] = 0.0                                                            # an all-zero window: slope 0.2 and the first element wins
    wide = torch.randn(B, H, W, 2 * Cc, generator=g)
    dp = torch.randn(B, (H + 1) // 2, (W + 1) // 2, Cc, generator=g)
    zt = z.permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = F.leaky_relu(zt, 0.2)
    pooled = F.max_pool2d(a, 2, 2, ceil_mode=True)
    ((a * wide[..., Cc:].permute(0, 3, 1, 2)).sum() + (pooled * dp.permute(0, 3, 1, 2)).sum()).backward()
    want = zt.grad.permute(0, 2, 3, 1)
    zd, wd, pd = z.to(DEV).contiguous(), wide.to(DEV).contiguous(), dp.to(DEV).contiguous()
    dz = torch.empty_like(zd)
    L.call("nd_leaky_grad_join_f32", zd.data_ptr(), dz.data_ptr(), wd.data_ptr() + 4 * Cc, 2 * Cc, pd.data_ptr(), B, H, W, Cc, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(dz.cpu(), want)


@pytest.mark.gpu
def test_a_network_of_tied_maxima_sends_its_gradient_where_pytorch_does():
    """Zero input and zero biases make every pre-activation 0: every pooling window ties (first element wins), every slope is 0.2, and the bias
    gradients depend on nothing but that routing."""
    net = _hip_net()
    ref = _net()
    x = torch.zeros(1, 4, 36, 44)
    t = synth.uniform(13, "lsid_train.ties", (1, 4, 36, 44), 0.0, 1.0)
    F.mse_loss(net(x.to(DEV)), t.to(DEV)).backward()
    F.mse_loss(ref(x), t).backward()
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert rel_err(p.grad.cpu().numpy(), q.grad.numpy()) < 2e-5, k


@pytest.mark.gpu
def test_two_backward_passes_are_bitwise_equal():
    x, y = (t.to(DEV) for t in _data(2, 64, 64))
    net = _hip_net()
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        F.l1_loss(net(x), y).backward()
        runs.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_a_hip_step_runs_no_aten_convolution_or_pooling():
    x, y = (t.to(DEV) for t in _data(2, 64, 64))
    net = _hip_net()
    F.l1_loss(net(x), y).backward()                                                # warm up
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        F.l1_loss(net(x), y).backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    bad = [n for n in names if any(s in n.lower() for s in ("aten::conv", "aten::_conv", "aten::cudnn", "aten::miopen", "max_pool", "miopen", "naive_conv",
                                                             "convolution", "conv_transpose", "col2im", "im2col"))]
    assert not bad, sorted(set(bad))
    assert any("leaky_grad_join" in n for n in names)                              # the trace does show the library's kernels


@pytest.mark.gpu
def test_weights_trained_with_adam_load_into_the_inference_lsid():
    from noisediff_amd import LSID, train
    x, y = (t.to(DEV) for t in _data(1, 36, 44))
    net = _hip_net()
    opt = train.Adam(net.parameters(), lr=1e-4)
    w0 = net.conv5_2.weight.detach().clone()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        F.l1_loss(net(x), y).backward()
        opt.step()
    assert not torch.equal(w0, net.conv5_2.weight.detach())
    inf = LSID(None)
    inf.load_state_dict(net.state_dict(), strict=True)
    inf = inf.to(DEV).eval()
    with torch.no_grad():
        want = net(x)
        got = inf(x)
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < NET_TOL


@pytest.mark.gpu
def test_a_captured_step_replays_as_the_eager_step():
    """forward + L1 loss + backward + train.Adam(capturable=True) captured as one torch.cuda.graph on the current stream; one replay moves the
    weights exactly as one eager step of an identical copy does."""
    from noisediff_amd import train
    x, y = (t.to(DEV) for t in _data(2, 64, 64))
    eager, cap = _hip_net(), _hip_net()
    opt_e = train.Adam(eager.parameters(), lr=1e-4, capturable=True)
    opt_c = train.Adam(cap.parameters(), lr=1e-4, capturable=True)

    def step(net, opt):
        opt.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(x), y)
        loss.backward()
        opt.step()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                      # warm-up steps off the capture, as torch's recipe asks
        for _ in range(2):
            step(cap, opt_c)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    opt_c.zero_grad(set_to_none=True)
    # relaxed: train.Adam stages its per-step pointer table through pinned host memory, which the capture's global mode refuses to allocate
    with torch.cuda.graph(g, capture_error_mode="relaxed"):
        gloss = F.l1_loss(cap(x), y)
        gloss.backward()
        opt_c.step()
    g.replay()
    torch.cuda.synchronize()
    for _ in range(3):                                                              # the same three steps, eagerly
        want = step(eager, opt_e)
    torch.cuda.synchronize()
    assert float(gloss) == float(want)
    for (k, p), q in zip(cap.named_parameters(), eager.parameters()):
        assert torch.equal(p.detach(), q.detach()), k


@pytest.mark.gpu
def test_the_input_gradient_is_refused():
    net = _hip_net()
    x = torch.rand(1, 4, 32, 32, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        net(x)
