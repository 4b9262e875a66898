"""The end of a denoiser training step on the HIP library (noisediff_amd/csrc/denoise_loss.hip, train.denoise_loss, TrainableLSID.loss,
lsid_train.denoise_lr; the reference: models/trainer_denoising.py:66-76, 185-188, 220-240).

CPU: TrainableLSID.loss on the PyTorch path reproduces the reference's loss and gradients (tests/golden/lsid_train.npz) for L1, MSE and a weighted sum of
both; denoise_lr replays the trainer's loop; the library path refuses CPU tensors.
GPU: the kernels against their arithmetic contract (denoise_loss_ref: a float32 difference, float64 after it) within one fp32 ulp -- the pure L1 gradient
to the bit --, the same bits for an NHWC and an NCHW output, a sample's terms independent of its batch; the fused end (network + loss as one Function)
against the unfused library path to the bit, against ATen's loss within the network's tolerance and against the golden record; a step that launches
neither an ATen loss kernel nor a layout pass; the captured step with a scheduled learning rate; the argument errors."""
import collections
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import denoise_loss_ref as R
from noisediff_amd import _lib as L, lsid_train, synth, train
from test_lsid_train import CASES, NET_TOL, _check_against_golden, _data, _net

LAMBDAS = [(1.0, 0.0), (0.0, 1.0), (0.5, 2.0)]
S = 1024                                        # asserted against nd_denoise_loss_slice_pixels() where a shape is built from it
SHAPES = [(1, 4, 33, 47),                       # odd HW: no plane after the first is 16-byte aligned
          (2, 4, 17, 9),                        # HW smaller than a workgroup
          (3, 4, 64, 64),                       # several slices, B not a power of two
          (1, 4, 1, S + 1),                     # one pixel past a slice
          (2, 3, 5, 7)]                         # C != 4: NCHW only
GOLDEN_LAMBDAS = {"l1": (1.0, 0.0), "mse": (0.0, 1.0)}


@functools.lru_cache(maxsize=None)
def pair(shape):
    """(output, target) of a shape, every seventh element of the output equal to the target so that sign(0) is exercised.  Shared: never written to."""
    out = synth.uniform(6, f"denoise_loss.out.{shape}", shape, -0.5, 1.5)
    target = synth.uniform(6, f"denoise_loss.target.{shape}", shape, 0.0, 1.0)
    out.view(-1)[::7] = target.view(-1)[::7]
    return out, target


@functools.lru_cache(maxsize=None)
def reference(shape, lambdas):
    out, target = pair(shape)
    return R.loss(out.numpy(), target.numpy(), *lambdas)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("loss_name,B,H,W", CASES)
def test_torch_path_loss_matches_the_reference(golden, loss_name, B, H, W):
    x, y = _data(B, H, W)
    net = _net()
    loss = net.loss(x, y, *GOLDEN_LAMBDAS[loss_name])
    loss.backward()
    _check_against_golden(golden, f"{loss_name}.{H}x{W}", net, loss, 2e-5, 2e-5, 1e-4)


def _check_against_the_golden_combination(golden, net, loss, H, W, l1, mse):
    """The loss and every recorded gradient sample against l1 * (the golden L1 record) + mse * (the golden MSE record), at that file's tolerances."""
    from util import sub
    want = l1 * float(golden("lsid_train", f"l1.{H}x{W}.loss")) + mse * float(golden("lsid_train", f"mse.{H}x{W}.loss"))
    assert float(loss.detach()) == pytest.approx(want, rel=2e-5)
    for k, p in net.named_parameters():
        ref = l1 * golden("lsid_train", f"l1.{H}x{W}.grad.{k}").astype(np.float64) + mse * golden("lsid_train", f"mse.{H}x{W}.grad.{k}").astype(np.float64)
        got = sub(p.grad.detach().cpu(), 2048)
        assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 36, 44)])
def test_torch_path_weighted_sum_is_the_combination_of_the_reference_records(golden, B, H, W):
    x, y = _data(B, H, W)
    net = _net()
    loss, info, out = net.loss(x, y, 0.5, 2.0, details=True, return_output=True)
    loss.backward()
    _check_against_the_golden_combination(golden, net, loss, H, W, 0.5, 2.0)
    assert float(info["l1"]) == pytest.approx(float(golden("lsid_train", f"l1.{H}x{W}.loss")), rel=2e-5)
    assert float(info["mse"]) == pytest.approx(float(golden("lsid_train", f"mse.{H}x{W}.loss")), rel=2e-5)
    assert tuple(info["sample_l1"].shape) == (B,) and float(info["sample_mse"].mean()) == pytest.approx(float(info["mse"]), rel=1e-6)
    assert not out.requires_grad and tuple(out.shape) == (B, 4, H, W)


@pytest.mark.parametrize("max_iter", [10, 1000])
def test_denoise_lr_replays_the_trainers_loop(max_iter):
    want = R.trainer_lrs(max_iter, 1e-4)
    assert [lsid_train.denoise_lr(i, max_iter, 1e-4) for i in range(max_iter)] == want
    assert want[0] == 1e-4 and want[max_iter // 2 + 1] == 5e-5 and want[-1] == 1e-5


def test_the_library_loss_refuses_cpu_tensors_and_bad_weights():
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(L.HipError, match="no CPU path"):
        train.denoise_loss(x, x)
    for bad in ((-1.0, 1.0), (0.0, 0.0), (float("inf"), 0.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="not both zero"):
            _net().loss(x, x, *bad)


# ------------------------------------------------------------------------------------------------------------------------------ GPU, the C ABI
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def abi_loss(ctx, out, target, lambdas, layout="nchw", g=None):
    """nd_denoise_loss_f32 (and, with g, the backward) on CPU NCHW tensors, the output handed over in ``layout``: (terms, sample terms, grad NCHW or None)
    as numpy."""
    import hiputil as hu
    B, Cc, H, W = out.shape
    o, code = (hu.dev(out), L.LAYOUT_NCHW) if layout == "nchw" else (hu.nhwc(out), L.LAYOUT_NHWC)
    tg = hu.dev(target)
    nbytes = ctx.lib.nd_denoise_loss_workspace_bytes(B, Cc, H * W)
    assert nbytes > 0
    ws = hu._settle(torch.empty(nbytes, dtype=torch.uint8, device=hu.DEV))
    terms, sample = hu.full((3,)), hu.full((B, 2))
    L.call("nd_denoise_loss_f32", o.data_ptr(), code, tg.data_ptr(), B, Cc, H * W, *lambdas, ws.data_ptr(), terms.data_ptr(), sample.data_ptr(), ctx.stream)
    grad = None
    if g is not None:
        gd, grad = hu.dev(torch.tensor([g], dtype=torch.float32)), hu.full(tuple(o.shape))
        L.call("nd_denoise_loss_backward_f32", o.data_ptr(), code, tg.data_ptr(), gd.data_ptr(), grad.data_ptr(), B, Cc, H * W, *lambdas, ctx.stream)
    ctx.sync()
    if grad is not None:
        grad = (grad.cpu() if layout == "nchw" else hu.nchw(grad)).numpy()
    return terms.cpu().numpy(), sample.cpu().numpy(), grad


@pytest.mark.gpu
@pytest.mark.parametrize("lambdas", LAMBDAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_meet_their_arithmetic_contract(ctx, shape, lambdas):
    """Loss, terms and sample terms within one fp32 ulp of the restatement (the order of the fp64 sum is the only freedom); the pure L1 gradient equal to
    float32(g / N) sign(d) bit for bit, the others within one ulp -- for g = 1 and g = 3."""
    assert ctx.lib.nd_denoise_loss_slice_pixels() == S
    out, target = pair(shape)
    want_terms, want_sample = reference(shape, lambdas)
    for layout in ["nchw", "nhwc"] if shape[1] == 4 else ["nchw"]:
        for g in (1.0, 3.0):
            terms, sample, grad = abi_loss(ctx, out, target, lambdas, layout, g=g)
            print(f"{shape} {lambdas} {layout} g={g}: terms {terms} ref {want_terms}; sample terms max |got - ref| {np.abs(sample - want_sample).max():.3e}")
            assert R.within_one_ulp(terms, want_terms), (terms, want_terms)
            assert R.within_one_ulp(sample, want_sample)
            assert np.isfinite(grad).all() and np.count_nonzero(grad == 0) >= out.numel() // 7      # sign(0) = 0 where the output meets the target
            if lambdas == (1.0, 0.0):
                assert np.array_equal(bits(grad), bits(R.l1_grad_exact(out.numpy(), target.numpy(), g)))
            else:
                ref = R.grad(out.numpy(), target.numpy(), *lambdas, g=g)
                print(f"    grad max |got - ref| / |ref| {np.nanmax(np.abs(grad - ref) / np.where(ref == 0, np.inf, np.abs(ref))):.3e}")
                assert R.within_one_ulp(grad, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("lambdas", LAMBDAS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] == 4])
def test_the_outputs_do_not_depend_on_the_layout_of_the_network_output(ctx, shape, lambdas):
    out, target = pair(shape)
    a = abi_loss(ctx, out, target, lambdas, "nhwc", g=3.0)
    b = abi_loss(ctx, out, target, lambdas, "nchw", g=3.0)          # (abi_loss brings both gradients back as NCHW: the two are transposes of each other)
    for x, y, what in zip(a, b, ("terms", "sample terms", "grad")):
        assert np.array_equal(bits(x), bits(y)), what


@pytest.mark.gpu
def test_a_samples_terms_do_not_depend_on_its_batch(ctx):
    shape = (3, 4, 64, 64)
    out, target = pair(shape)
    for layout in ("nchw", "nhwc"):
        _, whole, _ = abi_loss(ctx, out, target, (0.5, 2.0), layout)
        _, alone, _ = abi_loss(ctx, out[1:2].contiguous(), target[1:2].contiguous(), (0.5, 2.0), layout)
        assert np.array_equal(bits(alone[0]), bits(whole[1])), layout


@pytest.mark.gpu
def test_argument_errors_return_the_library_codes_and_launch_nothing(ctx):
    import hiputil as hu
    lib = ctx.lib
    B, Cc, HW = 2, 4, 16
    buf, out3 = hu.full((B * Cc * HW + 8,), 0.0), hu.full((3,), 0.0)
    ws = hu._settle(torch.zeros(lib.nd_denoise_loss_workspace_bytes(B, Cc, HW), dtype=torch.uint8, device=hu.DEV))
    p = buf.data_ptr()

    def fwd(out=p, layout=L.LAYOUT_NCHW, c=Cc, l1=1.0, mse=0.0):
        return lib.nd_denoise_loss_f32(out, layout, p, B, c, HW, l1, mse, ws.data_ptr(), out3.data_ptr(), None, ctx.stream)

    def bwd(out=p, layout=L.LAYOUT_NCHW, c=Cc, l1=1.0, mse=0.0, grad=p):
        return lib.nd_denoise_loss_backward_f32(out, layout, p, out3.data_ptr(), grad, B, c, HW, l1, mse, ctx.stream)

    for call in (fwd, bwd):
        assert call(l1=-1.0) == -1 and b"negative" in lib.nd_last_error()                           # ND_E_BADARG
        assert call(mse=float("inf")) == -1 and call(l1=float("nan")) == -1
        assert call(l1=0.0, mse=0.0) == -1 and b"both zero" in lib.nd_last_error()
        assert call(layout=L.LAYOUT_NHWC, c=3) == -2 and b"NHWC" in lib.nd_last_error()             # ND_E_SHAPE
        assert call(c=17) == -2 and call(layout=2) == -1
        assert call(out=p + 4) == -3 and b"aligned" in lib.nd_last_error()                          # ND_E_ALIGN
        assert call(out=p + 4, layout=L.LAYOUT_NHWC) == -3
    assert bwd(grad=p + 4) == -3
    assert lib.nd_denoise_loss_f32(None, 0, p, B, Cc, HW, 1.0, 0.0, ws.data_ptr(), out3.data_ptr(), None, ctx.stream) == -1
    assert lib.nd_denoise_loss_workspace_bytes(0, 4, 16) == -1 and lib.nd_denoise_loss_workspace_bytes(1, 17, 16) == -2
    assert lib.nd_denoise_loss_workspace_bytes(3, 4, S + 1) == 3 * 2 * 16
    ctx.sync()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0 and float(out3.abs().max()) == 0.0 and int(ws.max()) == 0   # nothing was launched


# ------------------------------------------------------------------------------------------------------------------------------ GPU, the Python layer
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 4, 33, 47), (2, 3, 5, 7)])
def test_denoise_loss_is_the_kernel_with_autograd_around_it(shape):
    out, target = pair(shape)
    want_terms, want_sample = reference(shape, (0.5, 2.0))
    o = out.to(DEV).requires_grad_(True)
    loss, info = train.denoise_loss(o, target.to(DEV), 0.5, 2.0, details=True)
    (loss * 3).backward()
    got = np.array([float(loss.detach()), float(info["l1"]), float(info["mse"])], dtype=np.float32)
    assert R.within_one_ulp(got, want_terms)
    assert R.within_one_ulp(torch.stack([info["sample_l1"], info["sample_mse"]], 1).cpu().numpy(), want_sample)
    assert not any(v.requires_grad for v in info.values()) and loss.requires_grad
    assert R.within_one_ulp(o.grad.cpu().numpy(), R.grad(out.numpy(), target.numpy(), 0.5, 2.0, g=3.0))
    with torch.no_grad():
        assert float(train.denoise_loss(o, target.to(DEV), 0.5, 2.0)) == float(loss)
    with pytest.raises(ValueError, match="contiguous"):
        train.denoise_loss(o.double(), target.to(DEV).double())
    with pytest.raises(ValueError, match="no gradient is produced for target"):
        train.denoise_loss(o, target.to(DEV).requires_grad_(True))
    with pytest.raises(ValueError, match="not both zero"):
        train.denoise_loss(o, target.to(DEV), 0.0, 0.0)


def _hip_net():
    return _net().to(DEV).hip()


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("lambdas", [(1.0, 0.0), (0.5, 2.0)])
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 33, 47)])
def test_the_fused_end_is_the_unfused_library_path_bit_for_bit(B, H, W, lambdas):
    x = synth.uniform(14, f"denoise_loss.x.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    y = synth.uniform(14, f"denoise_loss.y.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    fused, unfused = _hip_net(), _hip_net()
    loss, info, out = fused.loss(x, y, *lambdas, details=True, return_output=True)
    loss.backward()
    net_out = unfused(x)
    want, want_info = train.denoise_loss(net_out, y, *lambdas, details=True)
    want.backward()
    assert torch.equal(loss.detach(), want.detach()) and float(loss) > 0
    assert all(torch.equal(info[k], want_info[k]) for k in want_info)
    assert torch.equal(out, net_out.detach()) and not out.requires_grad
    a, b = _grads(fused), _grads(unfused)
    assert all(torch.equal(a[k], b[k]) for k in b) and len(a) == len(b) == len(lsid_train.PARAM_NAMES)
    with torch.no_grad():                                                          # nobody differentiates: the same launches, no graph
        assert torch.equal(fused.loss(x, y, *lambdas), loss.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 33, 47)])
def test_the_fused_end_against_the_aten_loss(B, H, W):
    """Every parameter gradient within NET_TOL of its max |g| of F.l1_loss(net(x), y).backward() on the same library network.  (Bit-equality is expected --
    the pure L1 gradient is float32(1 / N) sign(d) on both sides -- and printed, not asserted: ATen's GPU kernel is not ours to pin.)"""
    x = synth.uniform(14, f"denoise_loss.x.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    y = synth.uniform(14, f"denoise_loss.y.{B}x{H}x{W}", (B, 4, H, W), 0.0, 1.0).to(DEV)
    fused, aten = _hip_net(), _hip_net()
    loss = fused.loss(x, y)
    loss.backward()
    want = F.l1_loss(aten(x), y)
    want.backward()
    assert float(loss) == pytest.approx(float(want), rel=2e-6)
    a, b = _grads(fused), _grads(aten)
    worst = 0.0
    for k in b:
        scale = float(b[k].abs().max())
        assert scale > 0, k
        err = float((a[k] - b[k]).abs().max()) / scale
        worst = max(worst, err)
        assert err <= NET_TOL, (k, err)
    print(f"{B}x{H}x{W}: worst parameter gradient error {worst:.3e} of max |g|; bit-equal to the ATen-loss path: {all(torch.equal(a[k], b[k]) for k in b)}; "
          f"loss bits equal: {torch.equal(loss.detach(), want.detach())}")


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name,B,H,W", CASES)
def test_hip_loss_matches_the_reference(golden, loss_name, B, H, W):
    x, y = _data(B, H, W)
    net = _hip_net()
    loss = net.loss(x.to(DEV), y.to(DEV), *GOLDEN_LAMBDAS[loss_name])
    loss.backward()
    _check_against_golden(golden, f"{loss_name}.{H}x{W}", net, loss, 2e-5, 2e-5, 1e-4)


@pytest.mark.gpu
def test_hip_weighted_sum_is_the_combination_of_the_reference_records(golden):
    x, y = _data(2, 64, 64)
    net = _hip_net()
    loss = net.loss(x.to(DEV), y.to(DEV), 0.5, 2.0)
    loss.backward()
    _check_against_the_golden_combination(golden, net, loss, 64, 64, 0.5, 2.0)


def _aten_kernels(prof) -> collections.Counter:
    """ATen's kernel launches of a profile, by kernel name."""
    return collections.Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "at::native" in e.name)


@pytest.mark.gpu
def test_a_fused_step_launches_no_aten_loss_kernel_and_no_layout_pass(monkeypatch):
    x, y = (t.to(DEV) for t in _data(2, 64, 64))
    net = _hip_net()
    net.loss(x, y, 0.5, 2.0).backward()                                            # warm up
    net.zero_grad(set_to_none=True)                                                # (a step starts without gradients: nothing to accumulate into)
    torch.cuda.synchronize()
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        net.loss(x, y, 0.5, 2.0).backward()
        torch.cuda.synchronize()
    monkeypatch.undo()
    assert "nd_nhwc_to_nchw_f32" not in calls and "nd_nchw_to_nhwc_f32" not in calls
    assert calls.count("nd_denoise_loss_f32") == 1 and calls.count("nd_denoise_loss_backward_f32") == 1 and "nd_linear_wgrad_leaky_f32" in calls
    names = [e.name for e in prof.events()]
    ops = sorted({n for n in names if n.startswith("aten::")})
    bad = [n for n in ops if n.split("::")[1].rstrip("_") in ("abs", "sign", "sgn", "mean", "sub", "mul", "div", "pow", "l1_loss", "mse_loss")]
    assert not bad, bad
    # ATen's kernels of the step are the weight plumbing of the forward (conv1_1's zero padding, the ConvTranspose weights' permuted copies) and autograd's
    # fill of the seed gradient: no arithmetic and no reduction
    kernels = _aten_kernels(prof)
    print("ATen kernels of a fused step:", {k[:120]: v for k, v in kernels.items()})
    bad = [k for k in kernels if any(s in k for s in ("Abs", "abs_kernel", "sign_kernel", "sgn", "Mean", "reduce_kernel", "MulFunctor", "Functor_add",
                                                       "FunctorOnSelf_add", "FunctorOnOther_add", "DivFunctor", "BinaryFunctor", "BUnaryFunctor", "pow_"))]
    assert not bad, bad
    assert any("loss_partial_kernel" in n for n in names) and any("loss_backward_kernel" in n for n in names)
    # against the same launches with nobody differentiating: the one ATen kernel a backward pass adds is autograd's fill of the seed gradient
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            net.loss(x, y, 0.5, 2.0)
        torch.cuda.synchronize()
    forward = _aten_kernels(prof)
    extra = kernels - forward
    assert sum(extra.values()) == 1 and "FillFunctor" in next(iter(extra)), extra


@pytest.mark.gpu
def test_a_captured_fused_step_replays_as_the_eager_steps_and_follows_the_schedule():
    """net.loss + backward + train.Adam(capturable=True, lr=<device tensor>) captured once (one stream, no parallel branches) after two warm-up steps and
    replayed twice, the lr tensor refilled from denoise_lr before the second replay: parameters and Adam state equal four eager steps of an identical
    copy under the same schedule, to the bit -- and differ from a run that keeps the base rate."""
    x, y = (t.to(DEV) for t in _data(2, 64, 64))
    base, max_iter = 1e-3, 10
    lrs = [base, base, lsid_train.denoise_lr(0, max_iter, base), lsid_train.denoise_lr(6, max_iter, base)]
    assert lrs[2] == base and lrs[3] == base / 2

    def setup():
        net = _hip_net()
        return net, train.Adam(net.parameters(), lr=torch.tensor(base, device=DEV), capturable=True)

    def step(net, opt):
        opt.zero_grad(set_to_none=True)
        loss = net.loss(x, y, 0.5, 2.0)
        loss.backward()
        opt.step()
        return loss

    def state(net, opt):
        torch.cuda.synchronize()
        return [p.detach().clone() for p in net.parameters()] + [opt.state[p][k].clone() for p in net.parameters() for k in ("exp_avg", "exp_avg_sq", "step")]

    eager, flat = setup(), setup()
    for lr in lrs:
        eager[1].set_lr(lr)
        want_loss = step(*eager)
        step(*flat)                                                                 # the base rate throughout
    want, unscheduled = state(*eager), state(*flat)
    assert not all(torch.equal(a, b) for a, b in zip(want, unscheduled))

    cap, opt = setup()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                      # warm-up steps off the capture, as torch's recipe asks
        for _ in range(2):
            step(cap, opt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    # relaxed: train.Adam stages its per-step pointer table through pinned host memory, which the capture's global mode refuses to allocate
    with torch.cuda.graph(g, capture_error_mode="relaxed"):
        gloss = cap.loss(x, y, 0.5, 2.0)
        gloss.backward()
        opt.step()
    for lr in lrs[2:]:
        opt.set_lr(lr)
        opt.check_captured_lr()
        g.replay()
    got = state(cap, opt)
    assert float(gloss) == float(want_loss)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_the_fused_end_refuses_what_forward_refuses():
    net = _hip_net()
    x, y = torch.rand(1, 4, 32, 32, device=DEV), torch.rand(1, 4, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="gradient of its input"):
        net.loss(x.clone().requires_grad_(True), y)
    with pytest.raises(L.HipError):
        net.loss(x.cpu(), y)
    with pytest.raises(L.HipError):
        net.loss(x, y.cpu())
    with pytest.raises(ValueError, match=r"\(B, 4, H, W\)"):
        net.loss(x[:, :3], y[:, :3])
    with pytest.raises(ValueError, match="contiguous fp32"):
        net.loss(x, y.double())
    with pytest.raises(ValueError, match="contiguous fp32"):
        net.loss(x, y[:, :, :16])
    with pytest.raises(ValueError, match="detach"):
        net.loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="fp32 parameters"):
        _net().to(DEV).double().hip().loss(x, y)
