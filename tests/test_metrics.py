"""noisediff_amd.metrics: scoring of denoised frames (test_denoising.py's fourth stage) on the HIP library.

CPU: the float64 restatement (tests/metrics_ref.py) meets SSIM's closed forms; the Python layer rejects bad shapes and source batches; the C
entry points check their arguments before any HIP call.
GPU: PSNR / SSIM against the restatement, edge cases, bitwise repeatability and batch independence, IlluminanceCorrect against the
reference's own class (tests/golden/metrics.npz), the fused correction, and a whole SID frame through LSID and evaluate()."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as R
from noisediff_amd import synth

DEV = torch.device("cuda", 0)


def _pair(seed, shape, lo=-0.2, hi=1.2):
    x = synth.uniform(seed, "metrics.x", shape, lo, hi)
    y = synth.uniform(seed, "metrics.y", shape, 0.0, 1.0)
    return x, (0.7 * y + 0.3 * x).contiguous()           # correlated, so SSIM is well away from 0


# --------------------------------------------------------------------------- CPU: the restatement and argument checks

def test_restatement_closed_forms():
    x, y = _pair(1, (2, 20, 24))
    assert abs(R.ssim(x.numpy(), x.numpy()) - 1.0) < 1e-15
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5)):
        C1 = (R.K1 * 1.0) ** 2
        got = R.ssim(np.full((1, 9, 11), a, np.float32), np.full((1, 9, 11), b, np.float32))
        assert abs(got - (2 * a * b + C1) / (a * a + b * b + C1)) < 1e-12, (a, b)
    assert abs(R.ssim(x.numpy(), y.numpy()) - R.ssim(y.numpy(), x.numpy())) < 1e-15
    assert 0.2 < R.ssim(x.numpy(), y.numpy()) < 0.99
    assert R.psnr(x.numpy(), x.numpy()) == float("inf")
    with pytest.raises(ValueError):
        R.ssim(np.zeros((1, 6, 9)), np.zeros((1, 6, 9)))


def test_metrics_reject_bad_shapes_before_touching_a_device():
    from noisediff_amd import metrics
    a = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError):
        metrics.quality(a, torch.zeros(1, 4, 16, 17))
    with pytest.raises(ValueError):
        metrics.quality(torch.zeros(1, 4, 6, 16), torch.zeros(1, 4, 6, 16))
    with pytest.raises(ValueError):
        metrics.quality(torch.zeros(1, 4, 16, 6), torch.zeros(1, 4, 16, 6))
    with pytest.raises(ValueError):
        metrics.quality(torch.zeros(3, 4, 16, 16), torch.zeros(3, 4, 16, 16), illum_source=torch.zeros(2, 4, 16, 16))
    with pytest.raises(ValueError):
        metrics.IlluminanceCorrect()(torch.zeros(3, 4, 16, 16), torch.zeros(2, 4, 16, 16))
    with pytest.raises(ValueError):
        metrics.IlluminanceCorrect()(torch.zeros(3, 4, 16, 16), torch.zeros(3, 4, 16, 8))


def test_metrics_on_cpu_tensors_raise_hip_error():
    from noisediff_amd import _lib as L, metrics
    a = torch.zeros(1, 4, 16, 16)
    with pytest.raises(L.HipError):
        metrics.quality(a, a)
    with pytest.raises(L.HipError):
        metrics.IlluminanceCorrect()(a, a)


def test_entry_points_check_arguments_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(4096)                         # never dereferenced: every call below fails its checks first
    ws1 = lib.nd_image_quality_workspace_bytes(1, 4, 1424, 2128)
    assert ws1 > 0 and ws1 % 16 == 0
    for B in (2, 3, 16):
        assert lib.nd_image_quality_workspace_bytes(B, 4, 1424, 2128) == B * ws1
        assert lib.nd_illum_scale_workspace_bytes(B, 4, 1424, 2128) == B * lib.nd_illum_scale_workspace_bytes(1, 4, 1424, 2128)
    assert lib.nd_image_quality_workspace_bytes(1, 4, 6, 64) == -2
    assert lib.nd_image_quality_workspace_bytes(1, 4, 64, 6) == -2
    assert lib.nd_image_quality_workspace_bytes(0, 4, 64, 64) == -1
    assert lib.nd_illum_scale_workspace_bytes(1, 0, 64, 64) == -1
    q = lambda est, tgt, out, ws, B, Cc, H, W, rng=1.0: lib.nd_image_quality_f32(est, tgt, None, rng, out, out, out, ws, B, Cc, H, W, None)
    assert q(None, fake, fake, fake, 1, 4, 64, 64) == -1
    assert q(fake, None, fake, fake, 1, 4, 64, 64) == -1
    assert q(fake, fake, None, fake, 1, 4, 64, 64) == -1
    assert q(fake, fake, fake, None, 1, 4, 64, 64) == -1
    assert q(fake, fake, fake, fake, 0, 4, 64, 64) == -1
    assert q(fake, fake, fake, fake, 1, 4, 64, 64, 0.0) == -1
    assert q(fake, fake, fake, fake, 1, 4, 6, 64) == -2
    assert q(fake, fake, fake, fake, 1, 4, 64, 6) == -2
    assert b"at least 7" in lib.nd_last_error()
    assert lib.nd_illum_scale_f32(None, fake, 1, fake, fake, fake, 1, 4, 8, 8, None) == -1
    assert lib.nd_illum_scale_f32(fake, fake, 2, fake, fake, fake, 3, 4, 8, 8, None) == -1
    assert lib.nd_illum_scale_f32(fake, fake, 1, fake, fake, None, 3, 4, 8, 8, None) == -1
    assert lib.nd_illum_apply_f32(fake, None, fake, 1, 4, 8, 8, None) == -1
    assert lib.nd_illum_apply_f32(fake, fake, fake, 1, -4, 8, 8, None) == -1


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


def _quality_ref(x, y, R_=1.0):
    x, y = np.asarray(x), np.asarray(y)
    return np.array([R.psnr(x[b], y[b], R_) for b in range(x.shape[0])]), np.array([R.ssim(x[b], y[b], R_) for b in range(x.shape[0])])


SHAPES = [(1, 4, 64, 64), (3, 4, 37, 53), (2, 1, 7, 7), (1, 3, 96, 128), (1, 2, 70, 300), (1, 1, 33, 261)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_quality_matches_float64_restatement(shape):
    from noisediff_amd import metrics
    x, y = _pair(sum(shape), shape)
    r = metrics.quality(x.to(DEV), y.to(DEV))
    assert all(r[k].dtype == torch.float64 and r[k].shape == (shape[0],) and r[k].device == DEV for k in r)
    psnr, ssim = _quality_ref(x.numpy(), y.numpy())
    np.testing.assert_allclose(_np(r["PSNR"]), psnr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(_np(r["SSIM"]), ssim, rtol=0, atol=1e-10)
    mse = np.array([R.mse(x[b].numpy(), y[b].numpy()) for b in range(shape[0])])
    np.testing.assert_allclose(_np(r["MSE"]), mse, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_quality_data_range_255():
    from noisediff_amd import metrics
    x, y = _pair(7, (2, 4, 40, 72))
    x, y = x * 255.0, y * 255.0
    r = metrics.quality(x.to(DEV), y.to(DEV), data_range=255)
    psnr, ssim = _quality_ref(x.numpy(), y.numpy(), 255.0)
    np.testing.assert_allclose(_np(r["PSNR"]), psnr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(_np(r["SSIM"]), ssim, rtol=0, atol=1e-10)
    a = metrics.quality_assess(np.ascontiguousarray(R.clip(x[0].numpy(), 255).transpose(1, 2, 0)),
                               np.ascontiguousarray(R.clip(y[0].numpy(), 255).transpose(1, 2, 0)))
    assert set(a) == {"PSNR", "SSIM"} and isinstance(a["PSNR"], float)
    assert abs(a["PSNR"] - psnr[0]) < 1e-9 and abs(a["SSIM"] - ssim[0]) < 1e-10
    b = metrics.quality_assess(x[1].to(DEV), y[1].to(DEV), data_range=255)
    assert abs(b["PSNR"] - psnr[1]) < 1e-9 and abs(b["SSIM"] - ssim[1]) < 1e-10


@pytest.mark.gpu
def test_identical_inputs_and_nan():
    from noisediff_amd import metrics
    x, _ = _pair(3, (2, 4, 48, 64))
    r = metrics.quality(x.to(DEV), x.to(DEV))
    assert torch.isinf(r["PSNR"]).all() and (r["PSNR"] > 0).all() and (r["MSE"] == 0).all()
    assert float((r["SSIM"] - 1.0).abs().max()) < 1e-14
    xn = x.clone()
    xn[1, 2, 20, 30] = float("nan")                  # the clip keeps NaN: image 1 scores NaN, image 0 is untouched
    rn = metrics.quality(xn.to(DEV), x.to(DEV))
    assert torch.isnan(rn["PSNR"][1]) and torch.isnan(rn["SSIM"][1])
    assert torch.equal(rn["PSNR"][0], r["PSNR"][0]) and torch.equal(rn["SSIM"][0], r["SSIM"][0])


@pytest.mark.gpu
def test_bitwise_repeat_batch_independence_and_load_paths():
    from noisediff_amd import metrics
    x, y = _pair(5, (3, 4, 70, 300))
    xd, yd = x.to(DEV), y.to(DEV)
    a = metrics.quality(xd, yd, illum_source=yd)
    b = metrics.quality(xd, yd, illum_source=yd)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in range(3):
        one = metrics.quality(xd[i:i + 1].clone(), yd[i:i + 1].clone(), illum_source=yd[i:i + 1].clone())
        for k in a:
            assert torch.equal(one[k], a[k][i:i + 1]), (k, i)
    # a float-offset copy is not 16-byte aligned: the scalar loaders run, the arithmetic and its order are the same
    n = x.numel()
    buf = torch.empty(2 * n + 2, device=DEV)
    xs, ys = buf[1:n + 1].view(x.shape), buf[n + 2:].view(x.shape)
    xs.copy_(xd)
    ys.copy_(yd)
    assert xs.data_ptr() % 16 != 0
    c = metrics.quality(xs, ys, illum_source=ys)
    for k in a:
        assert torch.equal(c[k], a[k]), k


@pytest.mark.gpu
def test_illuminance_correct_matches_reference_fixture(golden):
    from noisediff_amd import metrics
    pred, source, source1 = (torch.from_numpy(golden("metrics", k)) for k in ("pred", "source", "source1"))
    corr = metrics.IlluminanceCorrect()
    for src, key in ((source, "out.b"), (source1, "out.b1")):
        got = corr(pred.to(DEV), src.to(DEV)).cpu()
        np.testing.assert_allclose(got.numpy(), golden("metrics", key), rtol=1e-5, atol=1e-7)
        k32, k64 = metrics.illumination_scale(pred.to(DEV), src.to(DEV))
        k32, k64 = k32.cpu(), k64.cpu()
        for b in range(pred.shape[0]):
            s_b = src[b if src.shape[0] > 1 else 0].numpy()
            ref = R.illum_scale(pred[b].numpy(), s_b)
            assert abs(float(k64[b]) - ref) <= 1e-13 * abs(ref), (key, b)
            assert abs(float(k32[b]) - ref) <= float(np.spacing(np.float32(ref))), (key, b)
            assert torch.equal(got[b], k32[b] * pred[b].clamp(0, 1)), (key, b)        # out == fl32(k) * clamp(p, 0, 1), bit for bit
    # the mask: changing pred where source == 1 does not change k
    moved = pred.clone()
    moved[source == 1.0] = 0.123
    assert torch.equal(metrics.illumination_scale(moved.to(DEV), source.to(DEV))[0], metrics.illumination_scale(pred.to(DEV), source.to(DEV))[0])
    # den == 0: NaN, as the reference
    pz = torch.from_numpy(golden("metrics", "pred_z"))
    got = corr(pz.to(DEV), source.to(DEV)).cpu()
    assert np.isnan(golden("metrics", "out.z")).all() and torch.isnan(got).all()
    r = metrics.quality(pz.to(DEV), source.to(DEV), illum_source=source.to(DEV))
    assert torch.isnan(r["PSNR"]).all() and torch.isnan(r["SSIM"]).all()


@pytest.mark.gpu
def test_fused_correction_equals_corrected_tensor():
    from noisediff_amd import metrics
    for shape, src_b in (((3, 4, 37, 53), 3), ((2, 4, 64, 96), 1)):
        p, s = _pair(11, shape)
        s[s > 0.9] = 1.0
        s = s[:src_b].contiguous()
        pd, sd = p.to(DEV), s.to(DEV)
        fused = metrics.quality(pd, sd.expand(shape).contiguous(), illum_source=sd)
        plain = metrics.quality(metrics.IlluminanceCorrect()(pd, sd), sd.expand(shape).contiguous())
        for k in fused:
            assert torch.equal(fused[k], plain[k]), (shape, k)


@pytest.mark.gpu
def test_evaluate_full_sid_frame_through_lsid():
    """One SID frame (1, 4, 1424, 2128: its deepest LSID level is 89 x 133) through LSID on the library and evaluate(): the network's output
    against plain-PyTorch LSID with the same weights on the same device, the scores against the restatement of the library's corrected output."""
    from types import SimpleNamespace
    from noisediff_amd import LSID, TrainableLSID, io, metrics
    from noisediff_amd.spec import lsid_param_spec
    from util import close
    H, W = io.PACKED_H, io.PACKED_W
    net = LSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    net = net.to(DEV).eval()
    clean = synth.uniform(31, "metrics.frame.clean", (1, 4, H, W), 0.0, 1.1).clamp(max=1.0)      # ~9 % saturated: excluded by the correction
    g = torch.Generator().manual_seed(31)
    noisy = io.compose_noisy(0.05 * torch.randn(clean.shape, generator=g), clean)
    nd, cd = noisy.to(DEV), clean.to(DEV)
    res = metrics.evaluate(net, nd, cd)
    assert set(res) == {"PSNR", "SSIM", "MSE"} and res["PSNR"].shape == (1,)
    with torch.no_grad():
        out = net(nd)
        ref = TrainableLSID(SimpleNamespace(), seed=0).to(DEV)(nd)
    assert out.shape == clean.shape
    assert close(out.cpu().numpy(), ref.cpu().numpy(), 2e-4, atol=5e-5)
    corrected = metrics.IlluminanceCorrect()(out.clamp(0.0, 1.0), cd).cpu().numpy()
    psnr, ssim = _quality_ref(corrected, clean.numpy())
    assert abs(res["PSNR"][0] - psnr[0]) < 1e-9 and abs(res["SSIM"][0] - ssim[0]) < 1e-10
    plain = metrics.evaluate(net, nd, cd, correct_illum=False)
    psnr0, ssim0 = _quality_ref(out.cpu().numpy(), clean.numpy())
    assert abs(plain["PSNR"][0] - psnr0[0]) < 1e-9 and abs(plain["SSIM"][0] - ssim0[0]) < 1e-10
