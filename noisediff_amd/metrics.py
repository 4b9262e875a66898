"""Scoring of denoised frames on the GPU: the fourth stage of the reference's ``script.sh`` (``test_denoising.py``).

For each SID / ELD frame the reference runs ``net(noisy).clamp(0, 1)``, ``IlluminanceCorrect`` (test_denoising.py:232-263), ``tensor2im``
(a device -> host copy and a clip to [0, 1]) and ``quality_assess`` (:220-226: skimage's ``peak_signal_noise_ratio`` and
``structural_similarity(channel_axis=2)`` on the CPU).  Here the last three steps are HIP kernels (``csrc/quality.hip``):

- ``quality(est, target, data_range, illum_source)``: PSNR, SSIM and MSE per image as fp64 (B,) device tensors; with ``illum_source`` the
  illumination correction is fused into the read of ``est``;
- ``IlluminanceCorrect``: the reference's module, ``forward(predict, source)``;
- ``quality_assess(X, Y, data_range=255)``: the reference's function, same arguments and return dict of floats;
- ``evaluate(net, noisy, clean)``: a whole ``test_denoising.py`` frame (steps 1-4) for a batch, one host read at the end;
- ``evaluate_raw(net, short, long, iso, ratio, shading)``: the same from the uint16 Bayer pair (``raw.load_pair``, then ``evaluate``).

The numerical contract (clip keeping NaN, fp64 accumulation, the interior crop, the fp32 scale) is in DESIGN.md, "Scoring the denoiser".
Deterministic: a repeated call gives the same bits and an image's results do not depend on the batch it is in.  CPU tensors raise
``HipError``; there is no fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib as L
from ._host import _stream

WINDOW = 7         # structural_similarity's default win_size


def _check_images(est: torch.Tensor, target: torch.Tensor) -> Tuple[int, int, int, int]:
    if not (isinstance(est, torch.Tensor) and isinstance(target, torch.Tensor)):
        raise TypeError("metrics take torch tensors")
    if est.dim() != 4 or est.shape != target.shape:
        raise ValueError(f"est and target must be (B, C, H, W) of one shape; got {tuple(est.shape)} and {tuple(target.shape)}")
    B, C, H, W = est.shape
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"SSIM needs H and W of at least {WINDOW} (its window); got H={H}, W={W}")
    if min(B, C) < 1:
        raise ValueError(f"empty batch: {tuple(est.shape)}")
    return B, C, H, W


def _check_source(source: torch.Tensor, shape) -> None:
    if not isinstance(source, torch.Tensor) or source.dim() != 4 or tuple(source.shape[1:]) != tuple(shape[1:]):
        raise ValueError(f"source must be (1 or B, C, H, W) with (C, H, W) = {tuple(shape[1:])}; got "
                         f"{tuple(source.shape) if isinstance(source, torch.Tensor) else type(source)}")
    if source.shape[0] not in (1, shape[0]):
        raise ValueError(f"source batch must be 1 or {shape[0]} (the reference's two branches); got {source.shape[0]}")


def _on_gpu(*ts: torch.Tensor) -> torch.device:
    dev = ts[0].device
    if dev.type != "cuda":
        raise L.HipError(f"image metrics run on the HIP library only; tensor is on {dev} and there is no CPU path")
    if any(t.device != dev for t in ts):
        raise ValueError("all tensors must be on one device")
    return dev


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _illum_scale(pred: torch.Tensor, source: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(k32, k64), each (B,): k = sum p s / sum p p over source != 1, p = clamp(pred, 0, 1)."""
    B, C, H, W = pred.shape
    ws = torch.empty(int(L.call("nd_illum_scale_workspace_bytes", B, C, H, W)), dtype=torch.uint8, device=pred.device)
    k32 = torch.empty(B, dtype=torch.float32, device=pred.device)
    k64 = torch.empty(B, dtype=torch.float64, device=pred.device)
    L.call("nd_illum_scale_f32", pred.data_ptr(), source.data_ptr(), source.shape[0], k32.data_ptr(), k64.data_ptr(), ws.data_ptr(),
           B, C, H, W, _stream(pred.device))
    return k32, k64


def illumination_scale(predict: torch.Tensor, source: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """IlluminanceCorrect's per-image scale num / den: (fp32 (B,), fp64 (B,)) device tensors."""
    if not isinstance(predict, torch.Tensor) or predict.dim() != 4:
        raise ValueError(f"predict must be (B, C, H, W); got {tuple(predict.shape) if isinstance(predict, torch.Tensor) else type(predict)}")
    _check_source(source, predict.shape)
    _on_gpu(predict, source)
    return _illum_scale(_f32(predict), _f32(source))


class IlluminanceCorrect(nn.Module):
    """test_denoising.py:232-263 on the HIP library: out = k * clamp(predict, 0, 1) with k = num / den per image, ``source`` of batch 1
    (one source for every image) or B.  k is formed in fp64 and applied in fp32; den == 0 gives NaN or inf, as in the reference."""

    def forward(self, predict: torch.Tensor, source: torch.Tensor) -> torch.Tensor:
        k32, _ = illumination_scale(predict, source)
        p = _f32(predict)
        B, C, H, W = p.shape
        out = torch.empty_like(p)
        L.call("nd_illum_apply_f32", p.data_ptr(), k32.data_ptr(), out.data_ptr(), B, C, H, W, _stream(p.device))
        return out


def quality(est: torch.Tensor, target: torch.Tensor, data_range: float = 1.0,
            illum_source: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """PSNR, SSIM and MSE of each image of ``est`` against ``target`` (both (B, C, H, W) on one GPU), fp64 (B,) device tensors.

    Both images are clipped to [0, data_range] first (NaN kept), as tensor2im does; with data_range 255 the caller multiplies by 255
    first, as utils/metric_util.py does.  ``illum_source``: correct ``est`` with IlluminanceCorrect()(est, illum_source) on the fly --
    bit for bit the scores of the corrected tensor, without writing it."""
    B, C, H, W = _check_images(est, target)
    if illum_source is not None:
        _check_source(illum_source, est.shape)
        _on_gpu(est, target, illum_source)
    else:
        _on_gpu(est, target)
    if not data_range > 0 or not np.isfinite(data_range):
        raise ValueError(f"data_range must be positive and finite, got {data_range}")
    x, y = _f32(est), _f32(target)
    k32 = _illum_scale(x, _f32(illum_source))[0] if illum_source is not None else None
    dev = x.device
    ws = torch.empty(int(L.call("nd_image_quality_workspace_bytes", B, C, H, W)), dtype=torch.uint8, device=dev)
    res = torch.empty(3, B, dtype=torch.float64, device=dev)
    L.call("nd_image_quality_f32", x.data_ptr(), y.data_ptr(), L.ptr(k32), float(data_range), res[0].data_ptr(), res[1].data_ptr(),
           res[2].data_ptr(), ws.data_ptr(), B, C, H, W, _stream(dev))
    return {"PSNR": res[0], "SSIM": res[1], "MSE": res[2]}


def _as_image(a, device: torch.device) -> torch.Tensor:
    """(H, W, C) numpy (tensor2im's layout) or (C, H, W) / (1, C, H, W) tensor -> (1, C, H, W) fp32 on ``device``."""
    if isinstance(a, np.ndarray):
        if a.ndim != 3:
            raise NotImplementedError("quality_assess takes one (H, W, C) image, as the reference")
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1), dtype=np.float32)).unsqueeze(0).to(device)
    if isinstance(a, torch.Tensor):
        if a.dim() == 3:
            a = a.unsqueeze(0)
        if a.dim() != 4 or a.shape[0] != 1:
            raise ValueError(f"quality_assess takes one image: (C, H, W) or (1, C, H, W) tensor; got {tuple(a.shape)}")
        return a
    raise TypeError(f"quality_assess takes a numpy array or a torch tensor, got {type(a)}")


def quality_assess(X, Y, data_range: float = 255) -> Dict[str, float]:
    """test_denoising.py:220-226 / utils/metric_util.py:28-35 on the HIP library: {'PSNR', 'SSIM'} of the estimate X against the ground
    truth Y.  X, Y: (H, W, C) numpy arrays (tensor2im's output; copied to the current GPU) or (C, H, W) / (1, C, H, W) GPU tensors."""
    dev = Y.device if isinstance(Y, torch.Tensor) else X.device if isinstance(X, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    r = quality(_as_image(X, dev), _as_image(Y, dev), float(data_range))
    v = torch.stack([r["PSNR"][0], r["SSIM"][0]]).cpu()
    return {"PSNR": float(v[0]), "SSIM": float(v[1])}


def evaluate(net: nn.Module, noisy: torch.Tensor, clean: torch.Tensor, correct_illum: bool = True,
             data_range: float = 1.0) -> Dict[str, np.ndarray]:
    """test_denoising.py:318-343 for a batch of frames on the device: output = net(noisy).clamp(0, 1), IlluminanceCorrect when
    ``correct_illum`` (--correct_illum), then PSNR and SSIM against ``clean``.  Returns {'PSNR', 'SSIM', 'MSE'} as float64 numpy (B,)
    arrays from one host read.  The clamp and the correction are read into the metric kernel (clip(k * clamp(output, 0, 1))), so the
    corrected frame is never written; data_range 255 scales both images by 255 first (utils/metric_util.py's tensor2im)."""
    _check_images(noisy, clean)
    _on_gpu(noisy, clean)
    with torch.no_grad():
        out = net(noisy)
    if out.shape != clean.shape:
        raise ValueError(f"net output {tuple(out.shape)} does not match clean {tuple(clean.shape)}")
    if data_range == 1.0:
        r = quality(out, clean, 1.0, illum_source=clean if correct_illum else None)
    else:
        est = IlluminanceCorrect()(out, clean) if correct_illum else _f32(out)
        r = quality(est * data_range, _f32(clean) * data_range, data_range)       # the kernel clips both to [0, data_range]
    v = torch.stack([r["PSNR"], r["SSIM"], r["MSE"]]).cpu().numpy()
    return {"PSNR": v[0], "SSIM": v[1], "MSE": v[2]}


def evaluate_raw(net: nn.Module, short, long, iso: int, ratio: float, shading=None, correct_illum: bool = True) -> Dict[str, np.ndarray]:
    """A ``test_denoising.py`` frame from its uint16 Bayer pair: ``raw.load_pair(short, long, iso, ratio, shading)`` (load_image, :86-114, with
    ``shading`` for --correct_darkshading) followed by ``evaluate``.  short, long: (2H, 2W) numpy uint16 or 16-bit integer device tensors."""
    from .raw import load_pair
    noisy, clean = load_pair(short, long, iso, ratio, shading)
    return evaluate(net, noisy, clean, correct_illum=correct_illum)
