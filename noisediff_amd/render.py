"""A packed RAW frame developed to an sRGB picture on the GPU: the last step of ``test_denoising.py --visualize_img``.

The reference's ``postprocess_bayer`` (:267-298) clips the network output, writes it into the uint16 mosaic and calls
``raw.postprocess(use_camera_wb=True, half_size=True, no_auto_bright=True, output_bps=8, bright=1)``.  Here that is one launch of
``csrc/develop.hip`` on the packed tensor (or on a uint16 mosaic), and rawpy is not needed for a view:

- ``gamma_curve(power=0.45, slope=4.5, imax=65536)``: dcraw's tone curve, numpy uint16[65536];
- ``Develop(black_level_per_channel, white, cam_mul, rgb_cam, gamma, bright, maximum, output_bps, half_size)``: the parameters of a camera,
  computed once; ``dev(x, window=None, out=None)`` develops (B, 4, H, W) / (4, H, W) fp32 or (B, 2H, 2W) / (2H, 2W) 16-bit integers (numpy
  uint16 through ``raw.frames_on_device``) to (B, H, W, 3), or (B, 2H, 2W, 3) with ``half_size=False`` (the bilinear demosaic), uint8 or
  uint16, interleaved as ``PIL.Image.fromarray`` takes it;
- ``postprocess_bayer(img4c, develop)``: the reference function's twin, an (H, W, 3) numpy array from ``img4c[0]``.

The arguments come from rawpy: ``black_level_per_channel``, ``camera_whitebalance`` (cam_mul) and ``color_matrix[:, :3]`` (rgb_cam).  The
numerical contract is LibRaw's develop steps restated in DESIGN.md section 20; it is checked against that restatement (tests/render_ref.py),
not against LibRaw itself.  Deterministic; an image's bytes do not depend on its batch.  CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._batch import need_gpu
from ._host import _stream
from .raw import _U16, WHITE, frame_shape, frames_on_device

_WHAT = "frames are developed on the HIP library"


def gamma_curve(power: float = 0.45, slope: float = 4.5, imax: int = 65536) -> np.ndarray:
    """dcraw's gamma_curve(power, slope, mode 2, imax) as uint16[65536], in float64: the toe slope meets the power segment at g3 (found by 48
    bisection steps); curve[i] = trunc(65536 (r < g3 ? r slope : r^power (1 + g4) - g4)) for r = i / imax < 1, else 65535."""
    g0, g1, imax = float(power), float(slope), int(imax)
    if not (math.isfinite(g0) and g0 > 0 and math.isfinite(g1) and g1 >= 0):
        raise ValueError(f"gamma needs a positive, finite power and a finite slope that is not negative; got {power}, {slope}")
    if imax < 1:
        raise ValueError(f"imax must be positive; got {imax}")
    g2 = g3 = g4 = 0.0
    bnd = [0.0, 0.0]
    bnd[g1 >= 1] = 1.0
    if g1 and (g1 - 1) * (g0 - 1) <= 0:
        for _ in range(48):
            g2 = (bnd[0] + bnd[1]) / 2
            bnd[((g2 / g1) ** -g0 - 1) / g0 - 1 / g2 > -1] = g2
        g3 = g2 / g1
        g4 = g2 * (1 / g0 - 1)
    r = np.arange(65536, dtype=np.float64) / np.float64(imax)
    v = 65536.0 * np.where(r < g3, r * g1, np.power(r, g0) * (1 + g4) - g4)
    return np.where(r < 1, np.clip(v, 0.0, 65535.0), 65535.0).astype(np.uint16)


def scale_multipliers(cam_mul: Sequence[float], maximum: float) -> np.ndarray:
    """LibRaw's scale_mul as float32[4]: pre = cam_mul in fp32 (the second green takes the first one's where it is 0), over its smallest;
    scale_mul[c] = fl32((double)pre[c] * 65535.0 / maximum)."""
    cam = [float(c) for c in cam_mul]
    if len(cam) != 4 or not all(math.isfinite(c) and c > 0 for c in cam[:3]) or not (math.isfinite(cam[3]) and cam[3] >= 0):
        raise ValueError(f"cam_mul needs three positive, finite multipliers and a fourth that is 0 (= the first green's) or positive; got {cam_mul}")
    if not (math.isfinite(float(maximum)) and float(maximum) > 0):
        raise ValueError(f"maximum must be positive and finite; got {maximum}")
    pre = np.array(cam, dtype=np.float32)
    if cam[3] == 0:
        pre[3] = pre[1]
    pre = pre / pre.min()
    mul = (pre.astype(np.float64) * 65535.0 / np.float64(maximum)).astype(np.float32)
    if not np.isfinite(mul).all():
        raise ValueError(f"cam_mul {cam_mul} over maximum {maximum} does not fit fp32")
    return mul


class Develop:
    """The develop parameters of one camera: black levels, white point, ``scale_mul`` from the camera multipliers, the camera-to-sRGB matrix and
    the tone curve (one copy per device, uploaded on first use).  ``maximum`` defaults to white - min(black); LibRaw's adjust_maximum lowers it
    for frames whose largest code lies in (0.75 max, max), so it is an argument."""

    def __init__(self, black_level_per_channel: Sequence[int] = (512,) * 4, white: int = WHITE, cam_mul: Sequence[float] = (1, 1, 1, 0),
                 rgb_cam=None, gamma: Tuple[float, float] = (0.45, 4.5), bright: float = 1.0, maximum: Optional[float] = None,
                 output_bps: int = 8, half_size: bool = True):
        bl = [int(b) for b in black_level_per_channel]
        if not 0 < int(white) <= 65535 or len(bl) != 4 or not all(0 <= b <= int(white) for b in bl):
            raise ValueError(f"need white in (0, 65535] and four black levels in [0, white]; got {bl}, white={white}")
        if output_bps not in (8, 16):
            raise ValueError(f"output_bps is 8 or 16; got {output_bps}")
        if not (math.isfinite(float(bright)) and float(bright) > 0 and int(65536 / float(bright)) >= 1):
            raise ValueError(f"bright must be positive, finite and at most 65536; got {bright}")
        m = np.eye(3, dtype=np.float32) if rgb_cam is None else np.asarray(rgb_cam, dtype=np.float32)
        if m.shape != (3, 3) or not np.isfinite(m).all():
            raise ValueError(f"rgb_cam is a finite 3 x 3 matrix; got {rgb_cam}")
        self.black, self.white, self.output_bps, self.half_size = bl, int(white), int(output_bps), bool(half_size)
        self.maximum = float(self.white - min(bl)) if maximum is None else float(maximum)
        self.scale_mul = scale_multipliers(cam_mul, self.maximum)
        self.rgb_cam = np.ascontiguousarray(m)
        self.curve = gamma_curve(gamma[0], gamma[1], int(65536 / float(bright)))
        self._curves: Dict[torch.device, torch.Tensor] = {}

    def device_curve(self, dev: torch.device) -> torch.Tensor:
        if dev not in self._curves:
            self._curves[dev] = torch.from_numpy(self.curve.view(np.int16)).to(dev)
        return self._curves[dev]

    def params(self, x0: int = 0, y0: int = 0) -> L.DevelopParams:
        """The host parameter block of one call."""
        return L.DevelopParams((C.c_int32 * 4)(*self.black), self.white, (C.c_float * 4)(*self.scale_mul.tolist()),
                               (C.c_float * 9)(*self.rgb_cam.reshape(-1).tolist()), int(x0), int(y0), self.output_bps, int(not self.half_size))

    def __call__(self, x, window: Optional[Sequence[int]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: (B, 4, H, W) or (4, H, W) fp32, or (B, 2H, 2W) or (2H, 2W) of a 16-bit integer dtype (numpy uint16 is copied to the current GPU).
        window = (x0, y0, h, w) in packed pixels (default: the frame).  Returns (B, h, w, 3), or (B, 2h, 2w, 3) at full resolution: uint8, or
        for 16 bits torch.uint16 where torch has it, else its storage as int16.  ``out``: the tensor to write into (no allocation)."""
        if isinstance(x, torch.Tensor) and x.dtype == torch.float32:
            f = x.unsqueeze(0) if x.dim() == 3 else x
            if f.dim() != 4 or f.shape[1] != 4 or min(f.shape) < 1:
                raise ValueError(f"a packed source is (B, 4, H, W) or (4, H, W); got {tuple(x.shape)}")
            B, _, H, W = f.shape
            packed = True
        elif isinstance(x, torch.Tensor) and x.dtype not in _U16:
            raise TypeError(f"the source is packed fp32 or a 16-bit integer mosaic; got {x.dtype}")
        else:
            f = x.reshape(frame_shape(x.shape)) if isinstance(x, torch.Tensor) else frames_on_device(x)
            B, H, W = f.shape[0], f.shape[1] // 2, f.shape[2] // 2
            packed = False
        x0, y0, h, w = (0, 0, H, W) if window is None else (int(v) for v in window)
        if h < 1 or w < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError(f"the window {h} x {w} at ({x0}, {y0}) leaves the packed frame {H} x {W}")
        k = 1 if self.half_size else 2
        shape = (B, k * h, k * w, 3)
        dtypes = (torch.uint8,) if self.output_bps == 8 else _U16
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype not in dtypes or tuple(out.shape) != shape or not out.is_contiguous()
                                or out.device != f.device):
            raise ValueError(f"out must be a contiguous {dtypes[-1]} tensor {shape} on {f.device}")
        dev = need_gpu(f, what=_WHAT)
        f = f.contiguous()
        if out is None:
            out = torch.empty(shape, dtype=dtypes[-1], device=dev)
        p = self.params(x0, y0)
        L.call("nd_raw_develop", f.data_ptr() if packed else None, None if packed else f.data_ptr(), B, H, W, C.byref(p),
               self.device_curve(dev).data_ptr(), out.data_ptr(), h, w, _stream(dev))
        return out


def postprocess_bayer(img4c: torch.Tensor, develop: Develop) -> np.ndarray:
    """test_denoising.py's postprocess_bayer without rawpy: ``img4c[0]`` (packed, values clipped to [0, 1]) developed by ``develop``;
    an (H, W, 3) numpy array, uint8 with the reference's output_bps=8."""
    out = develop(img4c.detach()[0])[0].cpu()
    if out.dtype == torch.uint8:
        return out.numpy()
    return (out if out.dtype == torch.int16 else out.view(torch.int16)).numpy().view(np.uint16)
