"""Raw Bayer frames on the GPU: what the reference does on the host before a frame reaches the denoiser and after it leaves it.

``test_denoising.py`` starts every frame pair with ``load_image`` (:86-114: ``raw_util.pack_raw_withdarkshading(raw, iso, ratio) * ratio`` or
``pack_raw(raw) * ratio``, ``pack_raw(gt)``, two clips) and ends a visualised one with ``postprocess_bayer`` (:267-293); the two training sets
of the comparison rows, ``RealSonyDenoisingDataset`` and ``PossionGaussianDenoisingDataset`` (dataloader/dataset_denoising.py:172-372), start
from ``pack_raw(rescale=False)`` and the second draws Poisson and Gaussian noise per pixel with numpy.  Here the frames stay on the device
as **uint16** and each of these is one launch of ``csrc/raw.hip``:

- ``pack_raw(frames, rescale=True)``: (N, 2H, 2W) uint16 -> (N, 4, H, W) fp32;
- ``load_pair(short, long, iso, ratio, shading=None)`` -> ``(noisy, clean)``, each (1, 4, H, W): ``load_image`` with and without
  ``--correct_darkshading``;
- ``to_bayer(img, black_level_per_channel, white=16383)``: (B, 4, h, w) fp32 -> (B, 2h, 2w) uint16, the write half of ``postprocess_bayer``;
- ``RealBatchBuilder(crop, shading=None)`` and ``PoissonGaussianBatchBuilder(crop)``: a training batch ``(noisy, clean)`` of crop windows
  from resident frames, with ``check`` / ``capture_inputs`` / ``update`` / ``launch`` / ``__call__`` and ``random_params`` as
  ``denoise_data.BatchBuilder`` has them (one ``_batch.BlockBuilder`` under all of them; the parameter block is ``RawInputs``);
- ``poisson_gaussian_params(K, VAR)``: the per-sample gain and variance of ``apply_noise`` (plain Python, not timed).

Frames are numpy uint16 arrays (copied to the device as uint16) or device tensors of a 16-bit integer dtype (torch's ``uint16`` support is
partial: pass the storage as ``int16`` where needed; the kernels read unsigned).  The numerical contract is in DESIGN.md section 12.
Deterministic: a repeated call gives the same bits and a sample's bits do not depend on the batch around it.  CPU tensors raise ``HipError``;
there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._batch import BlockBuilder, ParamBlock, check_frames, check_headroom, check_positive, need_gpu, per_sample, rng_key, write_rng
from ._host import _stream
from .denoise_data import HIGH_ISO, DarkShading, plane_ptrs as _plane_ptrs

BLACK, WHITE = 512, 16383            # the Sony sensor's black level and white point
_RNG_BYTES = 32                      # the {seed, first_sample, draw} triple as int64, padded
ROW = np.dtype([("frame", "<i4"), ("frame_clean", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("flip", "<i4"), ("branch", "<i4"), ("iso", "<f4"),
                ("ratio", "<f4"), ("blc", "<f4"), ("reserved", "<i4"), ("k", "<f8"), ("sd", "<f8"), ("ratio64", "<f8")])      # nd_raw_sample
assert ROW.itemsize == C.sizeof(L.RawSample) == 64
_WHAT = "raw frames are processed on the HIP library"              # need_gpu's half of the "no CPU path" message
_U16 = tuple(t for t in (torch.int16, getattr(torch, "uint16", None)) if t is not None)


# ----------------------------------------------------------------------------- frames

def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise L.HipError("raw frames are processed on the HIP library only; no GPU is visible and there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def frame_shape(shape: Sequence[int]) -> Tuple[int, int, int]:
    """(N, H2, W2) of a frame stack given as (H2, W2) or (N, H2, W2); ValueError unless both sides are even and positive."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or min(shape) < 1 or shape[1] % 2 or shape[2] % 2:
        raise ValueError(f"Bayer frames are (H2, W2) or (N, H2, W2) with even, positive sides; got {shape}")
    return shape


def frames_on_device(frames, device=None) -> torch.Tensor:
    """numpy uint16 (copied as uint16, to ``device`` or the current GPU) or a device tensor of a 16-bit integer dtype -> contiguous (N, H2, W2)."""
    if isinstance(frames, np.ndarray):
        if frames.dtype != np.uint16:
            raise TypeError(f"raw frames are uint16; got {frames.dtype}")
        shape = frame_shape(frames.shape)
        device = _default_device() if device is None else torch.device(device)
        if device.type != "cuda":
            raise L.HipError(f"raw frames are processed on the HIP library only; got device {device} and there is no CPU path")
        return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).reshape(shape)).to(device)
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames must be a numpy uint16 array or a torch tensor; got {type(frames)}")
    shape = frame_shape(frames.shape)
    if frames.dtype not in _U16:
        raise TypeError(f"raw frames are a 16-bit integer tensor (uint16, or its storage as int16); got {frames.dtype}")
    need_gpu(frames, what=_WHAT)
    return frames.contiguous().reshape(shape)


def _table(dev: torch.device, rows: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(rows.view(np.uint8)).to(dev)


def _whole_frame_rows(N: int, iso=0.0, ratio=1.0, shading: Optional[DarkShading] = None) -> np.ndarray:
    rows = np.zeros(N, ROW)
    rows["frame"] = np.arange(N)
    rows["iso"], rows["ratio"], rows["branch"] = iso, ratio, int(iso) > HIGH_ISO
    rows["blc"] = shading.black_level(int(iso)) if shading is not None else 0.0
    return rows


def _pack(frames: torch.Tensor, rows: np.ndarray, mode: int, flags: int, shading: Optional[DarkShading], h: int, w: int,
          black: float, white: float) -> torch.Tensor:
    dev = frames.device
    N, H2, W2 = frames.shape
    maps, mh, mw = _plane_ptrs(shading, dev)
    table = _table(dev, rows)
    out = torch.empty(len(rows), 4, h, w, dtype=torch.float32, device=dev)
    L.call("nd_raw_pack_u16_f32", frames.data_ptr(), N, H2, W2, *maps, mh, mw, table.data_ptr(), mode, flags, float(black), float(white),
           out.data_ptr(), None, len(rows), h, w, _stream(dev))
    return out


def pack_raw(frames, rescale: bool = True, black: float = BLACK, white: float = WHITE) -> torch.Tensor:
    """raw_util.pack_raw for a stack of frames: max(x - black, 0), divided by white - black when ``rescale``; (N, 4, H, W) fp32."""
    f = frames_on_device(frames)
    N, H2, W2 = f.shape
    return _pack(f, _whole_frame_rows(N), L.RAW_PACK, L.RAW_RESCALE if rescale else 0, None, H2 // 2, W2 // 2, black, white)


def load_pair(short, long, iso: int, ratio: float, shading: Optional[DarkShading] = None, black: float = BLACK,
              white: float = WHITE) -> Tuple[torch.Tensor, torch.Tensor]:
    """test_denoising.py's load_image on the device: (noisy, clean), each (1, 4, H, W) fp32 in [0, 1].

    noisy = clip(pack_raw_withdarkshading(short, iso, ratio) * ratio, 0, 1) with ``shading`` (--correct_darkshading), else
    clip(pack_raw(short) * ratio, 0, 1); clean = clip(pack_raw(long), 0, 1).  short, long: one (2H, 2W) frame each."""
    if not float(ratio) > 0 or not np.isfinite(float(ratio)):
        raise ValueError(f"ratio must be positive and finite; got {ratio}")
    s = frames_on_device(short)
    g = frames_on_device(long, s.device)
    if s.shape[0] != 1 or g.shape != s.shape:
        raise ValueError(f"short and long must be one frame each, of one shape; got {tuple(s.shape)} and {tuple(g.shape)}")
    need_gpu(s, g, what=_WHAT)
    _, H2, W2 = s.shape
    h, w = H2 // 2, W2 // 2
    if shading is not None and (shading.H < h or shading.W < w):
        raise ValueError(f"the shading planes ({shading.H} x {shading.W}) are smaller than the packed frame ({h} x {w})")
    rows = _whole_frame_rows(1, iso, ratio, shading)
    if shading is not None:
        noisy = _pack(s, rows, L.RAW_PACK_SHADED, 0, shading, h, w, black, white)
    else:
        noisy = _pack(s, rows, L.RAW_PACK, L.RAW_RESCALE | L.RAW_CLIP, None, h, w, black, white)
    clean = _pack(g, _whole_frame_rows(1), L.RAW_PACK, L.RAW_RESCALE | L.RAW_CLIP, None, h, w, black, white)
    return noisy, clean


def to_bayer(img: torch.Tensor, black_level_per_channel: Sequence[int], white: int = WHITE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The write half of postprocess_bayer: (B, 4, h, w) (or (4, h, w)) fp32 -> (B, 2h, 2w) uint16 codes
    trunc(clip(x, 0, 1) * (white - bl[c]) + bl[c]) at each channel's Bayer position; NaN gives 0.  The dtype is torch.uint16 where torch has
    it, else its storage as int16.  ``out``: a 16-bit integer tensor to write into (no allocation)."""
    if not isinstance(img, torch.Tensor):
        raise TypeError("to_bayer takes a torch tensor")
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[1] != 4 or min(img.shape) < 1:
        raise ValueError(f"img must be (B, 4, h, w); got {tuple(img.shape)}")
    bl = [int(b) for b in black_level_per_channel]
    if len(bl) != 4 or not all(0 <= b <= int(white) for b in bl) or not 0 < int(white) <= 65535:
        raise ValueError(f"need four black levels in [0, white] and white in (0, 65535]; got {bl}, white={white}")
    dev = need_gpu(img, what=_WHAT)
    x = img.to(torch.float32).contiguous()
    B, _, h, w = x.shape
    if out is None:
        out = torch.empty(B, 2 * h, 2 * w, dtype=_U16[-1], device=dev)
    elif out.dtype not in _U16 or tuple(out.shape) != (B, 2 * h, 2 * w) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous 16-bit integer tensor ({B}, {2 * h}, {2 * w}) on {dev}")
    L.call("nd_raw_to_bayer_u16", x.data_ptr(), out.data_ptr(), (C.c_int32 * 4)(*bl), int(white), B, h, w, _stream(dev))
    return out


# ----------------------------------------------------------------------------- training batches

def poisson_gaussian_params(K: float, VAR: float) -> Tuple[float, float]:
    """(k, var) of one apply_noise call: k ~ N(K, 1) truncated to [0.7 K, 1.3 K], var ~ N(VAR, 1) truncated to [0.7 VAR, 1.3 VAR], k first.

    Drawn by rejection on ``np.random.normal``: the same distribution as the reference's ``truncnorm.rvs(a, b, loc, scale=1)``, but NOT the
    same stream -- scipy inverts the CDF of one uniform, this draws normals until one lands in the interval."""
    def one(centre: float) -> float:
        centre = float(centre)
        if not centre > 0 or not np.isfinite(centre):
            raise ValueError(f"the centre of the truncated normal must be positive and finite; got {centre}")
        while True:
            v = float(np.random.normal(centre, 1.0))
            if 0.7 * centre <= v <= 1.3 * centre:
                return v
    return one(K), one(VAR)


class RawInputs(ParamBlock):
    """The device parameter block of one builder launch: the {seed, first_sample, draw} triple and the per-sample table (nd_raw_sample rows) in
    ONE byte buffer, written by ``update`` with one copy.  A captured launch reads it at replay."""
    DTYPE, HEAD, PER_SAMPLE = np.uint8, _RNG_BYTES, ROW.itemsize

    def __init__(self, B: int, device: torch.device):
        super().__init__(B, device, self.DTYPE, self.HEAD, self.PER_SAMPLE)

    rng_ptr = property(lambda self: self.ptr(0))
    table_ptr = property(lambda self: self.ptr(_RNG_BYTES))


class _WindowBuilder(BlockBuilder):
    """What the builders of crop windows share: resident frames, one table row per sample."""
    Inputs = RawInputs
    ROW = ROW                            # the table's row type: a subclass with another table names its own (and its Inputs)

    def __init__(self, crop: int, black: float = BLACK, white: float = WHITE):
        crop = int(crop)
        if crop <= 0:
            raise ValueError(f"crop must be positive; got {crop}")
        if not 0 <= float(black) < float(white) <= 65535:
            raise ValueError(f"need 0 <= black < white <= 65535; got {black}, {white}")
        self.crop, self.black, self.white = crop, float(black), float(white)

    def random_params(self, B: int, frame_hw: Tuple[int, int]) -> Dict[str, object]:
        """xy and flip of one step, drawn with the reference's calls in its order: per sample the crop's x then y (np.random.randint, rounded
        down to even; dataset_denoising.py:223-226 / :314-317), then one flip for the batch (np.random.randint(0, 2), trainer_denoising.py:108).
        frame_hw: the PACKED frame's (H, W)."""
        H, W = int(frame_hw[0]), int(frame_hw[1])
        if H < self.crop or W < self.crop:
            raise ValueError(f"the crop {self.crop} does not fit the packed frame {H} x {W}")
        xy = []
        for _ in range(int(B)):
            x = int(np.random.randint(0, W - self.crop + 1)) // 2 * 2
            y = int(np.random.randint(0, H - self.crop + 1)) // 2 * 2
            xy.append((x, y))
        return {"xy": xy, "flip": [int(np.random.randint(0, 2))] * int(B)}

    def _rows(self, host: np.ndarray, B: int, shape, frame, xy, flip) -> np.ndarray:
        """Validate the windows and write them into the table part of ``host``; returns the table as a ROW view."""
        N, H2, W2 = frame_shape(shape)
        c = self.crop
        if c > H2 // 2 or c > W2 // 2:
            raise ValueError(f"the crop {c} does not fit the packed frame {H2 // 2} x {W2 // 2}")
        frame = np.asarray(frame, dtype=np.int64).reshape(-1)
        xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
        flip = per_sample(0 if flip is None else flip, B, np.int64)
        if not (len(frame) == len(xy) == B):
            raise ValueError(f"frame indices and xy must have B={B} rows")
        check_frames(frame, N)
        if (xy < 0).any() or (xy[:, 0] > W2 // 2 - c).any() or (xy[:, 1] > H2 // 2 - c).any():
            raise ValueError(f"a {c} x {c} window at {xy.tolist()} leaves the packed frame {H2 // 2} x {W2 // 2}")
        rows = host[_RNG_BYTES:].view(self.ROW)
        rows[:] = np.zeros(B, self.ROW)
        rows["frame"], rows["x0"], rows["y0"], rows["flip"] = frame, xy[:, 0], xy[:, 1], flip != 0
        return rows

    @staticmethod
    def _ratio(ratio, B: int) -> np.ndarray:
        ratio = per_sample(ratio, B)
        check_positive(ratio, "ratio")
        return ratio

    def _device_frames(self, inputs: RawInputs, frames) -> torch.Tensor:
        if not isinstance(frames, torch.Tensor):
            raise TypeError("launch takes the frames as a device tensor (frames_on_device copies a numpy array once)")
        f = frames_on_device(frames)
        if f.device != inputs.device:
            raise ValueError(f"the parameter block is on {inputs.device}, the frames on {f.device}")
        return f


class RealBatchBuilder(_WindowBuilder):
    """RealSonyDenoisingDataset.__getitem__ for a batch, from resident frames: noisy = clip((max(x - 512, 0) [- darkshading]) * ratio, 0, 15871)
    / 15871 from the short-exposure frame, clean = max(x' - 512, 0) / 15871 from the long one, both on one crop window.

    shading: a ``DarkShading`` covering the packed frame (``--sub_darkshading``) or None."""

    def __init__(self, crop: int, shading: Optional[DarkShading] = None, black: float = BLACK, white: float = WHITE):
        super().__init__(crop, black, white)
        if shading is not None and (shading.H < self.crop or shading.W < self.crop):
            raise ValueError(f"the shading planes ({shading.H} x {shading.W}) are smaller than the crop ({self.crop})")
        self.shading = shading

    def _host_block(self, host: np.ndarray, B: int, shape, short, long, xy, iso, ratio, flip) -> None:
        rows = self._rows(host, B, shape, short, xy, flip)
        long, iso = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (long, iso))
        if not (len(long) == len(iso) == B):
            raise ValueError(f"long and iso must have B={B} entries")
        check_frames(long, frame_shape(shape)[0])
        sh = self.shading
        if sh is not None:
            if (rows["x0"] > sh.W - self.crop).any() or (rows["y0"] > sh.H - self.crop).any():
                raise ValueError(f"a window leaves the {sh.H} x {sh.W} shading planes")
            rows["blc"] = [sh.black_level(i) for i in iso]
        rows["frame_clean"], rows["iso"], rows["ratio"], rows["branch"] = long, iso, self._ratio(ratio, B), iso > HIGH_ISO

    def check(self, B: int, shape, short, long, xy, iso, ratio, flip=None) -> np.ndarray:
        """Validate one step's parameters on the host (no device is touched): ValueError for odd frame sides, a window outside the frame or
        the planes, a frame index >= N, ratio <= 0.  shape: the frames' (N, H2, W2).  Returns the parameter block as the device will read it."""
        return self._check(B, shape, short, long, xy, iso, ratio, flip)[0]

    def update(self, inputs: RawInputs, shape, short, long, xy, iso, ratio, flip=None) -> RawInputs:
        """Write one step's parameters into the device block: host validation, then ONE host-to-device copy on the current stream."""
        return self._update(inputs, shape, short, long, xy, iso, ratio, flip)

    def launch(self, inputs: RawInputs, frames: torch.Tensor, noisy: Optional[torch.Tensor] = None,
               clean_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``noisy`` and ``clean_out`` are given, no
        synchronisation, capturable.  frames: (N, H2, W2) 16-bit integers on the device."""
        f = self._device_frames(inputs, frames)
        dev, shape = f.device, (inputs.B, 4, self.crop, self.crop)
        noisy, clean_out = self._output("noisy", noisy, shape, dev), self._output("clean_out", clean_out, shape, dev)
        maps, mh, mw = _plane_ptrs(self.shading, dev)
        N, H2, W2 = f.shape
        L.call("nd_raw_pack_u16_f32", f.data_ptr(), N, H2, W2, *maps, mh, mw, inputs.table_ptr, L.RAW_TRAIN_REAL, 0, self.black, self.white,
               noisy.data_ptr(), clean_out.data_ptr(), inputs.B, self.crop, self.crop, _stream(dev))
        return noisy, clean_out

    def __call__(self, frames, short, long, xy, iso, ratio, flip=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One batch.  frames: (N, H2, W2); short, long: (B,) frame indices of each pair; xy: (B, 2) window origins (x, y) in packed pixels;
        iso, ratio: (B,); flip: (B,) or one 0/1.  Returns (noisy, clean), fp32 (B, 4, crop, crop)."""
        B = len(np.asarray(short).reshape(-1))
        host = self.check(B, tuple(frames.shape), short, long, xy, iso, ratio, flip)
        f = frames_on_device(frames)
        return self.launch(self._eager_inputs(B, host, f.device), f)


class PoissonGaussianBatchBuilder(_WindowBuilder):
    """PossionGaussianDenoisingDataset.__getitem__ for a batch, from resident long-exposure frames: clean = max(x - 512, 0) / 15871 and
    noisy = clip((k Poisson(clean_codes / ratio / k) + sqrt(var) N(0, 1)) ratio, 0, 15871) / 15871 with the per-sample k and var of
    ``poisson_gaussian_params``.  The draws are counter-based, keyed by (seed, first_sample + b, draw)."""

    def _host_block(self, host: np.ndarray, B: int, shape, frame, xy, ratio, k, var, flip, seed: int, first_sample: int, draw: int) -> None:
        rows = self._rows(host, B, shape, frame, xy, flip)
        ratio, k, var = self._ratio(ratio, B), per_sample(k, B), per_sample(var, B)
        check_positive(k, "the gain k")
        if not (var >= 0).all() or not np.isfinite(var).all():
            raise ValueError(f"the variance must be non-negative and finite; got {var.tolist()}")
        write_rng(host[:_RNG_BYTES], seed, first_sample, draw)
        check_headroom((self.white - self.black) / (ratio * k), "(white - black) / (ratio * k)")
        rows["ratio"], rows["k"], rows["sd"], rows["ratio64"] = ratio, k, np.sqrt(var), ratio

    def check(self, B: int, shape, frame, xy, ratio, k, var, flip=None, seed: int = 0, first_sample: int = 0, draw: int = 0) -> np.ndarray:
        """Validate one step's parameters on the host (no device is touched): ValueError for odd frame sides, a window outside the frame, a
        frame index >= N, k <= 0, var < 0, ratio <= 0 or (white - black) / (ratio k) >= 2**24.  Returns the parameter block."""
        return self._check(B, shape, frame, xy, ratio, k, var, flip, seed, first_sample, draw)[0]

    def update(self, inputs: RawInputs, shape, frame, xy, ratio, k, var, flip=None, seed: int = 0, first_sample: int = 0,
               draw: int = 0) -> RawInputs:
        """Write one step's parameters into the device block: host validation, then ONE host-to-device copy on the current stream."""
        return self._update(inputs, shape, frame, xy, ratio, k, var, flip, seed, first_sample, draw)

    def launch(self, inputs: RawInputs, frames: torch.Tensor, noisy: Optional[torch.Tensor] = None, clean_out: Optional[torch.Tensor] = None,
               counts: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, counts_out: Optional[torch.Tensor] = None,
               normals_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``noisy`` and ``clean_out`` are given, no
        synchronisation, capturable.  counts / normals replace the draws; counts_out / normals_out receive what was used."""
        f = self._device_frames(inputs, frames)
        dev, shape = f.device, (inputs.B, 4, self.crop, self.crop)
        noisy, clean_out = self._output("noisy", noisy, shape, dev), self._output("clean_out", clean_out, shape, dev)
        for name, t in (("counts", counts), ("normals", normals), ("counts_out", counts_out), ("normals_out", normals_out)):
            self._output(name, t, shape, dev, make=False)
        N, H2, W2 = f.shape
        L.call("nd_raw_poisson_gaussian_f32", f.data_ptr(), N, H2, W2, inputs.table_ptr, inputs.rng_ptr if inputs.use_rng else None,
               *rng_key(inputs.host[:_RNG_BYTES]), L.ptr(counts), L.ptr(normals), L.ptr(counts_out), L.ptr(normals_out),
               self.black, self.white, noisy.data_ptr(), clean_out.data_ptr(), inputs.B, self.crop, self.crop, _stream(dev))
        return noisy, clean_out

    def __call__(self, frames, frame, xy, ratio, k, var, flip=None, seed: int = 0, first_sample: int = 0, draw: int = 0,
                 counts: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, return_draws: bool = False):
        """One batch.  frames: (N, H2, W2); frame: (B,) indices; xy: (B, 2) window origins (x, y) in packed pixels; ratio, k, var: (B,) or one
        value; seed / first_sample / draw key the draws; counts, normals: (B, 4, crop, crop) to use instead of drawing.
        Returns (noisy, clean[, counts used, normals used])."""
        B = len(np.asarray(frame).reshape(-1))
        host = self.check(B, tuple(frames.shape), frame, xy, ratio, k, var, flip, seed, first_sample, draw)
        f = frames_on_device(frames)
        dev = f.device
        inputs = self._eager_inputs(B, host, dev, use_rng=False)
        given = [None if t is None else t.to(torch.float32).contiguous() for t in (counts, normals)]
        used = [torch.empty(B, 4, self.crop, self.crop, dtype=torch.float32, device=dev) for _ in range(2)] if return_draws else [None, None]
        noisy, clean = self.launch(inputs, f, counts=given[0], normals=given[1], counts_out=used[0], normals_out=used[1])
        return (noisy, clean, used[0], used[1]) if return_draws else (noisy, clean)
