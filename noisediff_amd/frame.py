"""Whole synthetic noisy frames: the sampled patches of a frame stitched into frame-sized tensors on the device, one launch of ``csrc/frame.hip``
(``nd_frame_assemble``) per batch of patches.

``io.patch_grid`` overlaps the patches of a frame by a quarter of the crop, and the tools that take the result (``metrics.evaluate_raw``,
``raw.load_pair``, ``noise_level.get_poisson_lambda``, ``Develop``, ``raw.to_bayer``) take whole frames.  Averaging the overlaps would halve the
noise variance in every overlap band, so nothing is averaged: every packed pixel has ONE owner, the patch in which it lies furthest from a patch
border, and a frame is the scatter of the patches' owned rectangles.

- ``FrameLayout(crop, frame_hw)``: the unique patch origins of one frame and the rectangle each patch owns (plain Python);
- ``FrameAssembler(crop, dark_frame=False)``: one launch for a batch of sampled patches into ``noise`` (fp32, the patches' bits), ``noisy`` (fp32,
  ``io.compose_noisy`` against the long exposure) and ``short`` (the uint16 mosaic of the short exposure, read by every raw-frame entry point as a
  camera file is), any subset; ``check`` / ``capture_inputs`` / ``update`` / ``launch`` / ``__call__`` as ``GenerationBatchBuilder`` has them
  (a ``_batch.BlockBuilder`` over a ``FrameInputs`` block);
- ``FrameSynthesizer(crop, dark_frame=False)``: the driver from resident long exposures to whole frames: condition, ``GaussianDiffusion.sample`` and
  the assembly, batch by batch at ONE batch size, with no host read in between.

The numerical contract is in DESIGN.md section 21.  CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import io
from ._batch import BlockBuilder, ParamBlock, check_frames, check_positive, cuda_device, need_gpu, per_sample
from ._host import _stream
from .diffusion_data import GenerationBatchBuilder
from .raw import _U16, BLACK, WHITE, frame_shape, frames_on_device

WANT = ("noise", "noisy", "short")                       # the entry point's argument order
ROW = np.dtype([("frame_out", "<i4"), ("frame_clean", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("ax0", "<i4"), ("ay0", "<i4"), ("ax1", "<i4"),
                ("ay1", "<i4"), ("ratio", "<f4"), ("reserved", "<i4", (3,))])                                                 # nd_frame_patch
assert ROW.itemsize == C.sizeof(L.FramePatch) == 48
_WHAT = "frames are assembled on the HIP library"          # need_gpu's half of the "no CPU path" message


def _want(want: Sequence[str]) -> Tuple[str, ...]:
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in WANT for k in want):
        raise ValueError(f"want names one at least of {WANT}; got {want}")
    return tuple(k for k in WANT if k in want)


# ----------------------------------------------------------------------------- the layout of one frame (host only)

def _seams(origins: List[int], crop: int, length: int) -> List[int]:
    """s[0] = 0, s[i + 1] = the middle of the overlap of patches i and i + 1, s[n] = length."""
    return [0] + [(a + crop + b) // 2 for a, b in zip(origins, origins[1:])] + [length]


class FrameLayout:
    """The patches of one packed frame ``frame_hw = (H, W)`` and what each owns.

    ``xs``, ``ys``: the unique, sorted per-axis origins of ``io.patch_grid(crop, W, H)`` (the reference's grid can repeat the border origin; a
    synthesizer has no use for sampling a patch twice).  ``patches``: the (x, y) origins, row-major, ``ys`` outer.  ``sx``, ``sy``: the seams,
    one between each neighbouring pair, in the middle of their overlap.  ``rects[k]`` = (ax0, ay0, ax1, ay1): patch k owns
    [ax0, ax1) x [ay0, ay1) of the packed frame.  Every pixel has exactly one owner, and lies inside its owner."""

    def __init__(self, crop: int, frame_hw: Optional[Tuple[int, int]] = None):
        crop = int(crop)
        H, W = (io.PACKED_H, io.PACKED_W) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        if crop <= 0:
            raise ValueError(f"crop must be positive; got {crop}")
        if H < crop or W < crop:
            raise ValueError(f"the crop {crop} does not fit the packed frame {H} x {W}")
        grid = io.patch_grid(crop, W, H)
        self.crop, self.H, self.W = crop, H, W
        self.xs, self.ys = sorted({x for x, _ in grid}), sorted({y for _, y in grid})
        self.sx, self.sy = _seams(self.xs, crop, W), _seams(self.ys, crop, H)
        self.patches = [(x, y) for y in self.ys for x in self.xs]
        self.rects = [(self.sx[i], self.sy[j], self.sx[i + 1], self.sy[j + 1]) for j in range(len(self.ys)) for i in range(len(self.xs))]

    def __len__(self) -> int:
        return len(self.patches)


# ----------------------------------------------------------------------------- one launch

class FrameInputs(ParamBlock):
    """The device parameter block of one assembly launch: the table of nd_frame_patch rows, written by ``update`` with one copy.  A captured
    launch reads it at replay.  ``n_out``: the number of output frames the rows were validated against."""
    DTYPE, HEAD, PER_SAMPLE = np.uint8, 0, ROW.itemsize

    def __init__(self, B: int, device: torch.device):
        super().__init__(B, device, self.DTYPE, self.HEAD, self.PER_SAMPLE)
        self.n_out = 0

    table_ptr = property(lambda self: self.ptr(0))


class FrameAssembler(BlockBuilder):
    """The owned rectangles of a batch of sampled patches (B, 4, crop, crop), scattered into whole frames: ``noise`` (F, 4, H, W) = the patch
    values, ``noisy`` (F, 4, H, W) = clip(clip(noise, -1, 1) + clean, 0, 1) with clean = max(x' - black, 0) / (white - black) of the long
    exposure, and ``short`` (F, 2H, 2W) 16-bit codes min(trunc(noisy (white - black) / ratio + black + 0.5), white).  dark_frame=True: there is
    no long exposure, clean = 0, and the packed frame's (H, W) stands where the frames would."""
    Inputs = FrameInputs

    def __init__(self, crop: int, dark_frame: bool = False, black: float = BLACK, white: float = WHITE):
        crop = int(crop)
        if crop <= 0:
            raise ValueError(f"crop must be positive; got {crop}")
        if not 0 <= float(black) < float(white) <= 65535:
            raise ValueError(f"need 0 <= black < white <= 65535; got {black}, {white}")
        self.crop, self.dark_frame, self.black, self.white = crop, bool(dark_frame), float(black), float(white)

    def _shape(self, shape) -> Tuple[int, int, int]:
        """The frames' (N, H2, W2); with dark_frame the PACKED frame's (H, W) stands for it and N is 0."""
        if self.dark_frame:
            if len(tuple(shape)) != 2:
                raise ValueError(f"a dark-frame assembler takes the packed frame's (H, W); got {tuple(shape)}")
            return (0,) + frame_shape((2 * int(shape[0]), 2 * int(shape[1])))[1:]
        return frame_shape(shape)

    def _host_block(self, host: np.ndarray, B: int, shape, n_out, frame_out, long, xy, rect, ratio, want) -> None:
        N, H2, W2 = self._shape(shape)
        H, W, c = H2 // 2, W2 // 2, self.crop
        want = _want(want)
        if c > H or c > W:
            raise ValueError(f"the crop {c} does not fit the packed frame {H} x {W}")
        if int(n_out) < 1:
            raise ValueError(f"n_out, the number of output frames, must be positive; got {n_out}")
        frame_out = np.asarray(frame_out, dtype=np.int64).reshape(-1)
        long = np.zeros(B, np.int64) if self.dark_frame else np.asarray(long, dtype=np.int64).reshape(-1)
        xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
        rect = np.asarray(rect, dtype=np.int64).reshape(-1, 4)
        if not (len(frame_out) == len(long) == len(xy) == len(rect) == B):
            raise ValueError(f"frame_out, long, xy and rect must have B={B} rows")
        check_frames(frame_out, int(n_out))
        if not self.dark_frame:
            check_frames(long, N)
        if (xy < 0).any() or (xy[:, 0] > W - c).any() or (xy[:, 1] > H - c).any():
            raise ValueError(f"a {c} x {c} patch at {xy.tolist()} leaves the packed frame {H} x {W}")
        (x0, y0), (ax0, ay0, ax1, ay1) = xy.T, rect.T
        if ((ax0 < x0) | (ax1 < ax0) | (ax1 > x0 + c) | (ay0 < y0) | (ay1 < ay0) | (ay1 > y0 + c)).any():
            raise ValueError(f"an owned rectangle (ax0, ay0, ax1, ay1) of {rect.tolist()} is not inside its {c} x {c} patch at {xy.tolist()}")
        live = np.flatnonzero((ax1 > ax0) & (ay1 > ay0))
        a, f = rect[live], frame_out[live]
        meet = ((f[:, None] == f[None, :])
                & (np.maximum(a[:, None, 0], a[None, :, 0]) < np.minimum(a[:, None, 2], a[None, :, 2]))
                & (np.maximum(a[:, None, 1], a[None, :, 1]) < np.minimum(a[:, None, 3], a[None, :, 3])))
        np.fill_diagonal(meet, False)
        if meet.any():
            i, j = (int(v) for v in np.argwhere(meet)[0])
            raise ValueError(f"rows {int(live[i])} and {int(live[j])} own overlapping rectangles of output frame {int(f[i])}: the result would "
                             "depend on the order of the writes")
        if "short" in want and ratio is None:
            raise ValueError("the short exposure needs the ratio")
        ratio = per_sample(1.0 if ratio is None else ratio, B)
        if "short" in want:
            check_positive(ratio, "ratio")
            with np.errstate(over="ignore"):
                check_positive(ratio.astype(np.float32).astype(np.float64), "ratio as fp32", ratio)      # the row holds it as fp32
        rows = host.view(ROW)
        rows[:] = np.zeros(B, ROW)
        rows["frame_out"], rows["frame_clean"], rows["x0"], rows["y0"] = frame_out, long, x0, y0
        rows["ax0"], rows["ay0"], rows["ax1"], rows["ay1"], rows["ratio"] = ax0, ay0, ax1, ay1, ratio

    def check(self, B: int, shape, n_out: int, frame_out, long, xy, rect, ratio=None, want: Sequence[str] = ("noisy",)) -> np.ndarray:
        """Validate one batch's rows on the host (no device is touched).  ValueError for odd frame sides, a crop that does not fit, a patch
        outside the frame, a rectangle outside its patch, a frame index outside [0, n_out) or [0, N), two non-empty rectangles of the batch
        that overlap on one output frame, and, when ``short`` is wanted, a ratio that is missing or not positive and finite.  An empty rectangle
        is valid.  shape: the frames' (N, H2, W2), or with dark_frame the packed (H, W), where ``long`` is ignored.  Returns the parameter
        block as the device will read it."""
        return self._check(B, shape, n_out, frame_out, long, xy, rect, ratio, want)[0]

    def update(self, inputs: FrameInputs, shape, n_out: int, frame_out, long, xy, rect, ratio=None,
               want: Sequence[str] = ("noisy",)) -> FrameInputs:
        """Write one batch's rows into the device block: host validation, then ONE host-to-device copy on the current stream."""
        self._update(inputs, shape, n_out, frame_out, long, xy, rect, ratio, want)
        inputs.n_out = int(n_out)
        return inputs

    def _out(self, name: str, t: Optional[torch.Tensor], F: int, H: int, W: int, dev: torch.device) -> torch.Tensor:
        if name != "short":
            return self._output(name, t, (F, 4, H, W), dev)
        shape = (F, 2 * H, 2 * W)
        if t is None:
            return torch.empty(shape, dtype=_U16[-1], device=dev)
        if t.dtype not in _U16 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"short must be a contiguous 16-bit integer tensor {shape} on {dev}")
        return t

    def launch(self, inputs: FrameInputs, patches: torch.Tensor, frames, out: Optional[Dict[str, torch.Tensor]] = None,
               want: Sequence[str] = ("noisy",)) -> Dict[str, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``out`` holds every tensor of ``want``, no
        synchronisation, capturable.  patches: (B, 4, crop, crop) fp32 on the device, what ``GaussianDiffusion.sample`` returns; frames:
        (N, H2, W2) 16-bit integers on the device, with dark_frame the packed frame's (H, W).  Only the tensors named in ``want`` are produced
        (the kernel gets NULL for the others), and only the rows' owned rectangles of them are written."""
        want = _want(want)
        if inputs.n_out < 1:
            raise ValueError("the parameter block holds no rows yet: update() it first")
        if not isinstance(patches, torch.Tensor):
            raise TypeError("patches must be a torch tensor")
        dev = need_gpu(patches, what=_WHAT)
        c = self.crop
        if tuple(patches.shape) != (inputs.B, 4, c, c) or patches.dtype != torch.float32 or not patches.is_contiguous():
            raise ValueError(f"patches must be fp32 contiguous {(inputs.B, 4, c, c)}; got {patches.dtype} {tuple(patches.shape)}")
        if dev != inputs.device:
            raise ValueError(f"the parameter block is on {inputs.device}, the patches on {dev}")
        f = None
        if self.dark_frame:
            N, H2, W2 = self._shape(frames)
        else:
            if not isinstance(frames, torch.Tensor):
                raise TypeError("launch takes the frames as a device tensor (frames_on_device copies a numpy array once)")
            f = frames_on_device(frames)
            if f.device != dev:
                raise ValueError(f"the patches are on {dev}, the frames on {f.device}")
            N, H2, W2 = f.shape
        res = {k: self._out(k, None if out is None else out.get(k), inputs.n_out, H2 // 2, W2 // 2, dev) for k in want}
        L.call("nd_frame_assemble", patches.data_ptr(), L.ptr(f), N, H2, W2, inputs.table_ptr, self.black, self.white,
               *[L.ptr(res.get(k)) for k in WANT], inputs.B, c, inputs.n_out, _stream(dev))
        return res

    def __call__(self, patches: torch.Tensor, frames, n_out: int, frame_out, long, xy, rect, ratio=None, want: Sequence[str] = ("noisy",),
                 out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """One batch.  patches: (B, 4, crop, crop); frames: (N, H2, W2), with dark_frame the packed (H, W); n_out: the number of output frames F;
        frame_out, long: (B,) indices of each patch's output frame and long exposure; xy: (B, 2) patch origins; rect: (B, 4) owned rectangles
        (ax0, ay0, ax1, ay1) in frame coordinates; ratio: (B,) or one value, needed for ``short``.  Returns a dict of the tensors named in
        ``want``; tensors it had to make are NOT initialised outside the rectangles written."""
        B = len(np.asarray(frame_out).reshape(-1))
        dark = self.dark_frame
        host = self.check(B, frames if dark else tuple(frames.shape), n_out, frame_out, long, xy, rect, ratio, want)
        if not isinstance(patches, torch.Tensor):
            raise TypeError("patches must be a torch tensor")
        dev = need_gpu(patches, what=_WHAT)
        f = frames if dark else frames_on_device(frames, dev)
        inputs = self._eager_inputs(B, host, dev)
        inputs.n_out = int(n_out)
        return self.launch(inputs, patches, f, out=out, want=want)


# ----------------------------------------------------------------------------- the driver

class FrameSynthesizer:
    """Whole synthetic noisy frames from resident clean long exposures: per batch of patches ``GenerationBatchBuilder`` makes the condition,
    ``GaussianDiffusion.sample`` generates the patches and ``FrameAssembler`` scatters what they own into the persistent outputs."""

    def __init__(self, crop: int, dark_frame: bool = False, black: float = BLACK, white: float = WHITE):
        self.assembler = FrameAssembler(crop, dark_frame, black, white)
        self.builder = GenerationBatchBuilder(crop, dark_frame, black, white)
        self.crop, self.dark_frame = self.assembler.crop, self.assembler.dark_frame

    @staticmethod
    def batches(layout: FrameLayout, n_frames: int, batch_size: int) -> Iterator[Tuple[int, List[int], List[Tuple[int, int]], List[Tuple[int, int, int, int]]]]:
        """(k0, frame_out, xy, rect) of each batch: the patches of all frames as one list, frame-major, in ``layout.patches`` order, walked in
        batches of EXACTLY ``batch_size``; the last batch is filled by repeating its last patch with an empty owned rectangle.  k0: the
        batch's first position in the list (plain Python)."""
        bs, P = int(batch_size), len(layout)
        if bs < 1:
            raise ValueError("batch_size must be positive")
        total = int(n_frames) * P
        if total < 1:
            raise ValueError("there must be one frame at least")
        for k0 in range(0, total, bs):
            fo, xy, rect = [], [], []
            for k in range(k0, k0 + bs):
                f, p = divmod(min(k, total - 1), P)
                x0, y0, x1, y1 = layout.rects[p]
                fo.append(f)
                xy.append(layout.patches[p])
                rect.append((x0, y0, x1, y1) if k < total else (x0, y0, x0, y0))
            yield k0, fo, xy, rect

    def __call__(self, diffusion, frames, long, iso_ratio_idx, ratio=None, batch_size: int = 16, seed: Optional[int] = None,
                 first_sample: int = 0, want: Sequence[str] = ("noisy",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """frames: (N, H2, W2) 16-bit frames, and ``long``: the indices into them of the F long exposures to synthesize from; with dark_frame
        ``frames`` is the packed (H, W) and ``long`` the number of frames F.  iso_ratio_idx, ratio: per frame, or one value for all (ratio is
        needed for ``short`` only).  Patch k of the list of ``batches`` is drawn as global sample ``first_sample + k`` of ``seed`` whatever the
        batch size (``diffusion.sample_offset`` is set per batch and restored), so the frames do not depend on ``batch_size``; seed=None draws
        one seed for the whole call.  Returns {"noise", "noisy" (F, 4, H, W) fp32, "short" (F, 2H, 2W) 16-bit}, those named in ``want``,
        written into ``out`` where it holds them."""
        want, bs, asm, gen = _want(want), int(batch_size), self.assembler, self.builder
        if self.dark_frame:
            shape, F = (int(frames[0]), int(frames[1])), int(long)
            src, dev, long = shape, cuda_device(diffusion.device), [0] * F
            H, W = shape
        else:
            src = frames_on_device(frames)
            shape, dev = tuple(src.shape), src.device
            long = [int(v) for v in np.asarray(long, dtype=np.int64).reshape(-1)]
            F, H, W = len(long), shape[1] // 2, shape[2] // 2
        if F < 1:
            raise ValueError("there must be one frame at least")
        if int(diffusion.image_size) != self.crop:
            raise ValueError(f"the diffusion model samples {diffusion.image_size} x {diffusion.image_size} patches, the synthesizer's crop is {self.crop}")
        if "short" in want and ratio is None:
            raise ValueError("the short exposure needs the ratio")
        layout = FrameLayout(self.crop, (H, W))
        idx = per_sample(iso_ratio_idx, F, np.int64)
        rat = np.array(per_sample(1.0 if ratio is None else ratio, F))
        plan = list(self.batches(layout, F, bs))
        res = {k: asm._out(k, None if out is None else out.get(k), F, H, W, dev) for k in want}
        idx_dev = torch.as_tensor(np.concatenate([idx[fo] for _, fo, _, _ in plan]), dtype=torch.int64).to(dev)       # per patch, padded tail included
        gin, ain = gen.capture_inputs(bs, dev), asm.capture_inputs(bs, dev)
        c = self.crop
        cond_out = {"position": torch.empty(bs, 2, c, c, dtype=torch.float32, device=dev)}
        if self.dark_frame:
            zeros = torch.zeros(bs, 4, c, c, dtype=torch.float32, device=dev)
        else:
            cond_out["clean_img"] = torch.empty(bs, 4, c, c, dtype=torch.float32, device=dev)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        saved = diffusion.sample_offset
        try:
            for n, (k0, fo, xy, rect) in enumerate(plan):
                lg = [long[f] for f in fo]
                gen.update(gin, shape, lg, xy)
                cond = dict(gen.launch(gin, src, cond_out))
                if self.dark_frame:
                    cond["clean_img"] = zeros
                cond["iso_ratio_idx"] = idx_dev[n * bs:(n + 1) * bs]
                diffusion.sample_offset = int(first_sample) + k0
                patches = diffusion.sample(batch_size=bs, condition=cond, seed=seed)
                asm.update(ain, shape, F, fo, lg, xy, rect, rat[fo], want)
                asm.launch(ain, patches, src, out=res, want=want)
        finally:
            diffusion.sample_offset = saved
        return res
