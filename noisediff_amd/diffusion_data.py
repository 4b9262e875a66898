"""The diffusion model's own batches from resident uint16 Bayer frames: what ``dataloader/dataset.py`` does on the host for the trainer and the
generator of ``trainer_diffusion.py``, as one launch of ``csrc/raw.hip`` (``nd_raw_diffusion_batch_f32``).

The reference packs two whole 12 M-pixel frames per training sample, multiplies, clips and subtracts over the whole frame, builds the whole
coordinate grid and only then crops (``SonyTrainDataset.__getitem__`` :106-145); for every patch of a generated frame it packs the whole long
exposure and builds the whole grid again (``NoiseImageGenerationDataset.__getitem__`` :242-281).  Here only the windows are computed:

- ``DiffusionBatchBuilder(crop)``: a training batch ``{"noise", "noisy_img", "clean_img", "coord"[, "iso_ratio_idx"]}`` for
  ``GaussianDiffusion.forward(batch["noise"], condition=builder.condition(batch))``;
- ``GenerationBatchBuilder(crop, dark_frame=False)``: the condition ``{"clean_img", "position", "iso_ratio_idx", "image_coord"}`` of
  ``GaussianDiffusion.sample(batch_size=B, condition=...)`` for patches of ``io.patch_grid``; ``dark_frame=True`` is ``GenDarkFrameDataset``
  (coordinates only, ``clean_img`` zeros);
- ``balanced_sample_list(pairs)``: the resampling of ``SonyTrainDataset.__init__`` (plain Python).

Both builders have ``check`` / ``capture_inputs`` / ``update`` / ``launch`` / ``__call__`` as ``raw.RealBatchBuilder`` has them (they
derive from ``raw._WindowBuilder``, a ``_batch.BlockBuilder`` over a ``raw.RawInputs`` block).  The
``(iso, ratio) -> iso_ratio_idx`` table belongs to the checkpoint and stays with the caller: the builders take indices.  The numerical contract
is in DESIGN.md section 13: every output equals the reference's bit for bit.  CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import io
from ._batch import check_frames, cuda_device
from ._host import _stream
from .raw import BLACK, WHITE, RawInputs, _WindowBuilder, _default_device, frame_shape, frames_on_device

TRAIN_KEYS = ("noise", "noisy_img", "clean_img", "coord")        # the reference's names, in the entry point's argument order
_CHANNELS = {"noise": 4, "noisy_img": 4, "clean_img": 4, "coord": 2, "position": 2}


def _need_side_of_two(shape) -> Tuple[int, int, int]:
    N, H2, W2 = frame_shape(shape)
    if H2 < 4 or W2 < 4:
        raise ValueError(f"the coordinates divide by H - 1 and W - 1: the packed frame {H2 // 2} x {W2 // 2} needs sides of 2 at least")
    return N, H2, W2


def _index_tensor(iso_ratio_idx, B: int, dev: torch.device) -> torch.Tensor:
    idx = torch.as_tensor(iso_ratio_idx, dtype=torch.int64).reshape(-1)
    if idx.numel() == 1 and B > 1:
        idx = idx.expand(B)
    if idx.numel() != B:
        raise ValueError(f"iso_ratio_idx must have B={B} entries; got {idx.numel()}")
    return idx.to(dev).contiguous()


class _DiffusionLaunch(_WindowBuilder):
    """The launch the two builders share: named outputs, the ones not asked for passed as NULL."""

    def _outputs(self, inputs: RawInputs, dev: torch.device, names: Sequence[str], out: Optional[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
        return {name: self._output(name, None if out is None else out.get(name), (inputs.B, _CHANNELS[name], self.crop, self.crop), dev)
                for name in names}

    def _launch(self, inputs: RawInputs, frames: Optional[torch.Tensor], shape, ptrs: Sequence[Optional[int]]) -> None:
        N, H2, W2 = shape
        L.call("nd_raw_diffusion_batch_f32", L.ptr(frames), N, H2, W2, inputs.table_ptr, self.black, self.white, *ptrs, inputs.B, self.crop,
               self.crop, _stream(inputs.device))


class DiffusionBatchBuilder(_DiffusionLaunch):
    """SonyTrainDataset.__getitem__ for a batch, from resident frames: noisy_img = clip(max(x - 512, 0) / 15871 * ratio, 0, 1) from the short
    exposure, clean_img = max(x' - 512, 0) / 15871 from the long one (not clipped), noise = noisy_img - clean_img, and coord = the window of
    make_coord(H, W, rescale=True) over the whole packed frame, channels first."""

    def random_params(self, B: int, frame_hw: Tuple[int, int]) -> Dict[str, object]:
        """xy of one step, drawn with the reference's calls in its order (dataset.py:92-99): per sample np.random.uniform(), then
        x = randint(0, W - crop + 1); a uniform below 0.5 draws y = randint(0, H - crop + 1) as well, any other takes the band
        y = H - crop - 1 without a second draw.  Nothing is rounded to even and there is no flip.  frame_hw: the PACKED frame's (H, W)."""
        H, W = int(frame_hw[0]), int(frame_hw[1])
        if H <= self.crop or W < self.crop:
            raise ValueError(f"the crop {self.crop} needs a packed frame of at least {self.crop + 1} x {self.crop} (the band's y is H - crop - 1); "
                             f"got {H} x {W}")
        xy = []
        for _ in range(int(B)):
            free = np.random.uniform() < 0.5
            x = int(np.random.randint(0, W - self.crop + 1))
            y = int(np.random.randint(0, H - self.crop + 1)) if free else H - self.crop - 1
            xy.append((x, y))
        return {"xy": xy}

    def _host_block(self, host: np.ndarray, B: int, shape, short, long, xy, ratio) -> None:
        N = _need_side_of_two(shape)[0]
        rows = self._rows(host, B, shape, short, xy, None)
        long = np.asarray(long, dtype=np.int64).reshape(-1)
        if len(long) != B:
            raise ValueError(f"long must have B={B} entries")
        check_frames(long, N)
        rows["frame_clean"], rows["ratio"] = long, self._ratio(ratio, B)

    def check(self, B: int, shape, short, long, xy, ratio) -> np.ndarray:
        """Validate one step's parameters on the host (no device is touched): ValueError for odd frame sides or a packed side below 2, a
        window outside the frame, a frame index outside [0, N), ratio <= 0 or not finite.  shape: the frames' (N, H2, W2).  Returns the
        parameter block as the device will read it."""
        return self._check(B, shape, short, long, xy, ratio)[0]

    def update(self, inputs: RawInputs, shape, short, long, xy, ratio) -> RawInputs:
        """Write one step's parameters into the device block: host validation, then ONE host-to-device copy on the current stream."""
        return self._update(inputs, shape, short, long, xy, ratio)

    def launch(self, inputs: RawInputs, frames: torch.Tensor, out: Optional[Dict[str, torch.Tensor]] = None,
               want: Sequence[str] = ("noise", "clean_img", "coord")) -> Dict[str, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``out`` holds every tensor of ``want``, no
        synchronisation, capturable.  Only the tensors named in ``want`` are produced; the kernel gets NULL for the others."""
        want = tuple(want)
        if not want or any(k not in TRAIN_KEYS for k in want):
            raise ValueError(f"want names one at least of {TRAIN_KEYS}; got {want}")
        f = self._device_frames(inputs, frames)
        _need_side_of_two(f.shape)
        res = self._outputs(inputs, f.device, [k for k in TRAIN_KEYS if k in want], out)
        self._launch(inputs, f, tuple(f.shape), [L.ptr(res.get(k)) for k in TRAIN_KEYS])
        return res

    def __call__(self, frames, short, long, xy, ratio, iso_ratio_idx=None,
                 want: Sequence[str] = ("noise", "clean_img", "coord")) -> Dict[str, torch.Tensor]:
        """One batch.  frames: (N, H2, W2); short, long: (B,) frame indices of each pair; xy: (B, 2) window origins (x, y) in packed pixels;
        ratio: (B,) or one value; iso_ratio_idx: (B,) indices into the checkpoint's table, returned as an int64 device tensor.
        Returns a dict of the tensors named in ``want``: noise, noisy_img, clean_img (B, 4, crop, crop) and coord (B, 2, crop, crop), fp32."""
        B = len(np.asarray(short).reshape(-1))
        host = self.check(B, tuple(frames.shape), short, long, xy, ratio)
        f = frames_on_device(frames)
        batch = self.launch(self._eager_inputs(B, host, f.device), f, want=want)
        if iso_ratio_idx is not None:
            batch["iso_ratio_idx"] = _index_tensor(iso_ratio_idx, B, f.device)
        return batch

    @staticmethod
    def condition(batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The condition dict of the trainer's ``self.diffusion(noise_gt, condition=...)`` (trainer_diffusion.py:179)."""
        return {"clean_img": batch["clean_img"], "iso_ratio_idx": batch["iso_ratio_idx"], "position": batch["coord"]}


class GenerationBatchBuilder(_DiffusionLaunch):
    """NoiseImageGenerationDataset.__getitem__ for a batch of patches: clean_img = max(x' - 512, 0) / 15871 from the long exposure and
    position = the patch's window of make_coord(H, W, rescale=True).  dark_frame=True is GenDarkFrameDataset: the launch makes the coordinates
    alone, from the frame's size, and clean_img is zeros (trainer_diffusion.py:289-291)."""

    def __init__(self, crop: int, dark_frame: bool = False, black: float = BLACK, white: float = WHITE):
        super().__init__(crop, black, white)
        self.dark_frame = bool(dark_frame)

    def grid(self, frame_hw: Optional[Tuple[int, int]] = None) -> List[Tuple[int, int]]:
        """io.patch_grid(crop, W, H): the (x, y) origins of one frame's patches, row-major.  frame_hw: the PACKED frame's (H, W); the default is
        the SID Sony geometry, which the reference hard-codes (dataset.py:203)."""
        H, W = (io.PACKED_H, io.PACKED_W) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        if H < self.crop or W < self.crop:
            raise ValueError(f"the crop {self.crop} does not fit the packed frame {H} x {W}")
        return io.patch_grid(self.crop, W, H)

    def frame_batches(self, frame_index: int, batch_size: int, frame_hw: Optional[Tuple[int, int]] = None) -> Iterator[Tuple[List[int], List[Tuple[int, int]]]]:
        """(frame, xy) lists of at most ``batch_size`` patches that walk one frame's grid in the reference's row-major order."""
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        grid = self.grid(frame_hw)
        for i in range(0, len(grid), int(batch_size)):
            xy = grid[i:i + int(batch_size)]
            yield [int(frame_index)] * len(xy), xy

    def _shape(self, shape) -> Tuple[int, int, int]:
        """The frames' (N, H2, W2); with dark_frame the PACKED frame's (H, W) stands for it."""
        if self.dark_frame:
            if len(tuple(shape)) != 2:
                raise ValueError(f"a dark-frame builder takes the packed frame's (H, W); got {tuple(shape)}")
            shape = (1, 2 * int(shape[0]), 2 * int(shape[1]))
        return _need_side_of_two(shape)

    def _host_block(self, host: np.ndarray, B: int, shape, frame, xy) -> None:
        frame = np.zeros(B, np.int64) if self.dark_frame else frame
        rows = self._rows(host, B, self._shape(shape), frame, xy, None)
        rows["frame_clean"], rows["ratio"] = rows["frame"], 1.0

    def check(self, B: int, shape, frame, xy) -> np.ndarray:
        """Validate one batch's parameters on the host (no device is touched): ValueError for odd frame sides or a packed side below 2, a patch
        outside the frame, a frame index outside [0, N).  shape: the frames' (N, H2, W2), or with dark_frame the packed (H, W), where
        ``frame`` is ignored.  Returns the parameter block as the device will read it."""
        return self._check(B, shape, frame, xy)[0]

    def update(self, inputs: RawInputs, shape, frame, xy) -> RawInputs:
        """Write one batch's parameters into the device block: host validation, then ONE host-to-device copy on the current stream."""
        return self._update(inputs, shape, frame, xy)

    def launch(self, inputs: RawInputs, frames, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``out`` holds clean_img and position, no
        synchronisation, capturable.  frames: (N, H2, W2) 16-bit integers on the device; with dark_frame the packed frame's (H, W), and only
        position is made."""
        if self.dark_frame:
            shape = self._shape(frames)
            res = self._outputs(inputs, inputs.device, ["position"], out)
            self._launch(inputs, None, shape, [None, None, None, res["position"].data_ptr()])
            return res
        f = self._device_frames(inputs, frames)
        _need_side_of_two(f.shape)
        res = self._outputs(inputs, f.device, ["clean_img", "position"], out)
        self._launch(inputs, f, tuple(f.shape), [None, None, res["clean_img"].data_ptr(), res["position"].data_ptr()])
        return res

    def __call__(self, frames, frame, xy, iso_ratio_idx, device=None) -> Dict[str, object]:
        """One batch of patches.  frames: (N, H2, W2) (with dark_frame: the packed frame's (H, W), and ``device`` or the current GPU is used);
        frame: (B,) indices of the long exposures (ignored with dark_frame); xy: (B, 2) patch origins (x, y); iso_ratio_idx: (B,) or one index.
        Returns {"clean_img" (B, 4, crop, crop), "position" (B, 2, crop, crop), "iso_ratio_idx" int64 (B,), "image_coord": io.image_coord(x, y)
        per patch}: the first three are ``GaussianDiffusion.sample``'s condition, the last names the files of ``io.save_generated``."""
        coords = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
        B = len(coords)
        if self.dark_frame:
            host = self.check(B, frames, None, xy)
            dev = _default_device() if device is None else cuda_device(device)
            batch: Dict[str, object] = dict(self.launch(self._eager_inputs(B, host, dev), frames))
            batch["clean_img"] = torch.zeros(B, 4, self.crop, self.crop, dtype=torch.float32, device=dev)
        else:
            host = self.check(B, tuple(frames.shape), frame, xy)
            f = frames_on_device(frames)
            dev = f.device
            batch = dict(self.launch(self._eager_inputs(B, host, dev), f))
        batch["iso_ratio_idx"] = _index_tensor(iso_ratio_idx, B, dev)
        batch["image_coord"] = [io.image_coord(x, y) for x, y in coords.tolist()]
        return batch


def balanced_sample_list(pairs: Sequence[Sequence]) -> List[Sequence]:
    """SonyTrainDataset.__init__'s resampling (dataset.py:36-83): ``(short, long, iso, ratio)`` entries grouped by (iso, int(ratio)); a group
    of 0 < n < 100 entries is repeated int(100 / n) times; the groups are concatenated in the order they were first seen."""
    groups: Dict[Tuple[int, int], list] = {}
    for entry in pairs:
        groups.setdefault((int(entry[2]), int(entry[3])), []).append(entry)
    out: list = []
    for value in groups.values():
        out.extend(int(100. / len(value)) * value if len(value) < 100 else value)
    return out
