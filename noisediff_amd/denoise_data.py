"""The denoiser's training batch on the GPU: what lies between ``GaussianDiffusion.sample`` and ``TrainableLSID`` in the reference's ``script.sh``.

``train_denoising.py --sub_darkshading --use_sna --trainset SyntheticNoisDiffDenoisingDataset`` turns generated noise patches into a batch with
host numpy (``SyntheticNoisDiffDenoisingDataset.__getitem__``, dataloader/dataset_denoising.py:132-168: compose, ``remove_darkshading`` :80-118,
the even-aligned crop :120-130), the flip of ``Trainer.prepare`` (models/trainer_denoising.py:100-112) and PMN's shot-noise augmentation
(``SNA_torch`` :140-166, one ``tdist.Poisson(...).sample()`` per sample in the loop :207-217).  Here all of it is ONE launch of
``csrc/denoise_batch.hip``:

- ``DarkShading``: the four Bayer maps packed once into 4-channel planes on the device, and the ``blc_mean`` table;
- ``BatchBuilder(crop, patch, shading)``: ``build(noise, clean, xy, iso, ratio, crop_xy=, flip=, wb=, K=, seed=, first_sample=, draw=)`` ->
  ``(noisy, clean_out)``, fp32 NCHW ``(B, 4, crop, crop)``; ``random_params`` draws crops, the flip and the augmentation as the reference does;
  ``capture_inputs`` / ``update`` / ``launch`` split a call into its device parameter block, the host write of that block and the bare launch,
  so the launch can sit in a captured training-step graph and replay with new parameters (the block and the scaffolding of these calls are
  ``_batch.ParamBlock`` and ``_batch.BlockBuilder``, shared with ``raw`` and ``diffusion_data``); ``plane_ptrs`` hands a launch the planes;
- ``philox_poisson(rate, seed, first_sample, draw)``: the counter-based Poisson draw alone;
- ``sna_white_balance`` / ``sna_white_balance_from_draws`` / ``sna_gain``: the augmentation's host-side parameters (plain Python, not timed).

The numerical contract (operation order, the fp64 rate, the keying of the draw) is in DESIGN.md section 11.  Deterministic: a repeated call gives
the same bits, and a sample's bits depend on (seed, first_sample + b, draw) and its own data, not on the batch around it.  CPU tensors raise
``HipError``; there is no fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._batch import BlockBuilder, ParamBlock, check_headroom, check_positive, need_gpu, per_sample, rng_key, write_rng
from ._host import _stream

WHITE_MINUS_BLACK = 15871            # 16383 - 512: the Sony sensor's white point minus its black level
HIGH_ISO = 1600                      # above it the high-ISO pair of dark-shading maps applies
# the third-stop ISO series the reference's noise-parameter table covers; there Kmax = 9.563e-4 * iso
TABLE_ISOS = (50, 64, 80, 100, 125, 160, 200, 250, 320, 400, 500, 640, 800, 1000, 1250, 1600, 2000, 2500, 3200, 4000, 5000, 6400, 8000, 10000,
              12800, 16000, 20000, 25600)
_RNG_WORDS, _TABLE_WORDS, _SNA_WORDS = 8, 12, 8      # 32-bit words: the {seed, first_sample, draw} triple (padded), nd_denoise_sample, wb[4] + K
_WHAT = "denoise_data runs on the HIP library"       # need_gpu's half of the "no CPU path" message


# ----------------------------------------------------------------------------- host-side parameters of the augmentation

def sna_gain(iso: int, jitter: float) -> float:
    """K of SNA_torch (trainer_denoising.py:144-152): the system gain at ``iso`` times (1 + jitter), jitter ~ U(-0.01, 0.01)."""
    iso = int(iso)
    if iso in TABLE_ISOS:
        return 9.563e-4 * iso * (1.0 + float(jitter))
    return 0.0009546 * iso * (1.0 + float(jitter)) - 0.00193


def sna_white_balance_from_draws(r_idx: int, gate: int, n_g, n_r, n_b) -> torch.Tensor:
    """get_aug_param_torch (trainer_denoising.py:115-138) as a function of its five draws: (B, 4) fp32 gains in (R, G, B, G) order.

    r_idx = randint(2), gate = randint(4) (0: no augmentation, every gain 0), n_g / n_r / n_b: the three randn(B) in the order drawn.
    sigma = 0.25 (r_idx + 1); g = clamp(sigma n_g, 0, 4 sigma); r, b = clamp((1 + sigma n) (1 + g) - 1, 0, 4 sigma).  The reference then
    divides (1 + gain) by 1 + min(min(r, g, b), 0), which is 1 because every gain was clamped at 0, and subtracts 1: the fp32 round trip
    (1 + gain) - 1 is kept, since it moves the last bit of a gain."""
    n_g, n_r, n_b = (torch.as_tensor(n, dtype=torch.float32).reshape(-1) for n in (n_g, n_r, n_b))
    if not (n_g.numel() == n_r.numel() == n_b.numel()):
        raise ValueError("n_g, n_r and n_b must have one length")
    if r_idx not in (0, 1):
        raise ValueError(f"r_idx is randint(2): 0 or 1, got {r_idx}")
    sigma = int(r_idx) * 0.25 + 0.25
    if gate:
        g = torch.clamp(n_g * sigma, 0, 4 * sigma)
        r = torch.clamp((1 + n_r * sigma) * (1 + g) - 1, 0, 4 * sigma)
        b = torch.clamp((1 + n_b * sigma) * (1 + g) - 1, 0, 4 * sigma)
    else:
        r = g = b = torch.zeros_like(n_g)
    r, g, b = ((1 + t) / 1 - 1 for t in (r, g, b))
    return torch.stack((r, g, b, g), dim=1)


def sna_white_balance(B: int) -> torch.Tensor:
    """The (B, 4) gains of one training step, drawn with get_aug_param_torch's calls in its order: np.random.randint(2), np.random.randint(4),
    then, unless that gate is 0, three torch.randn(B) (green, red, blue)."""
    r_idx = int(np.random.randint(2))
    gate = int(np.random.randint(4))
    if gate:
        n_g, n_r, n_b = torch.randn(B), torch.randn(B), torch.randn(B)
    else:
        n_g = n_r = n_b = torch.zeros(B)
    return sna_white_balance_from_draws(r_idx, gate, n_g, n_r, n_b)


# ----------------------------------------------------------------------------- device helpers

def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def philox_poisson(rate: torch.Tensor, seed: int = 0, first_sample: int = 0, draw: int = 0) -> torch.Tensor:
    """Poisson counts (fp32, the shape of ``rate``) with rate ``rate[b, ...]``: the draw of the shot-noise augmentation alone.  ``rate`` is
    (B, ...) on a GPU; element i of sample b is keyed by (seed, i, first_sample + b, draw), so a sample's counts do not depend on B."""
    if not isinstance(rate, torch.Tensor) or rate.dim() < 1 or rate.numel() == 0:
        raise ValueError("rate must be a non-empty (B, ...) tensor")
    dev = need_gpu(rate, what=_WHAT)
    r = _f32(rate)
    out = torch.empty_like(r)
    B = r.shape[0]
    L.call("nd_philox_poisson_f32", r.data_ptr(), out.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample), int(draw), B, r.numel() // B,
           _stream(dev))
    return out


class DarkShading:
    """The dark-shading resources of ``--sub_darkshading`` on the device.

    ds_k_high, ds_b_high, ds_k_low, ds_b_low: the Bayer maps (2H, 2W) of raw_util.load_darkshading, numpy or torch; blc_mean: {iso: level}.
    Each map is packed once into planes (4, H, W) in pack_np_raw's channel order, so channel c of packed pixel (Y, X) reads plane[c, Y, X]."""

    def __init__(self, ds_k_high, ds_b_high, ds_k_low, ds_b_low, blc_mean: Dict[int, float], device):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.HipError(f"DarkShading lives on a GPU; got device {device} and there is no CPU path")
        maps = [torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m) for m in (ds_k_high, ds_b_high, ds_k_low, ds_b_low)]
        shape = tuple(maps[0].shape)
        if any(m.dim() != 2 or tuple(m.shape) != shape for m in maps) or shape[0] % 2 or shape[1] % 2 or min(shape) < 2:
            raise ValueError(f"the four dark-shading maps must be Bayer maps (2H, 2W) of one shape; got {[tuple(m.shape) for m in maps]}")
        self.device = device
        self.H, self.W = shape[0] // 2, shape[1] // 2
        self.blc_mean = {int(k): float(v) for k, v in dict(blc_mean).items()}
        planes = []
        for m in maps:
            bayer = _f32(m.to(device))
            p = torch.empty(4, self.H, self.W, dtype=torch.float32, device=device)
            L.call("nd_pack_darkshading_f32", bayer.data_ptr(), p.data_ptr(), shape[0], shape[1], _stream(device))
            planes.append(p)
        torch.cuda.current_stream(device).synchronize()      # `bayer` is freed here: the pack must have read it
        self.k_high, self.b_high, self.k_low, self.b_low = planes

    def black_level(self, iso: int) -> float:
        if int(iso) not in self.blc_mean:
            raise ValueError(f"blc_mean has no entry for ISO {iso}")
        return self.blc_mean[int(iso)]


def plane_ptrs(shading: Optional[DarkShading], device: torch.device, other: str = "frames"):
    """([k_high, b_high, k_low, b_low] as pointers, H, W) of the planes on ``device``; four NULLs and 0, 0 for None."""
    if shading is None:
        return [None] * 4, 0, 0
    if shading.device != device:
        raise ValueError(f"the shading planes are on {shading.device}, the {other} on {device}")
    return [shading.k_high.data_ptr(), shading.b_high.data_ptr(), shading.k_low.data_ptr(), shading.b_low.data_ptr()], shading.H, shading.W


class BatchInputs(ParamBlock):
    """The device parameter block of one ``BatchBuilder.launch``: the {seed, first_sample, draw} triple, the per-sample table and the
    augmentation columns in ONE int32 buffer, written by ``BatchBuilder.update`` with one copy.  A captured launch reads it at replay."""
    DTYPE, HEAD, PER_SAMPLE = np.int32, _RNG_WORDS, _TABLE_WORDS + _SNA_WORDS

    def __init__(self, B: int, device: torch.device):
        super().__init__(B, device, self.DTYPE, self.HEAD, self.PER_SAMPLE)

    rng_ptr = property(lambda self: self.ptr(0))
    table_ptr = property(lambda self: self.ptr(_RNG_WORDS))
    sna_ptr = property(lambda self: self.ptr(_RNG_WORDS + self.B * _TABLE_WORDS))


class BatchBuilder(BlockBuilder):
    """Builds (noisy, clean) training batches of ``crop`` x ``crop`` from ``patch`` x ``patch`` generated patches.

    shading: a ``DarkShading`` (``--sub_darkshading``) or None.  The reference's hard-coded 512 * 2 shading window is ``patch`` here."""
    Inputs = BatchInputs

    def __init__(self, crop: int, patch: int, shading: Optional[DarkShading] = None):
        crop, patch = int(crop), int(patch)
        if crop <= 0 or patch <= 0 or crop > patch or crop % 2 or patch % 2:
            raise ValueError(f"crop and patch must be positive and even with crop <= patch; got crop={crop}, patch={patch}")
        if shading is not None and (shading.H < patch or shading.W < patch):
            raise ValueError(f"the shading planes ({shading.H} x {shading.W}) are smaller than the patch ({patch})")
        self.crop, self.patch, self.shading = crop, patch, shading

    # ------------------------------------------------------------------ parameters
    def random_params(self, B: int, iso: Sequence[int]) -> Dict[str, object]:
        """crop_xy, flip, wb and K of one step, drawn as the reference draws them and in its order: per sample the crop's x then y
        (np.random.randint, rounded down to even; dataset_denoising.py:123-126), one flip for the batch (np.random.randint(0, 2),
        trainer_denoising.py:108), the white-balance gains (``sna_white_balance``), and for every sample whose gains are not all zero the
        gain's jitter (np.random.uniform(-0.01, 0.01), :150-152)."""
        iso = [int(i) for i in iso]
        if len(iso) != B:
            raise ValueError(f"iso must have B={B} entries")
        span = self.patch - self.crop + 1
        crop_xy = []
        for _ in range(B):
            x = int(np.random.randint(0, span)) // 2 * 2
            y = int(np.random.randint(0, span)) // 2 * 2
            crop_xy.append((x, y))
        flip = [int(np.random.randint(0, 2))] * B
        wb = sna_white_balance(B)
        K = [sna_gain(iso[b], np.random.uniform(low=-0.01, high=+0.01) if float(wb[b].abs().max()) != 0 else 0.0) for b in range(B)]
        return {"crop_xy": crop_xy, "flip": flip, "wb": wb, "K": K}

    def _host_block(self, host: np.ndarray, B: int, xy, iso, ratio, crop_xy, flip, wb, K, seed: int, first_sample: int, draw: int) -> bool:
        """Validate one call's parameters and write them into ``host`` (the layout of BatchInputs.block).  Returns whether SNA is on."""
        P, c = self.patch, self.crop
        xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
        crop_xy = np.asarray(crop_xy, dtype=np.int64).reshape(-1, 2)
        iso = np.asarray(iso, dtype=np.int64).reshape(-1)
        ratio = np.asarray(ratio, dtype=np.float64).reshape(-1)
        flip = per_sample(0 if flip is None else flip, B, np.int64)
        if not (len(xy) == len(crop_xy) == len(iso) == len(ratio) == B):
            raise ValueError(f"xy, crop_xy, iso and ratio must have B={B} rows")
        if (crop_xy % 2).any() or (crop_xy < 0).any() or (crop_xy > P - c).any():
            raise ValueError(f"crop offsets must be even and in [0, {P - c}]; got {crop_xy.tolist()}")
        check_positive(ratio, "ratio")
        write_rng(host[:_RNG_WORDS], seed, first_sample, draw)
        blc = np.zeros(B)
        if self.shading is not None:
            if (xy < 0).any() or (xy[:, 0] > self.shading.W - P).any() or (xy[:, 1] > self.shading.H - P).any():
                raise ValueError(f"a patch at {xy.tolist()} leaves the {self.shading.H} x {self.shading.W} shading planes")
            blc = np.array([self.shading.black_level(i) for i in iso])
        if (np.abs(xy) >= 2 ** 31).any():
            raise ValueError("patch origin out of range")
        t = host[_RNG_WORDS:_RNG_WORDS + B * _TABLE_WORDS].reshape(B, _TABLE_WORDS)
        t[:, 0:2], t[:, 2:4], t[:, 4], t[:, 5] = xy, crop_xy, flip != 0, iso > HIGH_ISO
        tf = t.view(np.float32)
        tf[:, 6], tf[:, 7], tf[:, 8] = iso, ratio, blc
        s = host[_RNG_WORDS + B * _TABLE_WORDS:].reshape(B, _SNA_WORDS).view(np.float32)
        s[:] = 0
        if wb is None:
            return False
        wb = (wb.detach().cpu().numpy() if isinstance(wb, torch.Tensor) else np.asarray(wb)).astype(np.float32).reshape(-1, 4)
        if K is None:
            raise ValueError("wb needs K (sna_gain)")
        K = per_sample(K, B)
        if len(wb) != B:
            raise ValueError(f"wb must be (B={B}, 4)")
        if not (wb >= 0).all():
            raise ValueError("white-balance gains must be non-negative")
        K32 = K.astype(np.float32)
        check_positive(K32, "the gain K", got=K)
        top = WHITE_MINUS_BLACK * wb.max(axis=1).astype(np.float64) / (ratio.astype(np.float32).astype(np.float64) * K32.astype(np.float64))
        check_headroom(top, "15871 * max(wb) / (ratio * K)")
        s[:, 0:4], s[:, 4] = wb, K32
        return True

    def check(self, B: int, xy, iso, ratio, crop_xy, flip=None, wb=None, K=None, seed: int = 0, first_sample: int = 0,
              draw: int = 0) -> Tuple[np.ndarray, bool]:
        """Validate one step's parameters on the host (no device is touched): ValueError for K <= 0, negative gains, odd or out-of-range crop
        offsets, a patch outside the shading planes, or 15871 max(wb) / (ratio K) >= 2**24.  Returns (the parameter block as the device will
        read it, whether the augmentation is on)."""
        return self._check(B, xy, iso, ratio, crop_xy, flip, wb, K, seed, first_sample, draw)

    def update(self, inputs: BatchInputs, xy, iso, ratio, crop_xy, flip=None, wb=None, K=None, seed: int = 0, first_sample: int = 0,
               draw: int = 0) -> BatchInputs:
        """Write one step's parameters into the device block: host validation, then ONE host-to-device copy on the current stream.  A captured
        ``launch`` keeps the choice between augmentation and none that was in force at capture: switch it off per sample with zero gains."""
        return self._update(inputs, xy, iso, ratio, crop_xy, flip, wb, K, seed, first_sample, draw)

    # ------------------------------------------------------------------ the launch
    def _check_images(self, noise: torch.Tensor, clean: torch.Tensor) -> int:
        if not (isinstance(noise, torch.Tensor) and isinstance(clean, torch.Tensor)):
            raise TypeError("noise and clean must be torch tensors")
        want = (4, self.patch, self.patch)
        if noise.dim() != 4 or noise.shape != clean.shape or tuple(noise.shape[1:]) != want or noise.shape[0] < 1:
            raise ValueError(f"noise and clean must be (B, 4, {self.patch}, {self.patch}); got {tuple(noise.shape)} and {tuple(clean.shape)}")
        return noise.shape[0]

    def launch(self, inputs: BatchInputs, noise: torch.Tensor, clean: torch.Tensor, noisy: Optional[torch.Tensor] = None,
               clean_out: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
               counts_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``noisy`` and ``clean_out`` are given, no
        synchronisation, capturable.  noise, clean: fp32 contiguous (B, 4, patch, patch)."""
        B = self._check_images(noise, clean)
        dev = need_gpu(noise, clean, what=_WHAT)
        if B != inputs.B or dev != inputs.device:
            raise ValueError(f"the parameter block is for B={inputs.B} on {inputs.device}; got B={B} on {dev}")
        if noise.dtype != torch.float32 or clean.dtype != torch.float32 or not noise.is_contiguous() or not clean.is_contiguous():
            raise ValueError("launch takes fp32 contiguous tensors (the builder's call converts)")
        shape = (B, 4, self.crop, self.crop)
        noisy, clean_out = self._output("noisy", noisy, shape, dev), self._output("clean_out", clean_out, shape, dev)
        self._output("counts", counts, shape, dev, make=False)
        self._output("counts_out", counts_out, shape, dev, make=False)
        maps, mh, mw = plane_ptrs(self.shading, dev, "batch")
        L.call("nd_denoise_batch_f32", noise.data_ptr(), clean.data_ptr(), *maps, mh, mw, inputs.table_ptr,
               inputs.sna_ptr if inputs.use_sna else None, inputs.rng_ptr if inputs.use_rng else None, *rng_key(inputs.host[:_RNG_WORDS]),
               L.ptr(counts), L.ptr(counts_out), noisy.data_ptr(), clean_out.data_ptr(), B, self.patch, self.crop, self.crop, _stream(dev))
        return noisy, clean_out

    def __call__(self, noise: torch.Tensor, clean: torch.Tensor, xy, iso, ratio, crop_xy, flip=None, wb=None, K=None, seed: int = 0,
                 first_sample: int = 0, draw: int = 0, counts: Optional[torch.Tensor] = None, return_counts: bool = False):
        """One batch.  noise, clean: (B, 4, patch, patch) on a GPU (``clean`` is the patch of pack_raw's frame, not yet clipped); xy: (B, 2)
        patch origins (x, y) in the packed frame (the coord of the file name); iso, ratio: (B,); crop_xy: (B, 2) even offsets (x, y) inside
        the patch; flip: (B,) or one 0/1; wb: (B, 4) gains (None: no --use_sna) with K: (B,) or one gain; seed / first_sample / draw key the
        Poisson draw; counts: (B, 4, crop, crop) counts to use instead of drawing.  Returns (noisy, clean_out[, counts used])."""
        B = self._check_images(noise, clean)
        host, use_sna = self.check(B, xy, iso, ratio, crop_xy, flip, wb, K, seed, first_sample, draw)
        if counts is not None and (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (B, 4, self.crop, self.crop)):
            raise ValueError(f"counts must be a (B, 4, {self.crop}, {self.crop}) tensor")
        dev = need_gpu(noise, clean, what=_WHAT) if counts is None else need_gpu(noise, clean, counts, what=_WHAT)
        counts = None if counts is None else _f32(counts)
        inputs = self._eager_inputs(B, host, dev, use_rng=False, use_sna=use_sna)
        used = torch.empty(B, 4, self.crop, self.crop, dtype=torch.float32, device=dev) if return_counts else None
        noisy, clean_out = self.launch(inputs, _f32(noise), _f32(clean), counts=counts, counts_out=used)
        return (noisy, clean_out, used) if return_counts else (noisy, clean_out)
