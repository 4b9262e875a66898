"""The noise level function on the GPU: per-level moments of the noise and a Theil-Sen line of std on clean value.

The reference's value-based estimator (utils/raw_util.py:248-322: ``get_poisson_lambda``, ``get_poisson_lambda_all_images``,
``get_regression_result_all_images``) groups the noisy pixels by the clean value they sit on, takes the unbiased std of every group and fits
std against clean value with ``sklearn.linear_model.TheilSenRegressor``: slope lambda, intercept sigma.  It runs on the host there, one
full-frame pass per unique clean value.  Here it is HIP kernels (``csrc/noise_level.hip``) on tensors that stay on the device:

- ``LevelMoments(n_levels=15872, scale=15871.0, device=None)``: the exact integer table; ``.add(clean, noisy)``, ``.reset()``,
  ``.counters()``, ``.stats()`` -> ``(count, mean, std)``;
- ``level_curve(moments, below_median)`` -> ``(x, y, m)``: the fit's input, compacted on the device;
- ``theil_sen(x, y, m=None, pairs=None, max_iter=300, tol=1e-3)`` -> ``(slope, intercept, n_iter)``;
- ``get_poisson_lambda(clean, noisy)`` -> ``(lambda_, sigma_)``: the reference's function, with its cut at the median level;
- ``get_poisson_lambda_all_images(clean, noisy, moments)``: adds a frame; ``get_regression_result_all_images(moments)``: fits without a cut.

The contract (the level grid, the integer table, the curve, the spatial median) is in DESIGN.md section 15 and include/noisediff_hip.h.
Deviations from the reference, all stated there: an off-grid clean value and a non-finite noisy value are counted and left out; above 141
levels sklearn fits a random subset of 10 000 pairs and changes from run to run, this module fits ALL pairs and is repeatable (``pairs``
takes any subset, sklearn's own included); the two ``*_all_images`` functions merge a clean value across images, as their name says -- the
reference's dictionary never does (its keys are 0-dim tensors hashed by identity, and ``.extend`` on a tensor would raise).
Nothing is copied to the host.  CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import _stream

N_LEVELS, SCALE = 15872, 15871.0          # raw.WHITE - raw.BLACK + 1 codes; the packer divides by raw.WHITE - raw.BLACK
MAX_ELEMENTS = (1 << 31) - 1              # of one table: within it n sum q^2 - (sum q)^2 fits 128 bits


def _on_gpu(*ts: torch.Tensor) -> torch.device:
    for t in ts:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"the noise level function takes torch tensors, got {type(t)}")
    dev = ts[0].device
    if dev.type != "cuda":
        raise L.HipError(f"the noise level function runs on the HIP library only; tensor is on {dev} and there is no CPU path")
    if any(t.device != dev for t in ts):
        raise ValueError("all tensors must be on one device")
    return dev


class LevelMoments:
    """Per level l = rint(clean * scale): count, sum q and sum q^2 of q = rint(noisy * 2^30) + 2^32, as integers.  Integer adds commute, so the
    table is exact and does not depend on the order of the elements, on the split into ``add`` calls or on the batch.  ``table``: int64
    ``[n_levels, 4]`` (the bits of the library's uint64 words: count, sum q, low and high word of sum q^2)."""

    def __init__(self, n_levels: int = N_LEVELS, scale: float = SCALE, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.HipError(f"the noise level function runs on the HIP library only; device {dev} has no path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.n_levels, self.scale, self.device = int(n_levels), float(scale), dev
        nbytes = int(L.call("nd_level_table_bytes", self.n_levels))
        if nbytes < 0:
            raise ValueError(f"n_levels must be in [1, 2^24]; got {n_levels}")
        if not 0.0 < self.scale <= float(1 << 24):
            raise ValueError(f"scale must be in (0, 2^24]; got {scale}")
        self.table = torch.empty(nbytes // 32, 4, dtype=torch.int64, device=dev)
        self._counters = torch.empty(2, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self) -> None:
        L.call("nd_level_moments_reset", self.table.data_ptr(), self.n_levels, self._counters.data_ptr(), _stream(self.device))
        self.added = 0

    def add(self, clean: torch.Tensor, noisy: torch.Tensor) -> "LevelMoments":
        """Add every element of the pair (any shape, the same number of elements; rounded to fp32 contiguous).  The host counts what has been
        added and raises before the launch that would pass 2^31 - 1 elements: the library cannot see the total without a synchronisation."""
        dev = _on_gpu(clean, noisy)
        if dev != self.device:
            raise ValueError(f"the table is on {self.device}, the tensors on {dev}")
        if clean.numel() != noisy.numel() or clean.numel() == 0:
            raise ValueError(f"clean and noisy must hold the same positive number of elements; got {tuple(clean.shape)} and {tuple(noisy.shape)}")
        n = clean.numel()
        if self.added + n > MAX_ELEMENTS:
            raise ValueError(f"a table takes {MAX_ELEMENTS} elements; {self.added} are in and {n} more were offered")
        c, v = clean.to(torch.float32).contiguous(), noisy.to(torch.float32).contiguous()
        L.call("nd_level_moments_f32", c.data_ptr(), v.data_ptr(), n, self.scale, self.n_levels, self.table.data_ptr(), self._counters.data_ptr(),
               _stream(dev))
        self.added += n
        return self

    def counters(self) -> torch.Tensor:
        """int64 ``[2]`` on the device: the elements left out because clean is off the level grid, and because noisy is NaN, inf or >= 4."""
        return self._counters

    def stats(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(count, mean, std)`` per level: int64 and two float64 ``[n_levels]``.  std is the unbiased one, NaN below two elements."""
        dev = self.device
        count = torch.empty(self.n_levels, dtype=torch.int64, device=dev)
        mean = torch.empty(self.n_levels, dtype=torch.float64, device=dev)
        std = torch.empty(self.n_levels, dtype=torch.float64, device=dev)
        L.call("nd_level_stats_f64", self.table.data_ptr(), self.n_levels, count.data_ptr(), mean.data_ptr(), std.data_ptr(), _stream(dev))
        return count, mean, std


def level_curve(moments: LevelMoments, below_median: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The points the reference hands to sklearn: ``x`` the fp32 clean value of a level as float64, ``y`` its std, for the levels that hold an
    element, in ascending order; with ``below_median`` only those up to the lower median of these levels; levels with a NaN std dropped.
    ``x``, ``y``: float64 ``[n_levels]``, NaN past the first ``m``; ``m``: int32 0-dim.  All on the device, nothing is read back."""
    count, _, std = moments.stats()
    dev = moments.device
    x = torch.empty(moments.n_levels, dtype=torch.float64, device=dev)
    y = torch.empty(moments.n_levels, dtype=torch.float64, device=dev)
    m = torch.empty((), dtype=torch.int32, device=dev)
    L.call("nd_level_curve_f64", count.data_ptr(), std.data_ptr(), moments.n_levels, moments.scale, int(bool(below_median)), x.data_ptr(), y.data_ptr(),
           m.data_ptr(), _stream(dev))
    return x, y, m


def theil_sen(x: torch.Tensor, y: torch.Tensor, m: Optional[torch.Tensor] = None, pairs=None, max_iter: int = 300,
              tol: float = 1e-3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``TheilSenRegressor(max_iter=max_iter, tol=tol).fit(x[:m, None], y[:m])`` on ALL pairs: ``(slope, intercept, n_iter)`` as 0-dim device
    tensors (float64, float64, int64), n_iter the Weiszfeld steps taken.  ``x``, ``y``: 1-D float64, x strictly increasing; ``m``: an int32
    device tensor (the number of valid points, read on the device) or None for all of them.  ``pairs``: an int32 ``[P, 2]`` table of index
    pairs to fit instead of all pairs (a host array is uploaded).  No points give (0, 0), one point gives NaN."""
    dev = _on_gpu(x, y)
    if x.dim() != 1 or x.shape != y.shape or x.numel() < 1 or x.dtype != torch.float64 or y.dtype != torch.float64:
        raise ValueError(f"x and y must be non-empty 1-D float64 tensors of one length; got {tuple(x.shape)} {x.dtype} and {tuple(y.shape)} {y.dtype}")
    x, y = x.contiguous(), y.contiguous()
    max_m = x.numel()
    if m is None:
        m = torch.full((), max_m, dtype=torch.int32, device=dev)
    elif not isinstance(m, torch.Tensor) or m.dtype != torch.int32 or m.numel() != 1 or m.device != dev:
        raise ValueError("m must be a one-element int32 tensor on the device of x")
    n_pairs = 0
    if pairs is not None:
        if not isinstance(pairs, torch.Tensor):
            pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs, dtype=np.int32)))
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or pairs.dtype != torch.int32:
            raise ValueError(f"pairs must be an int32 [P, 2] table with P >= 1; got {tuple(pairs.shape)} {pairs.dtype}")
        pairs = pairs.to(dev).contiguous()
        n_pairs = pairs.shape[0]
    ws = torch.empty(int(L.call("nd_theil_sen_workspace_bytes", max_m, n_pairs)) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    L.call("nd_theil_sen_f64", x.data_ptr(), y.data_ptr(), m.data_ptr(), max_m, L.ptr(pairs), n_pairs, int(max_iter), float(tol), out.data_ptr(),
           ws.data_ptr(), _stream(dev))
    return out[1], out[0], out[2].to(torch.int64)


def _fit(moments: LevelMoments, below_median: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    x, y, m = level_curve(moments, below_median)
    slope, intercept, _ = theil_sen(x, y, m)
    return slope, intercept


def get_poisson_lambda(clean: torch.Tensor, noisy: torch.Tensor, n_levels: int = N_LEVELS, scale: float = SCALE) -> Tuple[torch.Tensor, torch.Tensor]:
    """utils/raw_util.py:248-280: ``(lambda_, sigma_)``, slope and intercept of the Theil-Sen line of the per-level std on the clean value over
    the levels up to the median one, as 0-dim float64 device tensors; (0, 0) when no level has two elements."""
    dev = _on_gpu(clean, noisy)
    return _fit(LevelMoments(n_levels, scale, dev).add(clean, noisy), True)


def get_poisson_lambda_all_images(clean: torch.Tensor, noisy: torch.Tensor, moments: LevelMoments) -> LevelMoments:
    """utils/raw_util.py:284-300 with the table in the dictionary's place: adds a frame and returns the table.  A clean value that several
    frames hold is ONE level here (see the module's docstring)."""
    return moments.add(clean, noisy)


def get_regression_result_all_images(moments: LevelMoments) -> Tuple[torch.Tensor, torch.Tensor]:
    """utils/raw_util.py:303-322: ``(lambda_, sigma_)`` over every level of the table, without the cut at the median."""
    return _fit(moments, False)
