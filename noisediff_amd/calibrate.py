"""The physics-based noise model's per-ISO table row from dark (bias) frames, on the GPU: dark frames -> row -> ``CameraNoiseModel``.

ELD and PMN calibrate on the host: row means give the row noise, ``scipy.stats.ppcc_max`` of what is left finds the Tukey-lambda shape and
``scipy.stats.probplot`` its scale ``sigTL`` and the Gaussian twin ``sigGs``.  Here the uint16 frames stay on the device and
``csrc/calibrate.hip`` does the arithmetic (include/noisediff_hip.h); ``torch.sort`` orders each frame's residual once.
Units are codes (DN); channels and the Bayer cell are ``raw``'s; a packed frame is ``h x w = H2 / 2 x W2 / 2`` and holds ``n = 4 h w`` values.

- ``DarkStack(H2, W2, device).add(frames)``: exact per-pixel integer sums; ``.count``, ``.sums``, ``.mean()``;
- ``row_sums(frames, black, subtract, stack)`` -> int64 ``(N, 4, h)`` and ``residuals(frames, R, black, subtract, stack)`` -> float64 ``(N, n)``:
  every pixel as the integer ``t = D code - P`` (``subtract="black"``: ``D = 1, P = black``; ``"mean"``: ``D = N, P`` the stack's sum), its exact
  row sums ``R`` per (channel, packed row) and the correctly rounded deviation ``x = (t w - R) / (w D)`` from its row's mean;
- ``probplot(xs, lam=None)`` -> ``(slope, intercept, r)`` and ``ppcc_max(xs, lo, hi, xtol, max_eval)`` -> ``(lam, r, n_eval)`` for SORTED values
  ``(N, n)``: the probability plot against the unit Tukey-lambda (or, without ``lam``, the normal) quantiles of scipy's order-statistic medians
  and Brent's bounded maximisation of its correlation, per frame, all on the device; ``quantiles(n, lam=None)``: those theoretical quantiles;
- ``calibrate_dark_frames(frames, black=512, subtract="black")`` -> ``CalibrationResult`` (per-frame device tensors; ``.cpu()`` a dict);
- ``table_row(result, K, q, row="corrected")`` -> one row with ``physics_noise.TABLE_KEYS``; ``{iso: row}`` is a ``CameraNoiseModel``'s table.

Deviations from PMN, all in DESIGN.md section 23: the row unit is (channel, packed row), what ``physics_noise`` draws its row variate for;
``sigR_pmn`` is the spread of the row means about their CHANNEL's mean (the bias is a parameter of its own); ``sigR`` has the read noise's
leakage into a mean of ``w`` pixels removed, ``sigR^2 = sigR_pmn^2 - V_x / (w - 1)``; the shape is searched on a bounded bracket inside
``(-0.5, inf)``; ``subtract="mean"`` removes the fixed pattern exactly and its factor ``(N - 1) / N`` on every variance is undone here
(``sqrt(N / (N - 1))`` on the scales).  The gain ``K`` and the quantisation step ``q`` are the caller's.  CPU tensors raise ``HipError``; there
is no fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._batch import cuda_device, need_gpu
from ._host import _stream
from .physics_noise import TABLE_KEYS
from .raw import BLACK, frame_shape, frames_on_device

MAX_FRAMES = 32767                    # 32767 * 65535 < 2^31: a stack's sums stay inside int32
MAX_SIDE = 32768                      # packed rows and columns: within it the row statistics fit 128 bits
LO, HI, XTOL, MAX_EVAL = -0.45, 0.5, 1e-6, 32
_WHAT = "dark frames are calibrated on the HIP library"
_SUBTRACT = ("black", "mean")


def _check_shape(shape) -> Tuple[int, int, int]:
    """(N, H2, W2) of a stack the calibration takes: even sides (``raw.frame_shape``), 1 <= N <= 32767, 2 <= h, w <= 32768, so n >= 16 >= 3."""
    N, H2, W2 = frame_shape(shape)
    if N > MAX_FRAMES:
        raise ValueError(f"a stack takes {MAX_FRAMES} frames (N * 65535 stays inside int32); got {N}")
    if not (4 <= H2 <= 2 * MAX_SIDE and 4 <= W2 <= 2 * MAX_SIDE):
        raise ValueError(f"the packed frame must be 2 .. {MAX_SIDE} rows and columns (n = 4 h w >= 3 values per frame); got frames {H2} x {W2}")
    return N, H2, W2


def _indexed(dev: torch.device) -> torch.device:
    """``cuda`` without an index is the current device: tensors report theirs with one."""
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _check_black(black) -> int:
    if isinstance(black, bool) or not float(black).is_integer() or not 0 <= float(black) <= 65535:
        raise ValueError(f"black is subtracted in the integer domain: an integer in [0, 65535]; got {black!r}")
    return int(black)


def check_search(lo: float = LO, hi: float = HI, xtol: float = XTOL, max_eval: int = MAX_EVAL) -> Tuple[float, float, float, int]:
    """The search's parameters, checked on the host: -0.5 < lo < hi (the unit variate's variance is infinite at -0.5), xtol > 0,
    3 <= max_eval <= 64."""
    lo, hi, xtol = float(lo), float(hi), float(xtol)
    if not lo < hi or not math.isfinite(hi):
        raise ValueError(f"the bracket needs lo < hi; got {lo}, {hi}")
    if not lo > -0.5:
        raise ValueError(f"lo must be above -0.5, where the Tukey-lambda variance becomes infinite; got {lo}")
    if not 0.0 < xtol < math.inf:
        raise ValueError(f"xtol must be positive; got {xtol}")
    if int(max_eval) != max_eval or not 3 <= int(max_eval) <= 64:
        raise ValueError(f"max_eval must be in [3, 64]; got {max_eval}")
    return lo, hi, xtol, int(max_eval)


def _out(name: str, t: Optional[torch.Tensor], shape, dtype, dev: torch.device) -> torch.Tensor:
    """An output the caller may bring: at least ``shape[0]`` leading entries of the trailing shape (what lies past them is not written)."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != len(shape)
            or t.shape[0] < shape[0] or tuple(t.shape[1:]) != tuple(shape[1:])):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor on {dev} of shape {tuple(shape)} (or longer along the first axis)")
    return t


class DarkStack:
    """T[y, x] = sum over the added frames of their code at (y, x), as integers: exact, and the same bits however the frames are split over
    ``add`` calls.  ``sums``: int32 ``(H2, W2)``; ``count``: the frames added so far, at most 32767."""

    def __init__(self, H2: int, W2: int, device=None):
        _, self.H2, self.W2 = _check_shape((1, H2, W2))
        if device is None:
            if not torch.cuda.is_available():
                raise L.HipError(f"{_WHAT} only; no GPU is visible and there is no CPU path")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = _indexed(cuda_device(device))
        self.sums = torch.zeros(self.H2, self.W2, dtype=torch.int32, device=self.device)
        self.count = 0

    def add(self, frames) -> "DarkStack":
        """Add a frame ``(H2, W2)`` or a stack ``(N, H2, W2)`` (numpy uint16, or a 16-bit integer tensor on the stack's device)."""
        N, H2, W2 = frame_shape(tuple(frames.shape))
        if (H2, W2) != (self.H2, self.W2):
            raise ValueError(f"the stack holds {self.H2} x {self.W2} frames; got {H2} x {W2}")
        if self.count + N > MAX_FRAMES:
            raise ValueError(f"a stack takes {MAX_FRAMES} frames (N * 65535 stays inside int32); {self.count} are in and {N} more were offered")
        f = frames_on_device(frames, self.device)
        if f.device != self.device:
            raise ValueError(f"the stack is on {self.device}, the frames on {f.device}")
        L.call("nd_dark_stack_add_u16", f.data_ptr(), N, H2, W2, self.sums.data_ptr(), _stream(self.device))
        self.count += N
        return self

    def mean(self) -> torch.Tensor:
        """The mean dark frame, float64 ``(H2, W2)``: one IEEE division per pixel."""
        if self.count < 1:
            raise ValueError("the stack is empty")
        out = torch.empty(self.H2, self.W2, dtype=torch.float64, device=self.device)
        L.call("nd_dark_stack_mean_f64", self.sums.data_ptr(), self.H2, self.W2, self.count, out.data_ptr(), _stream(self.device))
        return out


def check_subtract(shape, black=BLACK, subtract: str = "black", stack: Optional[DarkStack] = None) -> Tuple[int, int, int, int, int]:
    """What is subtracted, checked on the host (no device is touched): ``(N, H2, W2, black, D)``.  ValueError for odd or too small sides, more
    than 32767 frames, a non-integer black, an unknown ``subtract``, and with ``"mean"`` a single frame or a stack whose count or shape is not
    that of ``frames``."""
    N, H2, W2 = _check_shape(shape)
    black = _check_black(black)
    if subtract not in _SUBTRACT:
        raise ValueError(f"subtract is 'black' or 'mean'; got {subtract!r}")
    if subtract == "black":
        if stack is not None:
            raise ValueError("a DarkStack is read with subtract='mean' only")
        return N, H2, W2, black, 1
    if N < 2:
        raise ValueError("subtract='mean' needs two frames at least: one frame minus its own mean is zero")
    if stack is not None and (stack.count != N or (stack.H2, stack.W2) != (H2, W2)):
        raise ValueError(f"the DarkStack must hold these {N} frames of {H2} x {W2}; it holds {stack.count} of {stack.H2} x {stack.W2}")
    return N, H2, W2, black, N


def _prepare(frames, black, subtract: str, stack: Optional[DarkStack]):
    N, H2, W2, black, D = check_subtract(tuple(frames.shape), black, subtract, stack)
    f = frames_on_device(frames)
    if subtract == "mean":
        if stack is None:
            stack = DarkStack(H2, W2, f.device).add(f)
        elif stack.device != f.device:
            raise ValueError(f"the stack is on {stack.device}, the frames on {f.device}")
    return f, N, H2, W2, black, D, (stack.sums if subtract == "mean" else None)


def row_sums(frames, black=BLACK, subtract: str = "black", stack: Optional[DarkStack] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``R[n, c, Y] = sum over X of t``, int64 ``(N, 4, h)``, exact.  ``out``: where to write (N entries of a longer tensor are fine)."""
    f, N, H2, W2, black, _, T = _prepare(frames, black, subtract, stack)
    R = _out("out", out, (N, 4, H2 // 2), torch.int64, f.device)
    L.call("nd_calib_row_sums_i64", f.data_ptr(), N, H2, W2, L.ptr(T), black, R.data_ptr(), _stream(f.device))
    return R


def residuals(frames, R: torch.Tensor, black=BLACK, subtract: str = "black", stack: Optional[DarkStack] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x = (double)(t w - R) / (double)(w D)``, float64 ``(N, n)`` in (channel, row, column) order: a pixel's deviation from the mean of its
    (channel, packed row), one correctly rounded division.  ``R``: ``row_sums`` of the same arguments."""
    f, N, H2, W2, black, _, T = _prepare(frames, black, subtract, stack)
    h, w = H2 // 2, W2 // 2
    _out("R", R, (N, 4, h), torch.int64, f.device)
    x = _out("out", out, (N, 4 * h * w), torch.float64, f.device)
    L.call("nd_calib_residual_f64", f.data_ptr(), N, H2, W2, L.ptr(T), black, R.data_ptr(), x.data_ptr(), _stream(f.device))
    return x


def _sorted_values(xs: torch.Tensor) -> Tuple[torch.Tensor, torch.device, int, int]:
    if not isinstance(xs, torch.Tensor):
        raise TypeError(f"the probability plot takes a torch tensor; got {type(xs)}")
    if xs.dim() == 1:
        xs = xs[None]
    if xs.dim() != 2 or xs.dtype != torch.float64 or not 1 <= xs.shape[0] <= MAX_FRAMES or xs.shape[1] < 3:
        raise ValueError(f"xs must be float64 (N, n) sorted values with 1 <= N <= {MAX_FRAMES} and n >= 3; got {tuple(xs.shape)} {xs.dtype}")
    dev = need_gpu(xs, what=_WHAT)
    return xs.contiguous(), dev, xs.shape[0], xs.shape[1]


def _workspace(N: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(int(L.call("nd_ppcc_workspace_bytes", N)) // 8, dtype=torch.float64, device=dev)


def _probplot(xs: torch.Tensor, lam: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    xs, dev, N, n = _sorted_values(xs)
    if lam is not None:
        if not isinstance(lam, torch.Tensor) or lam.dtype != torch.float64 or lam.numel() != N or lam.device != dev:
            raise ValueError(f"lam must be a float64 tensor of N = {N} shapes on {dev}")
        lam = lam.contiguous()
    o = _out("out", out, (N, 6), torch.float64, dev)
    L.call("nd_probplot_f64", xs.data_ptr(), N, n, 0 if lam is None else 1, L.ptr(lam), o.data_ptr(), _workspace(N, dev).data_ptr(), _stream(dev))
    return o


def probplot(xs: torch.Tensor, lam: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``scipy.stats.probplot(x, sparams=(lam,), dist="tukeylambda")``'s ``(slope, intercept, r)`` for sorted ``xs (N, n)`` and one shape per
    frame (a float64 device tensor), or the normal probability plot ``scipy.stats.probplot(x)`` without ``lam``.  Three ``(N,)`` float64 views of
    ``out`` (``(N, 6)``: slope, intercept, r, mean, ddof-0 variance, 0)."""
    o = _probplot(xs, lam, out)
    N = 1 if xs.dim() == 1 else xs.shape[0]
    return o[:N, 0], o[:N, 1], o[:N, 2]


def ppcc_max(xs: torch.Tensor, lo: float = LO, hi: float = HI, xtol: float = XTOL, max_eval: int = MAX_EVAL,
             out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``scipy.stats.ppcc_max(x, dist="tukeylambda")`` with a bounded bracket, for sorted ``xs (N, n)``: the shape ``lam`` in ``(lo, hi)`` that
    maximises the probability plot's correlation, by Brent's bounded minimisation of ``1 - r(lam)``
    (``scipy.optimize.minimize_scalar(method="bounded", options={"xatol": xtol})``), every frame searched on the device at once.  Returns
    ``(lam, r, n_eval)``: float64, float64, int64 ``(N,)``.  A frame whose objective is NaN (a constant frame) gets NaN ``lam`` and ``r``; a
    frame that used all ``max_eval`` evaluations has ``n_eval == max_eval`` and its best point so far."""
    lo, hi, xtol, max_eval = check_search(lo, hi, xtol, max_eval)
    xs, dev, N, n = _sorted_values(xs)
    o = _out("out", out, (N, 3), torch.float64, dev)
    L.call("nd_ppcc_max_f64", xs.data_ptr(), N, n, lo, hi, xtol, max_eval, o.data_ptr(), _workspace(N, dev).data_ptr(), _stream(dev))
    return o[:N, 0], o[:N, 1], o[:N, 2].to(torch.int64)


def quantiles(n: int, lam: Optional[float] = None, device=None) -> torch.Tensor:
    """The theoretical quantiles of scipy's ``n`` order-statistic medians as the probability plots evaluate them: unit Tukey-lambda of shape
    ``lam``, standard normal without one.  float64 ``(n,)`` on the device."""
    if int(n) < 3:
        raise ValueError(f"n must be 3 at least; got {n}")
    if device is None and not torch.cuda.is_available():
        raise L.HipError(f"{_WHAT} only; no GPU is visible and there is no CPU path")
    dev = _indexed(cuda_device("cuda" if device is None else device))
    q = torch.empty(int(n), dtype=torch.float64, device=dev)
    L.call("nd_calib_quantiles_f64", int(n), 0 if lam is None else 1, 0.0 if lam is None else float(lam), q.data_ptr(), _stream(dev))
    return q


_FIELDS = ("lam", "sigTL", "uTL", "rTL", "sigGs", "uGs", "rGs", "sigR", "sigR_pmn", "bias", "n_eval")


class CalibrationResult:
    """Per-frame estimates as float64 device tensors ``(N,)`` (``bias``: ``(N, 4)``, ``n_eval``: int64): ``lam`` the Tukey-lambda shape with its
    correlation ``rTL``, scale ``sigTL`` and location ``uTL``; ``sigGs, uGs, rGs`` the same of the normal plot; ``sigR`` the row noise with the
    read noise's leakage removed and ``sigR_pmn`` without that correction; ``bias`` the channels' mean above what was subtracted."""

    def __init__(self, **fields: torch.Tensor):
        for k in _FIELDS:
            setattr(self, k, fields[k])

    def cpu(self) -> Dict[str, np.ndarray]:
        return {k: getattr(self, k).cpu().numpy() for k in _FIELDS}


def calibrate_dark_frames(frames, black=BLACK, subtract: str = "black", lo: float = LO, hi: float = HI, xtol: float = XTOL,
                          max_eval: int = MAX_EVAL, stack: Optional[DarkStack] = None) -> CalibrationResult:
    """Dark frames ``(N, H2, W2)`` (numpy uint16 or a 16-bit integer device tensor) to per-frame estimates.  Nothing is read back.

    ``subtract="black"``: the level ``black`` goes off every code.  ``"mean"``: the stack's own mean frame does (``stack``: a ``DarkStack`` over
    exactly these frames, made here when not given), which removes the fixed pattern, dark shading and the black level's error exactly and
    shrinks every variance by ``(N - 1) / N``; the four scales are multiplied by ``sqrt(N / (N - 1))`` here to undo it, and ``bias`` is then a
    frame's offset from the stack's mean."""
    lo, hi, xtol, max_eval = check_search(lo, hi, xtol, max_eval)
    N, H2, W2, black, D = check_subtract(tuple(frames.shape), black, subtract, stack)
    f = frames_on_device(frames)
    if subtract == "mean" and stack is None:
        stack = DarkStack(H2, W2, f.device).add(f)
    dev, h, w = f.device, H2 // 2, W2 // 2
    R = row_sums(f, black, subtract, stack)
    xs = torch.sort(residuals(f, R, black, subtract, stack), dim=1).values
    gauss = _probplot(xs, None)
    rows = torch.empty(N, 8, dtype=torch.float64, device=dev)
    L.call("nd_calib_row_stats_f64", R.data_ptr(), N, h, w, D, gauss.data_ptr() + 4 * 8, 6, rows.data_ptr(), _stream(dev))
    lam, _, n_eval = ppcc_max(xs, lo, hi, xtol, max_eval)
    tukey = _probplot(xs, lam)
    undo = math.sqrt(N / (N - 1.0)) if subtract == "mean" else 1.0
    return CalibrationResult(lam=lam, sigTL=tukey[:, 0] * undo, uTL=tukey[:, 1], rTL=tukey[:, 2], sigGs=gauss[:, 0] * undo, uGs=gauss[:, 1],
                             rGs=gauss[:, 2], sigR=rows[:, 1] * undo, sigR_pmn=rows[:, 0] * undo, bias=rows[:, 2:6], n_eval=n_eval)


def table_row(result, K: float, q: float, row: str = "corrected") -> Dict[str, float]:
    """One ``CameraNoiseModel`` row from a ``CalibrationResult`` (or its ``.cpu()`` dict): ``Kmax = K`` and ``q`` are the caller's (gain
    calibration needs flat fields); ``lam, sigGs, sigTL, sigR, bias`` are the means over the frames (``bias`` over frames and channels) and the
    ``...sig`` their ddof-1 standard deviations over the frames, 0 for a single frame.  ``row``: ``"corrected"`` takes ``sigR``, ``"pmn"`` the
    uncorrected ``sigR_pmn``.  The keys are ``physics_noise.TABLE_KEYS``."""
    if row not in ("corrected", "pmn"):
        raise ValueError(f"row is 'corrected' or 'pmn'; got {row!r}")
    if not float(K) > 0 or not math.isfinite(float(K)) or not float(q) >= 0 or not math.isfinite(float(q)):
        raise ValueError(f"K must be positive and q non-negative, both finite; got {K}, {q}")
    d = result.cpu() if isinstance(result, CalibrationResult) else result
    col = {"lam": d["lam"], "sigGs": d["sigGs"], "sigTL": d["sigTL"], "sigR": d["sigR" if row == "corrected" else "sigR_pmn"],
           "bias": np.asarray(d["bias"], np.float64).reshape(len(np.atleast_1d(d["lam"])), -1).mean(axis=1)}
    col = {k: np.atleast_1d(np.asarray(v, np.float64)) for k, v in col.items()}
    spread = lambda v: float(np.std(v, ddof=1)) if len(v) > 1 else 0.0          # noqa: E731
    out = {"Kmax": float(K), "q": float(q), "lam": float(col["lam"].mean())}
    for k in ("sigGs", "sigTL", "sigR", "bias"):
        out[k], out[k + "sig"] = float(col[k].mean()), spread(col[k])
    return {k: out[k] for k in TABLE_KEYS}
