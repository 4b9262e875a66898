"""The calibrated physics-based noise model of ELD / PMN on the GPU: the baseline a learned noise synthesizer has to beat.

Four parts, drawn per element of crop windows (or whole frames) of resident uint16 long-exposure frames by one launch of
``csrc/physics_noise.hip``: Poisson shot noise, read noise that is Gaussian or heavy-tailed Tukey-lambda, row noise, and quantisation noise
with a bias.  In codes above black at the short exposure (DN), with ``wb = white - black``::

    t = K Poisson(clean_codes / ratio / K) + s_read r + s_row g[row, channel] + (q wb) (u - 1/2) + bias
    noisy = clip(t, -black, wb) ratio / wb          (clipped to [0, 1] with clip01)

The reference ships this model's calibration for the SID camera (utils/raw_util.py ``get_camera_noisy_params_max``: one row per ISO with
``Kmax, lam, sigGs, sigTL, sigR, q, bias`` and their spreads) and uses nothing of a row but ``Kmax``.  The package ships no table: a
``CameraNoiseModel`` is built from one the caller supplies.

- ``PhysicsNoiseBatchBuilder(crop, black=512, white=16383, clip01=True)``: a training batch ``(noisy, clean)`` of crop windows, with ``check`` /
  ``capture_inputs`` / ``update`` / ``launch`` / ``__call__`` and ``random_params`` as ``raw.PoissonGaussianBatchBuilder`` has them;
- ``physics_frames(frames, frame, ratio, params, seed, ...)``: whole frames through the same entry, ``(B, 4, H, W)``; ``raw.to_bayer`` makes a mosaic;
- ``CameraNoiseModel(table).draw(iso, seed, first_sample, read)``: the per-sample ``params`` as PMN samples them;
- ``tukey_lambda_quantile(u, lam)``: the quantile the kernel evaluates, in numpy.

``params`` is a mapping with ``K, s_read, read_kind, lam, s_row, q, bias``, each one value or (B,) values.  ``s_read`` with ``read_kind`` 1 is
the SCALE of the unit Tukey-lambda variate (``scipy.stats.tukeylambda``'s ``scale=``, PMN's ``sigTL``), not a standard deviation: the unit
variate's variance is ``(2 / lam^2) (1 / (1 + 2 lam) - Gamma(lam + 1)^2 / Gamma(2 lam + 2))``, 2.06 at lam = 0.149 and 4.61 at lam = -0.091.
It is infinite for ``lam <= -0.5``; such a shape is drawn as asked and not refused.

The draws are counter-based: keyed by ``(seed, first_sample + b, draw)`` and the element's position in the output, so a
repeated call gives the same bits and a sample's bits do not depend on the batch around it.  The row variates are keyed by the SOURCE row and
a per-sample word ``row_stream`` (default ``first_sample + b``: every crop its own row pattern, as in PMN); windows that tile one frame are
given the frame's one value and then agree wherever their rows overlap.  CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import synth
from ._batch import ParamBlock, check_frames, check_headroom, check_positive, per_sample, rng_key, write_rng
from ._host import _stream
from .raw import BLACK, WHITE, _WindowBuilder, frame_shape, frames_on_device

_RNG_BYTES = 32                      # the {seed, first_sample, draw} triple as int64, padded
ROW = np.dtype([("frame", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("flip", "<i4"), ("read_kind", "<i4"), ("row_stream", "<u4"),
                ("reserved", "<i4", (2,)), ("ratio", "<f8"), ("K", "<f8"), ("s_read", "<f8"), ("lam", "<f8"), ("s_row", "<f8"), ("qstep", "<f8"),
                ("bias", "<f8")])                                                       # nd_physics_sample
assert ROW.itemsize == C.sizeof(L.PhysicsSample) == 88
PARAM_KEYS = ("K", "s_read", "read_kind", "lam", "s_row", "q", "bias")
READ_KINDS = {"gaussian": 0, "tukey": 1}
TABLE_KEYS = ("Kmax", "lam", "sigGs", "sigGssig", "sigTL", "sigTLsig", "sigR", "sigRsig", "bias", "biassig", "q")
_VARIATES = ("counts", "reads", "rows", "quants")


def tukey_lambda_quantile(u, lam: float) -> np.ndarray:
    """Q(u) of the unit Tukey-lambda distribution in float64, in the kernel's form: (expm1(lam log u) - expm1(lam log1p(-u))) / lam, and the
    logistic quantile log u - log1p(-u) at lam == 0.  pow(u, lam) - 1 cancels at the calibrated |lam| of 0.003; expm1 does not."""
    u, lam = np.asarray(u, np.float64), float(lam)
    a, b = np.log(u), np.log1p(-u)
    if lam == 0.0:
        return a - b
    return (np.expm1(lam * a) - np.expm1(lam * b)) / lam


def _write_params(rows: np.ndarray, B: int, ratio, params: Mapping[str, object], row_stream, first_sample: int, wb: float) -> None:
    """Validate one step's model parameters on the host and write them into the table ``rows``."""
    missing = [k for k in PARAM_KEYS if k not in params]
    if missing:
        raise ValueError(f"params lacks {missing}; it carries {list(PARAM_KEYS)}")
    ratio = per_sample(ratio, B)
    check_positive(ratio, "ratio")
    K = per_sample(params["K"], B)
    check_positive(K, "the gain K")
    for name in ("s_read", "s_row", "q"):
        v = per_sample(params[name], B)
        if not (v >= 0).all() or not np.isfinite(v).all():
            raise ValueError(f"the scale {name} must be non-negative and finite; got {v.tolist()}")
    lam, bias = per_sample(params["lam"], B), per_sample(params["bias"], B)
    if not np.isfinite(lam).all() or not np.isfinite(bias).all():
        raise ValueError(f"lam and bias must be finite; got {lam.tolist()}, {bias.tolist()}")
    given = params["read_kind"]
    given = [given] if isinstance(given, (str, int, np.integer)) else list(np.asarray(given, dtype=object).reshape(-1))
    kind = [READ_KINDS.get(k, -1) if isinstance(k, str) else (int(k) if isinstance(k, (int, np.integer)) else -1) for k in given]
    if len(kind) not in (1, B) or not all(k in (0, 1) for k in kind):
        raise ValueError(f"read_kind is 0 / 'gaussian' or 1 / 'tukey', one value or B = {B}; got {params['read_kind']}")
    check_headroom(wb / (ratio * K), "(white - black) / (ratio * K)")
    if row_stream is None:
        row_stream = int(first_sample) + np.arange(B, dtype=np.int64)
    row_stream = per_sample(row_stream, B, np.int64) & 0xFFFFFFFF
    rows["ratio"], rows["K"], rows["read_kind"], rows["lam"], rows["bias"], rows["row_stream"] = ratio, K, kind, lam, bias, row_stream
    rows["s_read"], rows["s_row"] = per_sample(params["s_read"], B), per_sample(params["s_row"], B)
    rows["qstep"] = per_sample(params["q"], B) * wb


def _wb(black: float, white: float) -> float:
    return float(np.float32(white) - np.float32(black))


class PhysicsInputs(ParamBlock):
    """The device parameter block of one launch: the {seed, first_sample, draw} triple and the per-sample table (nd_physics_sample rows) in ONE
    byte buffer, written by ``update`` with one copy.  A captured launch reads it at replay."""
    DTYPE, HEAD, PER_SAMPLE = np.uint8, _RNG_BYTES, ROW.itemsize

    def __init__(self, B: int, device: torch.device):
        super().__init__(B, device, self.DTYPE, self.HEAD, self.PER_SAMPLE)

    rng_ptr = property(lambda self: self.ptr(0))
    table_ptr = property(lambda self: self.ptr(_RNG_BYTES))


class PhysicsNoiseBatchBuilder(_WindowBuilder):
    """A training batch of the physics-based model from resident long-exposure frames: clean = max(x - black, 0) / wb and noisy as the head of
    this module gives it, both on one crop window per sample.  clip01: noisy is clipped to [0, 1] (the training sets' range); without it the
    sensor's own range [-black, wb] ratio / wb stays, which is what a noise histogram wants."""
    Inputs = PhysicsInputs
    ROW = ROW

    def __init__(self, crop: int, black: float = BLACK, white: float = WHITE, clip01: bool = True):
        super().__init__(crop, black, white)
        self.flags = L.PHYS_CLIP01 if clip01 else 0

    def _host_block(self, host: np.ndarray, B: int, shape, frame, xy, ratio, params, flip, row_stream, seed: int, first_sample: int, draw: int) -> None:
        rows = self._rows(host, B, shape, frame, xy, flip)
        write_rng(host[:_RNG_BYTES], seed, first_sample, draw)
        _write_params(rows, B, ratio, params, row_stream, first_sample, _wb(self.black, self.white))

    def check(self, B: int, shape, frame, xy, ratio, params, flip=None, row_stream=None, seed: int = 0, first_sample: int = 0,
              draw: int = 0) -> np.ndarray:
        """Validate one step's parameters on the host (no device is touched): ValueError for what the window builders refuse (odd frame sides, a
        window outside the frame, a frame index >= N, ratio <= 0, a negative draw), K <= 0, a negative or non-finite scale (s_read, s_row, q), a
        non-finite lam or bias, an unknown read_kind, or (white - black) / (ratio K) >= 2**24.  Returns the parameter block."""
        return self._check(B, shape, frame, xy, ratio, params, flip, row_stream, seed, first_sample, draw)[0]

    def update(self, inputs: PhysicsInputs, shape, frame, xy, ratio, params, flip=None, row_stream=None, seed: int = 0, first_sample: int = 0,
               draw: int = 0) -> PhysicsInputs:
        """Write one step's parameters into the device block: host validation, then ONE host-to-device copy on the current stream."""
        return self._update(inputs, shape, frame, xy, ratio, params, flip, row_stream, seed, first_sample, draw)

    def launch(self, inputs: PhysicsInputs, frames: torch.Tensor, noisy: Optional[torch.Tensor] = None, clean_out: Optional[torch.Tensor] = None,
               noise_out: Optional[torch.Tensor] = None, given: Optional[Mapping[str, torch.Tensor]] = None,
               used: Optional[Mapping[str, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The one kernel launch, on the current stream, reading ``inputs``: no allocation when ``noisy`` and ``clean_out`` are given, no
        synchronisation, capturable.  given / used: {"counts", "reads", "rows", "quants"} -> fp32 tensors that replace the draws / receive what
        was used ((B, 4, crop, crop); rows: (B, 4, crop), indexed by the output row)."""
        f = self._device_frames(inputs, frames)
        c = self.crop
        return _launch(f, inputs.table_ptr, inputs.rng_ptr if inputs.use_rng else None, rng_key(inputs.host[:_RNG_BYTES]), inputs.B, c, c,
                       self.black, self.white, self.flags, noisy, clean_out, noise_out, given, used)

    def __call__(self, frames, frame, xy, ratio, params, flip=None, row_stream=None, seed: int = 0, first_sample: int = 0, draw: int = 0,
                 counts: Optional[torch.Tensor] = None, reads: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
                 quants: Optional[torch.Tensor] = None, return_draws: bool = False, return_noise: bool = False):
        """One batch.  frames: (N, H2, W2); frame: (B,) indices; xy: (B, 2) window origins (x, y) in packed pixels; ratio: (B,) or one value;
        params: the model's per-sample parameters; seed / first_sample / draw key the draws; counts, reads, quants (B, 4, crop, crop) and rows
        (B, 4, crop): variates to use instead of drawing.  Returns (noisy, clean[, noise][, counts, reads, rows, quants used])."""
        B = len(np.asarray(frame).reshape(-1))
        host = self.check(B, tuple(frames.shape), frame, xy, ratio, params, flip, row_stream, seed, first_sample, draw)
        f = frames_on_device(frames)
        dev, c = f.device, self.crop
        inputs = self._eager_inputs(B, host, dev, use_rng=False)
        given = {k: t.to(torch.float32).contiguous() for k, t in zip(_VARIATES, (counts, reads, rows, quants)) if t is not None}
        used = {k: torch.empty((B, 4, c) if k == "rows" else (B, 4, c, c), dtype=torch.float32, device=dev) for k in _VARIATES} if return_draws else {}
        noise = torch.empty(B, 4, c, c, dtype=torch.float32, device=dev) if return_noise else None
        noisy, clean = self.launch(inputs, f, noise_out=noise, given=given, used=used)
        return (noisy, clean) + ((noise,) if return_noise else ()) + (tuple(used[k] for k in _VARIATES) if return_draws else ())


def _launch(f: torch.Tensor, table_ptr: int, rng_ptr: Optional[int], key: Tuple[int, int, int], B: int, h: int, w: int, black: float, white: float,
            flags: int, noisy, clean_out, noise_out, given, used) -> Tuple[torch.Tensor, torch.Tensor]:
    """nd_raw_physics_noise_f32 on the current stream of the frames' device, its tensors checked."""
    dev, shape = f.device, (B, 4, h, w)
    out = _WindowBuilder._output
    noisy, clean_out = out("noisy", noisy, shape, dev), out("clean_out", clean_out, shape, dev)
    out("noise_out", noise_out, shape, dev, make=False)
    ptrs = []
    for what, group in (("", given or {}), ("_out", used or {})):
        unknown = set(group) - set(_VARIATES)
        if unknown:
            raise ValueError(f"the variate arrays are {list(_VARIATES)}; got {sorted(unknown)}")
        for k in _VARIATES:
            ptrs.append(L.ptr(out(k + what, group.get(k), (B, 4, h) if k == "rows" else shape, dev, make=False)))
    N, H2, W2 = f.shape
    L.call("nd_raw_physics_noise_f32", f.data_ptr(), N, H2, W2, table_ptr, rng_ptr, *key, *ptrs, black, white, flags, noisy.data_ptr(),
           clean_out.data_ptr(), L.ptr(noise_out), B, h, w, _stream(dev))
    return noisy, clean_out


def physics_frames(frames, frame, ratio, params, seed: int = 0, first_sample: int = 0, draw: int = 0, row_stream=None, black: float = BLACK,
                   white: float = WHITE, clip01: bool = True, return_noise: bool = False):
    """Whole noisy frames of the physics-based model: the builder's entry with one window per sample that covers the frame.

    frames: (N, H2, W2) long exposures; frame: (B,) indices into them; ratio: (B,) or one value; params, seed, first_sample, draw, row_stream
    as ``PhysicsNoiseBatchBuilder`` takes them.  Returns (noisy, clean[, noise]), each (B, 4, H2 / 2, W2 / 2); ``raw.to_bayer`` turns noisy into
    a mosaic.  Sample b equals the same sample drawn alone with ``first_sample + b`` (and the same row_stream)."""
    if not 0 <= float(black) < float(white) <= 65535:
        raise ValueError(f"need 0 <= black < white <= 65535; got {black}, {white}")
    N, H2, W2 = frame_shape(tuple(frames.shape))
    h, w = H2 // 2, W2 // 2
    if 4 * h * w >= 2 ** 32:
        raise ValueError(f"the packed frame {h} x {w} does not fit the 32-bit element counter")
    idx = np.asarray(frame, dtype=np.int64).reshape(-1)
    B = len(idx)
    if B < 1:
        raise ValueError("give one frame index at least")
    check_frames(idx, N)
    host = np.zeros(_RNG_BYTES + B * ROW.itemsize, np.uint8)
    write_rng(host[:_RNG_BYTES], seed, first_sample, draw)
    rows = host[_RNG_BYTES:].view(ROW)
    rows["frame"] = idx
    _write_params(rows, B, ratio, params, row_stream, first_sample, _wb(black, white))
    f = frames_on_device(frames)
    block = torch.from_numpy(host).to(f.device)
    noise = torch.empty(B, 4, h, w, dtype=torch.float32, device=f.device) if return_noise else None
    noisy, clean = _launch(f, block.data_ptr() + _RNG_BYTES, None, rng_key(host[:_RNG_BYTES]), B, h, w, float(black), float(white),
                           L.PHYS_CLIP01 if clip01 else 0, None, None, noise, None, None)
    return (noisy, clean, noise) if return_noise else (noisy, clean)


def _host_normal(seed: int, name: str, count: int, offset: int) -> np.ndarray:
    """float64 standard normals of ``synth``'s host streams, elements offset .. offset + count - 1 (synth.normal's Box-Muller, not rounded)."""
    u1 = synth.uniform01(seed, name + "#r", count, offset)
    u2 = synth.uniform01(seed, name + "#a", count, offset)
    return np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * math.pi * u2)


class CameraNoiseModel:
    """A camera's calibration of the physics-based model, sampled as PMN samples it.

    table: {iso: row}, each row a mapping with the keys of the reference's get_camera_noisy_params_max rows: ``Kmax, lam, sigGs, sigGssig,
    sigTL, sigTLsig, sigR, sigRsig, bias, biassig, q`` (``wp`` and ``bl`` are not read: the levels belong to the builder).  The package ships no
    table; tests/golden/physics_params.json holds four rows of the SID camera's."""

    def __init__(self, table: Mapping[int, Mapping[str, float]]):
        self.table: Dict[int, Dict[str, float]] = {}
        for iso, row in table.items():
            missing = [k for k in TABLE_KEYS if k not in row]
            if missing:
                raise ValueError(f"the row of ISO {iso} lacks {missing}")
            self.table[int(iso)] = {k: float(row[k]) for k in TABLE_KEYS}
        if not self.table:
            raise ValueError("the table is empty")

    def row(self, iso: int) -> Dict[str, float]:
        if int(iso) not in self.table:
            raise KeyError(f"ISO {iso} is not in the table; it has {sorted(self.table)}")
        return self.table[int(iso)]

    def draw(self, iso, seed: int, first_sample: int = 0, read: str = "gaussian") -> Dict[str, np.ndarray]:
        """The ``params`` of a batch: iso is one value or (B,) values, sample b takes element first_sample + b of four host streams of ``synth``,
        so a sample's parameters do not depend on its batch.

        K = Kmax (1 + U(-0.01, 0.01)) (trainer_denoising.py's jitter of the gain); s_read ~ N(sigGs, sigGssig) for ``read="gaussian"`` or
        N(sigTL, sigTLsig) for ``"tukey"``; s_row ~ N(sigR, sigRsig); bias ~ N(bias, biassig); the scales floored at 0; lam and q from the row."""
        if read not in READ_KINDS:
            raise ValueError(f"read is 'gaussian' or 'tukey'; got {read!r}")
        rows = [self.row(i) for i in np.asarray(iso).reshape(-1)]
        B, off = len(rows), int(first_sample)
        col = lambda k: np.array([r[k] for r in rows], np.float64)          # noqa: E731
        centre, spread = ("sigGs", "sigGssig") if read == "gaussian" else ("sigTL", "sigTLsig")
        u = synth.uniform01(seed, "physics_noise.K", B, off)
        K = col("Kmax") * (1.0 + (0.02 * u - 0.01))
        s_read = np.maximum(col(centre) + col(spread) * _host_normal(seed, "physics_noise.s_read", B, off), 0.0)
        s_row = np.maximum(col("sigR") + col("sigRsig") * _host_normal(seed, "physics_noise.s_row", B, off), 0.0)
        bias = col("bias") + col("biassig") * _host_normal(seed, "physics_noise.bias", B, off)
        return {"K": K, "s_read": s_read, "read_kind": np.full(B, READ_KINDS[read], np.int64), "lam": col("lam"), "s_row": s_row, "q": col("q"),
                "bias": bias}
