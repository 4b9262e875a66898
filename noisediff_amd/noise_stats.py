"""Scoring of generated noise on the GPU: the reference's KL-divergence yardstick and its signal-dependence check.

The reference measures generated noise with the noise-generation literature's metric, adopted from noise_flow (utils/util.py:185-255): value
histograms of the generated and of the real noise on the 66 bins of ``kldiv_patch_set`` and the KL divergences between them; and with
``compute_poisson_lambda_by_patch`` (utils/raw_util.py:161-189): the std and mean of every 3 x 3 window and a line fit of std on mean per
(sample, channel).  Both run on the host there.  Here they are HIP kernels (``csrc/noise_stats.hip``) on tensors that stay on the device:

- ``kld_edges()``: the 67 float64 edges, computed with numpy exactly as ``kldiv_patch_set`` does;
- ``histogram_counts(data, bin_edges, per_sample=False)``: int64 counts, ``np.histogram(data, bin_edges)[0]``;
- ``get_histogram(data, bin_edges=None, left_edge=0.0, right_edge=1.0, n_bins=1000)``: the reference's function, ``(hist, bin_centers)``;
- ``kl_div_forward`` / ``kl_div_inverse`` / ``kl_div_sym`` / ``kl_div_3``: of two hists, or of two count tensors and their element counts;
- ``noise_kld(generated, real, per_sample=False)``: the whole metric, a dict of device tensors;
- ``patch_std_mean(x)`` and ``poisson_lambda_by_patch(x)``: the window statistics and the fitted (lambda, intercept), ``[B, C]`` float64.

The numerical contract (the bin rule, fp64 everywhere past the counts, the fixed summation orders) is in DESIGN.md section 14.  Nothing is
copied to the host.  Deterministic: a repeated call gives the same bits and a set's results do not depend on the other sets in the call.
CPU tensors raise ``HipError``; there is no fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._host import _stream

MAX_BINS = 4096
_KLD_EDGES_ON: Dict[torch.device, torch.Tensor] = {}


def kld_edges() -> np.ndarray:
    """The bin edges of kldiv_patch_set (utils/util.py:245-246): -1000, 65 edges from -0.1 to 0.1 in steps of 0.2 / 64, 1000.  np.arange's
    edges are not round (the one next to 0 is 8.3e-17), so they are computed as the reference computes them, never re-derived."""
    bw = 0.2 / 64
    return np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, bw), [1000.0]), axis=0)


def check_edges(bin_edges) -> np.ndarray:
    """The host edge array as contiguous float64, refused unless 2 to 4097 finite, strictly increasing values (numpy also takes repeated
    edges; the kernel does not)."""
    e = np.ascontiguousarray(np.asarray(bin_edges, dtype=np.float64))
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError(f"bin_edges must be a 1-D array of 2 to {MAX_BINS + 1} values; got shape {e.shape}")
    if not np.isfinite(e).all():
        raise ValueError("bin_edges must be finite")
    if not (np.diff(e) > 0).all():
        raise ValueError("bin_edges must be strictly increasing")
    return e


def _on_gpu(*ts: torch.Tensor) -> torch.device:
    for t in ts:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"noise statistics take torch tensors, got {type(t)}")
    dev = ts[0].device
    if dev.type != "cuda":
        raise L.HipError(f"noise statistics run on the HIP library only; tensor is on {dev} and there is no CPU path")
    if any(t.device != dev for t in ts):
        raise ValueError("all tensors must be on one device")
    return dev


def device_edges(bin_edges, device: torch.device) -> torch.Tensor:
    """Checked float64 edges on ``device``: a host array is checked (``check_edges``) and uploaded.  A float64 tensor that is already on the
    device is taken AS IT IS -- reading it back to check it would be a host copy and a synchronisation -- so for such a tensor finite, strictly
    increasing edges are the caller's contract, as they are in the C header: with repeated or decreasing edges the counts are not numpy's (the
    kernel stays inside its tables whatever the edges hold).  The tensors this function returns meet it."""
    if isinstance(bin_edges, torch.Tensor) and bin_edges.device.type == "cuda":
        if bin_edges.dtype != torch.float64 or bin_edges.dim() != 1 or not 2 <= bin_edges.numel() <= MAX_BINS + 1 or bin_edges.device != device:
            raise ValueError("device bin_edges must be a 1-D float64 tensor of 2 to 4097 values on the data's device")
        return bin_edges.contiguous()
    if isinstance(bin_edges, torch.Tensor):
        bin_edges = bin_edges.numpy()
    return torch.from_numpy(check_edges(bin_edges)).to(device)


def _kld_edges_on(device: torch.device) -> torch.Tensor:
    if device not in _KLD_EDGES_ON:
        _KLD_EDGES_ON[device] = device_edges(kld_edges(), device)
    return _KLD_EDGES_ON[device]


def _sets(data: torch.Tensor, per_sample: bool) -> Tuple[torch.Tensor, int, int]:
    x = data.to(torch.float32).contiguous()
    if x.numel() == 0:
        raise ValueError(f"empty data: {tuple(data.shape)}")
    if per_sample and x.dim() < 1:
        raise ValueError("per_sample needs a leading set axis")
    S = x.shape[0] if per_sample else 1
    return x, S, x.numel() // S


def _fraction(counts: torch.Tensor, n: int) -> torch.Tensor:
    """counts / n in float64 by IEEE division: the divisor is a device tensor, since torch divides by a host scalar with a reciprocal multiply."""
    return counts.to(torch.float64) / torch.full((), float(n), dtype=torch.float64, device=counts.device)


def histogram_counts(data: torch.Tensor, bin_edges, per_sample: bool = False) -> torch.Tensor:
    """``np.histogram(data, bin_edges)[0]`` as an int64 device tensor ``[n_bins]``, or ``[S, n_bins]`` with ``per_sample`` (the leading axis of
    ``data`` is then the set axis).  ``bin_edges``: a host array (checked and uploaded) or the result of ``device_edges``.  Element v is in bin
    i when edges[i] <= v < edges[i + 1] in float64, the last bin closed; NaN, inf and values outside the edges are counted nowhere.
    The kernel bins fp32 values: ``data`` of another dtype (float64, integers, half) is rounded to fp32 FIRST, so a float64 value within fp32
    rounding of an edge can land in the neighbouring bin of where numpy puts the float64 value.  Generated patches are fp32.  A ``bin_edges``
    tensor already on the device is not checked: finite, strictly increasing edges are then the caller's contract (see ``device_edges``)."""
    dev = _on_gpu(data)
    edges = device_edges(bin_edges, dev)
    x, S, n = _sets(data, per_sample)
    n_bins = edges.numel() - 1
    ws = torch.empty(int(L.call("nd_histogram_workspace_bytes", S, n, n_bins)), dtype=torch.uint8, device=dev)
    counts = torch.empty(S, n_bins, dtype=torch.int64, device=dev)
    L.call("nd_histogram_f32", x.data_ptr(), S, n, edges.data_ptr(), n_bins + 1, counts.data_ptr(), ws.data_ptr(), _stream(dev))
    return counts if per_sample else counts[0]


def get_histogram(data: torch.Tensor, bin_edges=None, left_edge: float = 0.0, right_edge: float = 1.0, n_bins: int = 1000,
                  per_sample: bool = False) -> Tuple[torch.Tensor, np.ndarray]:
    """utils/util.py:188-196: ``(hist, bin_centers)`` with hist = counts / np.prod(data.shape) as a float64 device tensor (per set with
    ``per_sample``) and bin_centers the host float64 array the reference forms from the edges.  ``data`` is binned as fp32 (see
    ``histogram_counts``)."""
    data_range = right_edge - left_edge
    bin_width = data_range / n_bins
    if bin_edges is None:
        bin_edges = np.arange(left_edge, right_edge + bin_width, bin_width)
    counts = histogram_counts(data, bin_edges, per_sample)
    host = bin_edges.cpu().numpy() if isinstance(bin_edges, torch.Tensor) else np.asarray(bin_edges, dtype=np.float64)
    n = data.numel() // (data.shape[0] if per_sample else 1)
    return _fraction(counts, n), host[:-1] + (bin_width / 2.0)


def kl_div_3(p: torch.Tensor, q: torch.Tensor, n_p: Optional[int] = None, n_q: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """utils/util.py:223-227: (forward sum p log(p / q), inverse sum q log(q / p), their mean) over the bins with p > 0 and q > 0, in fp64.
    ``p``, ``q``: two float64 hists, or two int64 count tensors with their element counts ``n_p``, ``n_q`` (np.prod(data.shape), dropped values
    included).  Shapes ``[n_bins]`` (scalar results) or ``[S, n_bins]`` (results ``[S]``); ``q`` may be one histogram for every set of ``p``."""
    dev = _on_gpu(p, q)
    if p.dim() not in (1, 2) or q.dim() not in (1, 2) or p.shape[-1] != q.shape[-1] or p.shape[-1] < 1:
        raise ValueError(f"histograms must be [n_bins] or [S, n_bins] with one n_bins; got {tuple(p.shape)} and {tuple(q.shape)}")
    S, q_sets = (p.shape[0] if p.dim() == 2 else 1), (q.shape[0] if q.dim() == 2 else 1)
    if S < 1 or q_sets not in (1, S):
        raise ValueError(f"q must hold 1 or {S} histograms, got {q_sets}")
    n_bins = p.shape[-1]
    out = torch.empty(S, 3, dtype=torch.float64, device=dev)
    if p.dtype == torch.int64 and q.dtype == torch.int64:
        if n_p is None or n_q is None or int(n_p) < 1 or int(n_q) < 1:
            raise ValueError("count histograms need the element counts n_p and n_q (positive)")
        pc, qc = p.contiguous(), q.contiguous()
        L.call("nd_kl_div_f64", pc.data_ptr(), qc.data_ptr(), int(n_p), int(n_q), n_bins, S, q_sets, out.data_ptr(), _stream(dev))
    elif p.dtype == torch.float64 and q.dtype == torch.float64:
        if n_p is not None or n_q is not None:
            raise ValueError("n_p and n_q go with int64 counts, not with float64 hists")
        pc, qc = p.contiguous(), q.contiguous()
        L.call("nd_kl_div_hist_f64", pc.data_ptr(), qc.data_ptr(), n_bins, S, q_sets, out.data_ptr(), _stream(dev))
    else:
        raise TypeError(f"p and q must both be float64 hists or both int64 counts; got {p.dtype} and {q.dtype}")
    res = out if p.dim() == 2 else out[0]
    return res[..., 0], res[..., 1], res[..., 2]


def kl_div_forward(p, q, n_p=None, n_q=None) -> torch.Tensor:
    """utils/util.py:199-206."""
    return kl_div_3(p, q, n_p, n_q)[0]


def kl_div_inverse(p, q, n_p=None, n_q=None) -> torch.Tensor:
    """utils/util.py:209-216."""
    return kl_div_3(p, q, n_p, n_q)[1]


def kl_div_sym(p, q, n_p=None, n_q=None) -> torch.Tensor:
    """utils/util.py:219-220."""
    return kl_div_3(p, q, n_p, n_q)[2]


def noise_kld(generated: torch.Tensor, real: torch.Tensor, per_sample: bool = False) -> Dict[str, torch.Tensor]:
    """The metric of kldiv_patch_set (utils/util.py:244-253): both histograms on ``kld_edges()`` and the divergences of real against generated,
    ``kl_div_forward(hist_real, hist_generated)`` in the reference's argument order.  Returns {'kl_fwd', 'kl_inv', 'kl_sym', 'hist_generated',
    'hist_real'} as float64 device tensors (scalars, or ``[S]`` and ``[S, 66]`` with ``per_sample``: set s of ``generated`` against set s of
    ``real``, or against the one set of a ``real`` whose leading axis is 1).  Nothing is copied to the host."""
    dev = _on_gpu(generated, real)
    edges = _kld_edges_on(dev)
    cg, cr = histogram_counts(generated, edges, per_sample), histogram_counts(real, edges, per_sample)
    n_g = generated.numel() // (generated.shape[0] if per_sample else 1)
    n_r = real.numel() // (real.shape[0] if per_sample else 1)
    if per_sample and cr.shape[0] != cg.shape[0]:
        if cr.shape[0] != 1:
            raise ValueError(f"real must hold 1 or {cg.shape[0]} sets, got {cr.shape[0]}")
        cr = cr.expand(cg.shape[0], -1).contiguous()
    fwd, inv, sym = kl_div_3(cr, cg, n_r, n_g)
    return {"kl_fwd": fwd, "kl_inv": inv, "kl_sym": sym, "hist_generated": _fraction(cg, n_g), "hist_real": _fraction(cr, n_r)}


def _patch(x: torch.Tensor, want_maps: bool):
    dev = _on_gpu(x)
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"x must be a non-empty (B, C, H, W) tensor; got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    B, C, H, W = x.shape
    ws = torch.empty(int(L.call("nd_patch_std_mean_workspace_bytes", B, C, H, W)), dtype=torch.uint8, device=dev)
    fit = torch.empty(B * C, 7, dtype=torch.float64, device=dev)
    std = torch.empty_like(x) if want_maps else None
    mean = torch.empty_like(x) if want_maps else None
    L.call("nd_patch_std_mean_f32", x.data_ptr(), L.ptr(std), L.ptr(mean), fit.data_ptr(), ws.data_ptr(), B, C, H, W, _stream(dev))
    return std, mean, fit.view(B, C, 7)


def patch_std_mean(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``torch.std_mean(sliding_window(x), dim=2)`` (utils/raw_util.py:161-172) as two (B, C, H, W) fp32 maps: the unbiased std and the mean of
    every pixel's 3 x 3 window, zeros outside the image."""
    std, mean, _ = _patch(x, True)
    return std, mean


def poisson_lambda_by_patch(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """compute_poisson_lambda_by_patch (utils/raw_util.py:169-189): slope and intercept of the least-squares line of the window std on the
    window mean per (sample, channel), ``[B, C]`` float64 device tensors.  The maps are not written.  A plane whose means are all equal gives NaN."""
    _, _, fit = _patch(x, False)
    return fit[..., 5], fit[..., 6]
