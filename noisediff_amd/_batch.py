"""What the GPU batch builders share (``denoise_data.BatchBuilder``, ``raw.RealBatchBuilder`` / ``PoissonGaussianBatchBuilder``,
``diffusion_data.DiffusionBatchBuilder`` / ``GenerationBatchBuilder``): the device parameter block with its host mirror, the ``check`` /
``capture_inputs`` / ``update`` / eager-call scaffolding around a builder's ``_host_block`` and launch, and the validators of the per-sample
parameters.  Imports only ``numpy``, ``torch`` and ``_lib``; needs neither a GPU nor the built library at import time.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L


def need_gpu(*ts: torch.Tensor, what: str) -> torch.device:
    """The one device of the tensors.  There is no fallback: a CPU tensor raises ``HipError`` (``what``: the caller's half of the message)."""
    dev = ts[0].device
    if dev.type != "cuda":
        raise L.HipError(f"{what} only; tensor is on {dev} and there is no CPU path")
    if any(t.device != dev for t in ts):
        raise ValueError("all tensors must be on one device")
    return dev


def cuda_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise L.HipError(f"the batch is built on a GPU; got device {device} and there is no CPU path")
    return device


# ----------------------------------------------------------------------------- validators of one step's parameters (host only)

def per_sample(v, B: int, dtype=np.float64) -> np.ndarray:
    """One value or (B,) values -> (B,)."""
    return np.broadcast_to(np.asarray(v, dtype=dtype).reshape(-1), (B,))


def check_frames(frame: np.ndarray, N: int) -> None:
    if (frame < 0).any() or (frame >= N).any():
        raise ValueError(f"frame indices must be in [0, {N}); got {frame.tolist()}")


def check_positive(v: np.ndarray, what: str, got: Optional[np.ndarray] = None) -> None:
    if not (v > 0).all() or not np.isfinite(v).all():
        raise ValueError(f"{what} must be positive and finite; got {(v if got is None else got).tolist()}")


def check_headroom(top: np.ndarray, what: str) -> None:
    """A Poisson rate's bound ``top`` (``what``: its formula) must stay below 2**24, where fp32 stops holding every integer."""
    if (top >= 2.0 ** 24).any():
        raise ValueError(f"{what} = {top.max():.4g} reaches 2**24: Poisson counts would not stay exact in fp32")


def write_rng(head: np.ndarray, seed: int, first_sample: int, draw: int) -> None:
    """The {seed, first_sample, draw} triple into the head of a host block, as int64."""
    if int(draw) < 0 or int(draw) >= 2 ** 31:
        raise ValueError(f"draw must be in [0, 2**31); got {draw}")
    rng = head.view(np.int64)
    rng[0] = np.array(int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).view(np.int64)
    rng[1], rng[2] = int(first_sample), int(draw)


def rng_key(head: np.ndarray) -> Tuple[int, int, int]:
    """(seed, first_sample, draw) back from the head ``write_rng`` wrote: what an eager launch passes as arguments."""
    key = head.view(np.int64)
    return int(key[0]) & 0xFFFFFFFFFFFFFFFF, int(key[1]), int(key[2])


# ----------------------------------------------------------------------------- the parameter block and the builder around it

class ParamBlock:
    """The device parameter block of one builder launch and its host mirror, ``head + B * per_sample`` elements of ``dtype``: a builder's
    ``update`` writes ``host`` and copies it to ``block`` with one copy; a captured launch reads ``block`` at replay."""

    def __init__(self, B: int, device: torch.device, dtype, head: int, per_sample: int):
        self.B, self.device = int(B), device
        self.host = np.zeros(head + self.B * per_sample, dtype=dtype)
        self.block = torch.zeros(self.host.size, dtype=torch.from_numpy(self.host).dtype, device=device)
        self.use_rng, self.use_sna = True, False             # use_rng: the launch reads the device triple (False: the key goes as arguments)

    def ptr(self, offset: int) -> int:
        return self.block.data_ptr() + offset * self.host.itemsize


class BlockBuilder:
    """The host side of a builder: a subclass names its block class (``Inputs``, a ``ParamBlock`` with DTYPE, HEAD and PER_SAMPLE) and supplies
    ``_host_block(host, B, *params)``, which validates one step's parameters and writes them into ``host``, and the launch."""

    def _check(self, B: int, *params) -> Tuple[np.ndarray, bool]:
        """``check``: (a fresh host block for B with the parameters in it, what ``_host_block`` returned as a flag)."""
        cls = self.Inputs
        host = np.zeros(cls.HEAD + int(B) * cls.PER_SAMPLE, dtype=cls.DTYPE)
        return host, bool(self._host_block(host, int(B), *params))

    @staticmethod
    def _upload(inputs: ParamBlock) -> ParamBlock:
        inputs.block.copy_(torch.from_numpy(inputs.host))
        return inputs

    def _update(self, inputs: ParamBlock, *params) -> ParamBlock:
        """``update``: validate into ``inputs.host``, then ONE host-to-device copy on the current stream."""
        inputs.use_sna = bool(self._host_block(inputs.host, inputs.B, *params))
        return self._upload(inputs)

    def _eager_inputs(self, B: int, host: np.ndarray, device: torch.device, use_rng: bool = True, use_sna: bool = False) -> ParamBlock:
        """The block of one eager call, from the host block ``check`` returned.  The builders that draw pass ``use_rng=False``: an eager call
        passes the key as arguments; a captured one reads the device triple."""
        inputs = self.Inputs(B, device)
        inputs.host[:], inputs.use_rng, inputs.use_sna = host, use_rng, use_sna
        return self._upload(inputs)

    def capture_inputs(self, B: int, device) -> ParamBlock:
        """A persistent device parameter block for batches of B: ``update`` writes it, ``launch`` reads it (also from inside a graph)."""
        device = cuda_device(device)
        if int(B) < 1:
            raise ValueError("B must be positive")
        return self.Inputs(B, device)

    @staticmethod
    def _output(name: str, t: Optional[torch.Tensor], shape, dev: torch.device, make: bool = True) -> Optional[torch.Tensor]:
        """``t`` if it is an fp32 contiguous tensor of ``shape`` on ``dev``; for None a new one (``make``) or None."""
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev) if make else None
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be fp32 contiguous {shape} on {dev}")
        return t
