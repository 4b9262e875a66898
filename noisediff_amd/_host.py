"""Host-side helpers of everything that launches the HIP library on torch tensors and torch's streams -- inference (lsid, metrics) and training
(train) alike: the stream and device of a launch, fp32 allocations and workspaces, the "no CPU path" check, and the one rule that picks the kernel
of a 3x3 convolution outside the sampling engine.  Imports only ``torch`` and ``_lib``; needs neither a GPU nor the built library at import time.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib as L


class _Nop:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOP = _Nop()


def _on(device: torch.device):
    """The library launches on the CURRENT device: switch only when the tensors live elsewhere (the context manager costs ~10 us of
    host time per call, and a training step makes several hundred calls)."""
    return _NOP if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def _stream(device: Optional[torch.device] = None) -> C.c_void_p:
    """torch's current stream OF THE TENSORS' DEVICE (not of the current device: a caller may sit on another GPU)."""
    idx = torch.cuda.current_device() if device is None or device.index is None else device.index
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))         # (torch.cuda.current_stream(...).cuda_stream builds a Stream object: 5 us, x 1800 per step)


def _need_gpu(t: torch.Tensor) -> None:
    """There is no fallback: a CPU tensor raises."""
    if t.device.type != "cuda":
        raise L.HipError(f"noisediff_amd.train runs on the HIP library only; tensor is on {t.device} and there is no CPU path")


def _empty(shape, device: torch.device, **kw) -> torch.Tensor:
    """An uninitialised fp32 tensor on the tensors' device."""
    return torch.empty(shape, dtype=torch.float32, device=device, **kw)


def _workspace(entry: str, device: torch.device, *dims) -> torch.Tensor:
    """A buffer sized by the library's own rule ``entry`` for these dimensions: the scratch of one launch (``nd_*_workspace_floats``) or a packed
    weight (``nd_pack_*_floats``).  One call of the entry per buffer."""
    return torch.empty(int(getattr(L.load(), entry)(*dims)), dtype=torch.float32, device=device)


def conv3x3_takes(kernel: int, B: int, H: int, W: int, cin: int, cout: int, c0: int, c1: int, ld0: int, ld1: int, mode: int = L.PRO_NONE, upsample: bool = False,
                  map_blocked: bool = False, ldo: Optional[int] = None, splits: int = 1) -> bool:
    """Does the conv3x3 kernel ``kernel`` (L.CONV3X3_*) take a layer of these sizes?  The library's answer (nd_conv3x3_takes: the kernel's own shape checks, the
    only place its limits are written); ``splits`` > 1: its split-K entry.  Host code: needs the built library and no GPU."""
    d = L.conv3x3(L.src(None, None, mode, c0, ld0, 0, c1, ld1, upsample=int(upsample), map_blocked=int(map_blocked)), None, None, None, B, H, W, cin, cout, ldo)
    return bool(L.load().nd_conv3x3_takes(kernel, C.byref(d), splits))


@functools.lru_cache(maxsize=None)
def conv3x3_trains(cin: int, cout: int) -> bool:
    """Can a 3x3 layer of these widths train on the library?  Its forward and its data gradient (the same operator, widths swapped) at least on the direct kernel."""
    return conv3x3_takes(L.CONV3X3_DIRECT, 1, 1, 1, cin, cout, cin, 0, cin, 0) and conv3x3_takes(L.CONV3X3_DIRECT, 1, 1, 1, cout, cin, cout, 0, cout, 0)


# The other kernel families' questions: like conv3x3_takes the library's own answer, the only place a limit is written (host code: the built library, no GPU).
# Cached, since a training step asks several hundred times.
@functools.lru_cache(maxsize=None)
def _asks(question: str, *dims: int) -> int:
    return int(getattr(L.load(), question)(*dims))


def group_norm_takes(C_: int, groups: int) -> bool:
    """nd_groupnorm(_silu)_train_*_f32."""
    return bool(_asks("nd_groupnorm_train_takes", C_, groups))


def layer_norm_takes(C_: int) -> bool:
    """nd_layernorm_train_*_f32."""
    return bool(_asks("nd_layernorm_train_takes", C_))


def rms_norm_takes(C_: int) -> bool:
    """nd_rmsnorm_backward_f32 (the forward kernels take any multiple of 4)."""
    return bool(_asks("nd_rmsnorm_train_takes", C_))


def token_sum_takes(C_: int) -> bool:
    return bool(_asks("nd_token_sum_takes", C_))


def chain_takes(HW: int, cin: int, n1: int, n2: int, n3: int = 0) -> bool:
    """nd_pointwise_chain(_split)_nhwc_f32: the instantiated widths over whole pixel tiles."""
    return bool(_asks("nd_pointwise_chain_takes", HW, cin, n1, n2, n3))


def conv3x3_wgrad_cat_takes(B: int, H: int, W: int, c0: int, c1: int, cout: int) -> bool:
    """nd_conv3x3_wgrad_cat_nhwc_f32 on dense tensors.  Not cached: the answer follows the pin of nd_conv3x3_wgrad_form."""
    return bool(L.load().nd_conv3x3_wgrad_cat_takes(B, H, W, c0, c1, cout, c0, c1, cout))


@functools.lru_cache(maxsize=None)
def pointwise_takes(cin: int, cout: int, c1: int = 0, split: bool = False) -> bool:
    """Does nd_pointwise_gemm_nhwc_f32 (``split``: nd_pointwise_gemm_split_nhwc_f32) take a plain dense 1x1 / Linear layer of these widths, the last ``c1`` input
    channels from a second source?  One pixel: no limit of either entry depends on the pixel count."""
    d = L.pointwise(L.src(None, None, L.PRO_NONE, cin - c1, cin - c1, 0, c1, c1), None, None, None, 1, 1, 1, cin, cout)
    return bool((L.load().nd_pointwise_gemm_split_takes if split else L.load().nd_pointwise_gemm_takes)(C.byref(d)))


@functools.lru_cache(maxsize=None)
def conv3x3_kind(B: int, H: int, W: int, cin: int, cout: int, c0: int, c1: int, ld: int, wino4: bool = True) -> str:
    """The kernel of a 3x3 convolution outside the sampling engine: 'wino4', 'wino2', 'wino' (F(2x2,3x3) past wino2's limits) or 'direct'.
    ``c0`` / ``c1``: the channels of the two sources (c1 = 0: one source); ``ld``: the pixel stride the source-size limits are computed with;
    ``wino4`` False: never the F(4x4,3x3) kernel.  Policy only -- the order of preference, images of at least one 16 x 16 tile, F(4x4) where the image fills its
    16 x 32-pixel regions; what a kernel can take is the library's answer.  Needs the built library and no GPU; cached (a training step asks several hundred times)."""
    takes = lambda kernel: conv3x3_takes(kernel, B, H, W, cin, cout, c0, c1, ld, ld if c1 else 0)
    wino = H >= 16 and W >= 16 and takes(L.CONV3X3_WINO)
    if wino4 and wino and W >= 32 and (W % 32 == 0 or W >= 96) and takes(L.CONV3X3_WINO4):
        return "wino4"
    if wino and takes(L.CONV3X3_WINO2):
        return "wino2"
    return "wino" if wino else "direct"


class Conv3x3Kernel(NamedTuple):
    """What the host knows of one conv3x3 kernel; CONV3X3 is keyed by conv3x3_kind's answer, which is engine.conv3x3_form's but for its "" (direct)."""
    kernel: int                  # L.CONV3X3_*: the kernel nd_conv3x3_takes is asked about
    entry: str
    splitk: Optional[str]        # its split-K entry
    pack: str                    # the weight packing; + "_floats": its size, + "_dgrad": the data gradient's, from the forward weight
    slot: str                    # the suffix of the sampling engine's arena slot of that packing
    tiling: Optional[int]        # the id bench.py reads from an op's meta; None: the library's nd_conv3x3_tiling_id of the shape
    stat_slots: Callable         # (lib, B, H, W, cout) -> slots per sample of the statistics epilogue


_direct_slots = lambda lib, B, H, W, cout: lib.nd_conv3x3_stat_slots(H, W, cout, B)
_wino_slots = lambda lib, B, H, W, cout: lib.nd_conv3x3_wino_stat_slots(H, W)
_wino4_slots = lambda lib, B, H, W, cout: lib.nd_conv3x3_wino4_stat_slots(H, W)
CONV3X3 = {
    "direct": Conv3x3Kernel(L.CONV3X3_DIRECT, "nd_conv3x3_nhwc_f32", None, "nd_pack_conv3x3_weight", ".weight", None, _direct_slots),
    "wino": Conv3x3Kernel(L.CONV3X3_WINO, "nd_conv3x3_wino_nhwc_f32", None, "nd_pack_conv3x3_wino_weight", ".weight.wino", 9001, _wino_slots),
    "wino2": Conv3x3Kernel(L.CONV3X3_WINO2, "nd_conv3x3_wino2_nhwc_f32", None, "nd_pack_conv3x3_wino_weight", ".weight.wino", 9002, _wino_slots),
    "wino4": Conv3x3Kernel(L.CONV3X3_WINO4, "nd_conv3x3_wino4_nhwc_f32", "nd_conv3x3_wino4_splitk_nhwc_f32", "nd_pack_conv3x3_wino4_weight", ".weight.wino4", 9004,
                           _wino4_slots),
    "wino4_16": Conv3x3Kernel(L.CONV3X3_WINO4_16, "nd_conv3x3_wino4_16_nhwc_f32", "nd_conv3x3_wino4_16_splitk_nhwc_f32", "nd_pack_conv3x3_wino4_weight", ".weight.wino4",
                              9016, _wino4_slots),
}
