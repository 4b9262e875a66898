"""``LSID``: the reference's denoiser arch (models/archs/SID_arch.py:49-175) on the HIP library -- the
consumer of the synthesized noise (BASELINE config 5).

Same plug-in contract as NoiseDiffNet: ``LSID(args)``, reference state-dict names/shapes (strict load),
``forward(x)`` with an NCHW (B, 4, H, W) tensor.  It reuses the sampler's kernels: every ``Conv2d(3x3)`` is
``nd_conv3x3_{wino4, wino2, wino, direct}_nhwc_f32`` (chosen by ``_host.conv3x3_kind``) storing the *pre-activation*; ``LeakyReLU(0.2)`` is
applied by the consumer's prologue (ND_PRO_LEAKY; it commutes with max-pooling, and ND_PRO_LEAKY_SECOND handles
``cat(up(x), skip)`` where only the skip is activated); ``ConvTranspose2d(2, s=2)`` is one pointwise GEMM to
4*C' columns with a pixel-shuffle store that also performs the crop.  Inference only; no CPU fallback.

``lsid_forward_hip`` is the network's one list of launches: the plan here records it once per input shape and replays it,
``lsid_train`` runs it on torch's stream as the forward of training.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib as L
from .net import _attach, _init
from .spec import LSID_STAGES, lsid_param_spec
from ._host import CONV3X3, _stream, conv3x3_kind

WINO4 = os.environ.get("ND_WINO4", "1") != "0"           # A-B knob: 0 = never the F(4x4,3x3) kernel


class LSID(nn.Module):
    def __init__(self, args=None):
        super().__init__()
        self.block_size = 2
        for p in lsid_param_spec():
            _attach(self, p.name, nn.Parameter(_init(p)))
        self._plans: Dict[Tuple[int, int, int, int], "_LsidPlan"] = {}
        self._sig = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"], state["_sig"] = {}, None
        return state

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("noisediff_amd.LSID is inference-only; train with the reference's LSID (same state dict)")
        if x.device.type != "cuda":
            raise L.HipError(f"LSID runs on the HIP library only; tensor is on {x.device} and there is no CPU path")
        sig = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if sig != self._sig:
            self._plans, self._sig = {}, sig
        B, Cc, H, W = x.shape
        key = (x.device.index or 0, B, H, W)
        if key not in self._plans:
            self._plans[key] = _LsidPlan(self, x.device, B, H, W)
        return self._plans[key].run(x)


# ------------------------------------------------------------------ the network's launches, shared with lsid_train
class _Launcher:
    """Buffers and launches of one LSID pass; ``keep`` owns every buffer a launch reads or writes.  Weight packs and allocations execute at once.
    The launches run now on torch's current stream (training), or, with ``stream`` given, are recorded in ``ops`` for replay on that stream
    (the inference plan).  ``wino4`` False: no 3x3 convolution on the F(4x4,3x3) kernel."""

    def __init__(self, dev: torch.device, wino4: bool, stream: Optional[C.c_void_p] = None):
        self.lib = L.load()
        self.dev, self.wino4 = dev, wino4
        self.st = _stream(dev) if stream is None else stream
        self.ops: Optional[List[tuple]] = None if stream is None else []
        self.keep: List[object] = []

    def empty(self, *shape) -> torch.Tensor:
        t = torch.empty(*shape, dtype=torch.float32, device=self.dev)
        self.keep.append(t)
        return t

    def launch(self, name: str, *args) -> None:
        args += (self.st,)
        if self.ops is None:
            L.call(name, *args)
        else:
            self.keep.append(args)
            self.ops.append((getattr(self.lib, name), args, name))

    def pack(self, name: str, *args) -> None:
        """A weight packing, run now; off torch's stream it first waits for torch, which produced the weight."""
        if self.ops is not None:
            torch.cuda.synchronize(self.dev)
        L.call(name, *args, self.st)

    # ---- weight packings
    def pack_pw(self, m: torch.Tensor, cin: int, cout: int, unshuffle_c: int = 0) -> torch.Tensor:
        out = self.empty(int(self.lib.nd_pack_pointwise_weight_floats(cin, cout)))
        self.keep.append(m)
        self.pack("nd_pack_pointwise_weight", m.data_ptr(), out.data_ptr(), cin, cout, unshuffle_c)
        return out

    def pack_pw_t(self, w: torch.Tensor, cin: int, cout: int) -> torch.Tensor:
        out = self.empty(int(self.lib.nd_pack_pointwise_weight_floats(cin, cout)))
        self.pack("nd_pack_pointwise_weight_t", w.data_ptr(), out.data_ptr(), cin, cout)
        return out

    def conv3x3(self, w_oihw: torch.Tensor, bias: Optional[torch.Tensor], src: L.Src, B: int, h: int, w: int, cin: int, cout: int,
                dgrad: bool = False) -> torch.Tensor:
        """One 3x3 convolution (``dgrad``: the data gradient of the layer whose forward weight is ``w_oihw``; cin / cout are the operator's)."""
        k = CONV3X3[conv3x3_kind(B, h, w, cin, cout, src.c0, src.c1, max(src.ld0, src.ld1), self.wino4)]
        wp = self.empty(int(getattr(self.lib, k.pack + "_floats")(cin, cout)))
        self.pack(k.pack + ("_dgrad" if dgrad else ""), w_oihw.data_ptr(), wp.data_ptr(), cin, cout)
        out = self.empty(B, h, w, cout)
        d = L.conv3x3(src, wp, bias, out, B, h, w, cin, cout)
        self.keep.append(d)
        self.launch(k.entry, C.byref(d))
        return out

    def pointwise(self, src: L.Src, wp: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, B: int, HW: int, W: int, cin: int, cout: int,
                  ldo: int, shuffle: Optional[Tuple[int, int, int]] = None, crop_src: Optional[Tuple[int, int]] = None) -> None:
        d = L.pointwise(src, wp, bias, out, B, HW, W, cin, cout, ldo, shuffle=shuffle)
        self.keep.append(d)
        if crop_src is not None:
            self.launch("nd_pointwise_gemm_unshuffle_crop_nhwc_f32", C.byref(d), crop_src[0], crop_src[1])
        else:
            self.launch("nd_pointwise_gemm_nhwc_f32", C.byref(d))

    def join(self, z: torch.Tensor, dz: torch.Tensor, d_direct: Optional[torch.Tensor], ld_direct: int, d_pool: Optional[torch.Tensor],
             direct_offset: int = 0) -> torch.Tensor:
        B, h, w, c = z.shape
        self.launch("nd_leaky_grad_join_f32", z.data_ptr(), dz.data_ptr(), d_direct.data_ptr() + 4 * direct_offset if d_direct is not None else None,
                    ld_direct, d_pool.data_ptr() if d_pool is not None else None, B, h, w, c)
        return dz


def _sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """Spatial size of each encoder stage: ceil-mode pooling halves with rounding up."""
    out = [(H, W)]
    for _ in range(4):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def lsid_forward_hip(P: Dict[str, torch.Tensor], x: torch.Tensor, saved: Dict[str, torch.Tensor], run: _Launcher, head_nhwc: bool = False) -> torch.Tensor:
    """LSID.forward (SID_arch.py:105-175) as launches of ``run`` on the parameter table ``P``: the (B, 4, H, W) output; fills ``saved`` with the raw
    tensors lsid_train's backward reads.  ``head_nhwc``: stop at the 1x1 head's own output (B, H, W, 4), without the transpose to NCHW (the fused loss
    of lsid_train reads it as it lies)."""
    B, _, H, W = x.shape
    sizes = _sizes(H, W)
    xn = x.detach().to(torch.float32).contiguous()
    run.keep.append(xn)
    x8 = run.empty(B, H, W, 8)
    run.launch("nd_nchw_to_nhwc_pad_f32", xn.data_ptr(), x8.data_ptr(), B, 4, H, W, 8)
    saved["x8"] = x8
    w11 = P["conv1_1.weight"]
    w11 = torch.cat((w11, torch.zeros(w11.shape[0], 4, 3, 3, dtype=w11.dtype, device=w11.device)), 1).contiguous()   # conv1_1: 4 input channels padded to 8
    run.keep.append(w11)
    cur, mode, cin = x8, L.PRO_NONE, 8
    for i, c in enumerate(LSID_STAGES, start=1):
        h, w = sizes[i - 1]
        wi1 = w11 if i == 1 else P[f"conv{i}_1.weight"]
        a = run.conv3x3(wi1, P[f"conv{i}_1.bias"], L.src(cur, mode=mode), B, h, w, cin, c)
        z = run.conv3x3(P[f"conv{i}_2.weight"], P[f"conv{i}_2.bias"], L.src(a, mode=L.PRO_LEAKY), B, h, w, c, c)   # raw; consumers apply LeakyReLU
        saved[f"a{i}"], saved[f"z{i}"] = a, z
        cur, mode, cin = z, L.PRO_LEAKY, c
        if i < 5:
            ph, pw = sizes[i]
            p = run.empty(B, ph, pw, c)                                                  # max commutes with LeakyReLU
            run.launch("nd_maxpool2x2_nhwc_f32", z.data_ptr(), p.data_ptr(), B, h, w, c)
            saved[f"p{i}"] = p
            cur = p
    for j, c in zip(range(6, 10), reversed(LSID_STAGES[:-1])):
        i = 10 - j                                           # the encoder stage of the skip
        sh, sw = sizes[i - 1]
        hp, wp_ = sizes[i]
        wt = P[f"up{j}.weight"]                              # ConvTranspose2d(2, s=2) + crop to the skip's size (:135): (cin, c, 2, 2) -> rows (p1 p2 c'), columns cin
        m = wt.permute(2, 3, 1, 0).reshape(4 * c, cin).contiguous()
        up = run.empty(B, sh, sw, c)
        run.pointwise(L.src(cur, mode=L.PRO_LEAKY), run.pack_pw(m, cin, 4 * c), None, up, B, hp * wp_, wp_, cin, 4 * c, c, shuffle=(c, sh, sw))
        a = run.conv3x3(P[f"conv{j}_1.weight"], P[f"conv{j}_1.bias"], L.src(up, saved[f"z{i}"], L.PRO_LEAKY_SECOND), B, sh, sw, 2 * c, c)
        z = run.conv3x3(P[f"conv{j}_2.weight"], P[f"conv{j}_2.bias"], L.src(a, mode=L.PRO_LEAKY), B, sh, sw, c, c)
        saved[f"u{j}"], saved[f"a{j}"], saved[f"z{j}"] = up, a, z
        cur, cin = z, c
    y = run.empty(B, H, W, 4)
    w10 = P["conv10.weight"].reshape(4, cin).contiguous()
    run.pointwise(L.src(cur, mode=L.PRO_LEAKY), run.pack_pw(w10, cin, 4), P["conv10.bias"], y, B, H * W, W, cin, 4, 4)
    return y if head_nhwc else head_to_nchw(run, y)


def head_to_nchw(run: _Launcher, y: torch.Tensor) -> torch.Tensor:
    """The network's (B, 4, H, W) output from the head's (B, H, W, 4)."""
    B, H, W, _ = y.shape
    out = run.empty(B, 4, H, W)
    run.launch("nd_nhwc_to_nchw_f32", y.data_ptr(), out.data_ptr(), B, 4, H, W)
    return out


class _LsidPlan:
    """One input shape: the forward recorded once by lsid_forward_hip (weights packed, buffers allocated), replayed on the plan's own HIP stream."""

    def __del__(self):                      # the plan owns its HIP stream
        s, self.stream = getattr(self, "stream", None), None
        if s:
            try:
                L.call("nd_stream_sync", s)
                L.call("nd_stream_destroy", s)
            except Exception:               # interpreter shutdown: the library or the device may already be gone
                pass

    def __init__(self, net: LSID, dev: torch.device, B: int, H: int, W: int):
        self.dev = dev
        with torch.cuda.device(dev), torch.inference_mode(False):
            s = C.c_void_p()
            L.call("nd_stream_create", C.byref(s))
            self.stream = s
            P = {k: v.detach().to(dev, torch.float32).contiguous() for k, v in net.state_dict().items()}
            self.x_nchw = torch.empty(B, 4, H, W, device=dev)
            rec = _Launcher(dev, WINO4, stream=s)
            rec.keep.append(P)                                # the packs read the weights, the recorded launches the biases
            self.out_nchw = lsid_forward_hip(P, self.x_nchw, {}, rec)
            self.ops, self.keep = rec.ops, rec.keep
            L.call("nd_stream_sync", self.stream)

    def run(self, x: torch.Tensor) -> torch.Tensor:
        with torch.cuda.device(self.dev):
            self.x_nchw.copy_(x.to(self.dev, torch.float32))
            torch.cuda.synchronize(self.dev)
            for fn, args, name in self.ops:
                r = fn(*args)
                if r != 0:
                    L.check(r, name)
            L.call("nd_stream_sync", self.stream)
            return self.out_nchw.clone()
