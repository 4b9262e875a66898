"""Training on MI355X, first slice: the 3x3 convolutions of a differentiable network -- 85 % of the FLOPs of
``GaussianDiffusion.p_losses`` (models/denoising_diffusion_pytorch.py:481-531) -- forward AND backward on the HIP library.

    model = <the reference NoiseDiffNet, or any nn.Module>            # differentiable PyTorch
    noisediff_amd.train.accelerate(model)                             # every nn.Conv2d(3x3, padding 1, stride 1) -> HIP
    loss = noisediff_amd.GaussianDiffusion(model, ...)(img, condition); loss.backward()

``Conv3x3Function`` is a ``torch.autograd.Function`` over the C ABI:
  * forward      nd_conv3x3_{wino4, wino2, direct}_nhwc_f32 (the sampling path's kernels, chosen by ``conv3x3_kind``)
  * grad input   the SAME forward kernels on weights packed from ``w.flip(2, 3).transpose(0, 1)`` -- the data gradient of a
                 stride-1 "same" convolution is that convolution with the taps flipped and the channel roles swapped
                 (nd_pack_conv3x3_*_weight_dgrad read the forward weight that way in place)
  * grad weight  nd_conv3x3_wgrad_nhwc_f32 (conv3x3_wgrad.hip: nine tap GEMMs over the pixels on the fp32 MFMA, fixed
                 summation order, no atomics)
  * grad bias    falls out of the weight-gradient kernel's staged dY tiles
Tensors stay what PyTorch hands over: NCHW-shaped, ``channels_last`` in memory (= the library's NHWC; other layouts are
converted once per call), fp32, on the caller's CUDA stream -- so autograd's stream ordering holds without synchronisation.
``GroupNormFunction`` (second slice) does the same for nn.GroupNorm: nd_groupnorm_train_forward_f32 / _backward_f32 (norm_train.hip) stream
the channels_last tensors once per pass, where PyTorch's NCHW group norm first copies them to NCHW and back -- on the full-resolution
blocks the norms cost more than the convolutions before this.  ``LinearFunction`` (third slice) keeps the output and the data
gradient of token Linears / 1x1 convolutions on the library GEMM and takes their weight and bias gradient -- a reduction over up to
10^6 tokens that library GEMMs run at a tenth of HBM speed -- to nd_linear_wgrad_f32 (linear_wgrad.hip); ``LayerNormFunction``:
nn.LayerNorm over token channels forward and backward (norm_train.hip).  ``attention_core`` / ``linear_attention_core`` / ``rms_norm``: the cores of
Attention and LinearAttention and their RMSNorm, forward and backward (attn_train.hip).  Activations stay on PyTorch's own ROCm kernels.
``diffusion_noising`` / ``diffusion_loss``: the two ends of ``GaussianDiffusion.forward`` around the network (diffusion_train.hip) -- timestep, noising and
target in one launch from a counter-based Philox stream, the weighted loss in fp64 in a fixed order, its gradient in one pass.
``denoise_loss``: the denoiser trainer's mse * lambda_mse + l1 * lambda_l1 the same way (denoise_loss.hip); ``lsid_train`` fuses it with LSID's head.

There is no fallback: a CPU tensor or a missing library raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable
from torch import nn

from . import _lib as L
from ._host import (CONV3X3, _empty, _need_gpu, _on, _stream, _workspace, conv3x3_kind, conv3x3_trains, conv3x3_wgrad_cat_takes, group_norm_takes,
                    layer_norm_takes, pointwise_takes, rms_norm_takes, token_sum_takes)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """NCHW-shaped tensor whose memory is NHWC (channels_last), fp32, contiguous in that format."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous(memory_format=torch.channels_last)


_SPLIT_K = __import__("os").environ.get("ND_TRAIN_SPLITK", "1") != "0"      # A/B knob (tools/): 0 = never the split-K form of conv3x3_wino4


def _pack_pointwise(w_ptr: int, packed_ptr: int, cin: int, cout: int, transposed: bool, st) -> None:
    """The operand of nd_pointwise_gemm_nhwc_f32 from a Linear / 1x1 weight (cout, cin); ``transposed``: from the FORWARD weight (cin, cout) of the layer
    whose data gradient dx = dy @ w the GEMM is, read in place."""
    if transposed:
        L.call("nd_pack_pointwise_weight_t", w_ptr, packed_ptr, cin, cout, st)
    else:
        L.call("nd_pack_pointwise_weight", w_ptr, packed_ptr, cin, cout, 0, st)       # (0: no pixel-unshuffled input channels)


def _pack_conv3x3(kind: str, w_ptr: int, packed_ptr: int, cin: int, cout: int, dgrad: bool, st) -> None:
    """The operand of the ``kind`` kernel (conv3x3_kind) from an OIHW weight; ``dgrad``: the data gradient's, read in place from the FORWARD weight
    (cin / cout are the operator's)."""
    L.call(CONV3X3[kind].pack + ("_dgrad" if dgrad else ""), w_ptr, packed_ptr, cin, cout, st)


def _conv3x3_nhwc(x: torch.Tensor, w_oihw: torch.Tensor, bias: Optional[torch.Tensor], dgrad: bool = False, stats: bool = False,
                  x1: Optional[torch.Tensor] = None):
    """y = conv2d(x, w, bias, padding=1) on the HIP library; x (B, cin, H, W) channels_last, returns (B, cout, H, W) channels_last.
    ``dgrad``: ``w_oihw`` is the FORWARD layer's weight and the operator is its data gradient, conv2d(x, w.flip(2, 3).transpose(0, 1),
    padding=1) -- the pack kernels read the flipped / role-swapped weight in place (nd_pack_conv3x3_*_weight_dgrad).
    ``stats``: returns (y, st, sc) with the kernel's GroupNorm statistics epilogue -- per-(sample, slot, channel) {sum, M2} partials ``st`` and the
    pixel counts ``sc`` of the slots, what nd_groupnorm_finalize*_f32 pools."""
    lib = L.load()
    B, cin, H, W = x.shape
    c0 = cin
    if x1 is not None:                                                   # the virtual concatenation cat((x, x1), 1): the kernels read both sources (nd_src.p0 / p1)
        if x1.shape[0] != B or tuple(x1.shape[2:]) != (H, W) or x1.device != x.device or dgrad:
            raise ValueError(f"conv3x3: second source {tuple(x1.shape)} does not extend {tuple(x.shape)}")
        cin = c0 + x1.shape[1]
    cout = w_oihw.shape[1 if dgrad else 0]
    if w_oihw.shape[0 if dgrad else 1] != cin:
        raise ValueError(f"conv3x3: x {tuple(x.shape)} does not match weight {tuple(w_oihw.shape)}" + (" (data gradient)" if dgrad else ""))
    _need_gpu(x)
    if cin % 4 or cout % 4:
        raise L.HipError(f"conv3x3 on the HIP library needs channel counts that are multiples of 4 (cin={cin}, cout={cout})")
    st = _stream(x.device)
    wbase = _PackCache._base(w_oihw) if _PackCache.cacheable(w_oihw) else None     # a parameter: the packing lives until the optimizer changes it, all stale ones repacked in one launch
    cached = wbase is not None
    w_oihw = w_oihw.detach().to(torch.float32).contiguous()
    with _on(x.device):
        out = _empty((B, cout, H, W), x.device, memory_format=torch.channels_last)
        kind = conv3x3_kind(B, H, W, cin, cout, c0, cin - c0, cin)       # ld = c0 + c1 for a concat: stricter than the kernel's widest-source bound
        if x1 is not None and (kind != "wino4" or x1.shape[1] % 16):
            raise L.HipError(f"conv3x3 over two sources needs the F(4x4) kernel and sources of whole 16-channel chunks ({c0} + {x1.shape[1]} channels, {H}x{W})")
        kind = "direct" if kind == "wino" else kind                      # past wino2's limits: the direct kernel
        if kind == "direct" and cin % 8:
            raise L.HipError(f"conv3x3 on the HIP library needs cin % 8 == 0 (cin={cin})")
        k, wino4 = CONV3X3[kind], kind == "wino4"
        if wino4 and cached:
            wptr = _pack_cache(x.device).get(w_oihw, cin, cout, dgrad, st, kind="w4", base=wbase)
        else:
            wp = _workspace(k.pack + "_floats", x.device, cin, cout)
            _pack_conv3x3(kind, w_oihw.data_ptr(), wp.data_ptr(), cin, cout, dgrad, st)
            wptr = wp.data_ptr()
        b = None if bias is None else bias.detach().to(torch.float32).contiguous()
        st_t = sc_t = None
        if stats:                                                 # (the split-K form leaves the same slots from its reduction kernel)
            slots = int(k.stat_slots(lib, B, H, W, cout))
            st_t, sc_t = _empty((B, slots, cout, 2), x.device), _empty(slots, x.device)
        d = L.conv3x3(L.src(x, x1, L.PRO_NONE, c0, c0, 0, cin - c0, cin - c0), wptr, b, out, B, H, W, cin, cout, None, st_t, sc_t)
        splits = int(lib.nd_conv3x3_wino4_splitk_plan(B, H, W, cin, cout)) if wino4 and _SPLIT_K else 1
        if splits > 1:      # few (sample, region, cout tile) items for 256 CUs (the deep layers at training batch sizes): cut along cin
            ws = _workspace("nd_conv3x3_wino4_splitk_workspace_floats", x.device, B, H, W, cout, splits)
            L.call("nd_conv3x3_wino4_splitk_nhwc_f32", C.byref(d), ws.data_ptr(), splits, st)
        else:
            L.call(k.entry, C.byref(d), st)
        # wp / b are dropped on return: safe, because the kernels were enqueued on torch's CURRENT stream and the caching
        # allocator reuses a block only for work that is enqueued later on that same stream
    return (out, st_t, sc_t) if stats else out


def _conv3x3_forward(ctx, xn, weight, bias, want_stats, x1=None):
    """The forward of Conv3x3Function / Conv3x3CatFunction (``x1``: the second source); ``want_stats``: (y, st, sc) with the statistics epilogue."""
    ctx.has_bias = bias is not None
    if not want_stats:
        return _conv3x3_nhwc(xn, weight, bias, x1=x1)
    y, st, sc = _conv3x3_nhwc(xn, weight, bias, stats=True, x1=x1)
    ctx.mark_non_differentiable(st, sc)
    ctx.set_materialize_grads(False)                             # no zero tensors for the statistics outputs' (never used) gradients
    return y, st, sc


def _conv3x3_wgrad(xn: torch.Tensor, g: torch.Tensor, cout: int, want_b: bool):
    """(dW (cout, cin, 3, 3), db or None) of a 3x3 convolution from its input ``xn`` and its output gradient ``g`` (both channels_last) on
    nd_conv3x3_wgrad_nhwc_f32; the bias gradient falls out of the staged dY tiles."""
    B, cin, H, W = xn.shape
    dev = xn.device
    with _on(dev):
        dw = _empty((cout, cin, 3, 3), dev)
        db = _empty(cout, dev) if want_b else None
        ws = _workspace("nd_conv3x3_wgrad_workspace_floats", dev, B, H, W, cin, cout)
        L.call("nd_conv3x3_wgrad_nhwc_f32", xn.data_ptr(), cin, g.data_ptr(), cout, dw.data_ptr(), L.ptr(db), ws.data_ptr(), B, H, W, cin, cout, _stream(dev))
    return dw, db


class Conv3x3Function(torch.autograd.Function):
    """nn.Conv2d(cin, cout, 3, padding=1) forward and backward on libnoisediff_hip."""

    @staticmethod
    def forward(ctx, x, weight, bias, want_stats=False):
        xn = _nhwc(x)
        ctx.save_for_backward(xn, weight)
        return _conv3x3_forward(ctx, xn, weight, bias, want_stats)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *unused):
        xn, weight = ctx.saved_tensors
        if grad_out is None:                                     # (materialize_grads is off for the statistics variant)
            return None, None, None, None
        g = _nhwc(grad_out)
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            # dL/dx = conv(dL/dy, flip(w)^T): the forward operator itself, its weight packed straight from the forward layer's
            grad_x = _conv3x3_nhwc(g, weight, None, dgrad=True)
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            grad_w, grad_b = _conv3x3_wgrad(xn, g, weight.shape[0], want_b)
        elif want_b:
            grad_b = g.sum(dim=(0, 2, 3))
        return grad_x, grad_w, grad_b, None


def _check_conv3x3(x: torch.Tensor, weight: torch.Tensor) -> None:
    if tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"conv3x3: x {tuple(x.shape)} / weight {tuple(weight.shape)} is not a 3x3 convolution")


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable F.conv2d(x, weight, bias, padding=1) for 3x3 kernels on the HIP library."""
    _check_conv3x3(x, weight)
    return Conv3x3Function.apply(x, weight, bias)


def conv3x3_with_stats(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """conv3x3 plus the kernel's GroupNorm statistics epilogue: (y, (st, sc)) for ``group_norm_silu(y, ..., conv_stats=)`` -- the norm then needs no
    pass of its own over y for its moments, as in the sampling engine (Block: conv -> statistics -> finalize -> apply); the split-K form of the deep
    layers leaves the same slots from its reduction kernel."""
    _check_conv3x3(x, weight)
    y, st, sc = Conv3x3Function.apply(x, weight, bias, True)
    return y, (st, sc)


def cat_sources_ok(x0: torch.Tensor, x1: torch.Tensor, cout: Optional[int] = None) -> bool:
    """Can conv3x3_cat / conv1x1_cat take this pair (else the caller concatenates)?  The F(4x4) kernel's geometry and whole 16-channel chunks per source;
    ``cout`` (when given): one the layer can train with (conv3x3_trains; within the kernel's bias table: conv3x3_kind's question)."""
    B, c0, H, W = x0.shape
    c1 = x1.shape[1]
    if cout is not None and not conv3x3_trains(c0 + c1, cout):
        return False
    return (x0.is_cuda and x1.is_cuda and x0.dim() == 4 and tuple(x1.shape[2:]) == (H, W) and x1.shape[0] == B and c1 % 16 == 0
            and conv3x3_kind(B, H, W, c0 + c1, cout or 8, c0, c1, c0 + c1) == "wino4")      # ld = c0 + c1 as in _conv3x3_nhwc; no cout: 8


class Conv3x3CatFunction(torch.autograd.Function):
    """conv3x3(torch.cat((x0, x1), 1), weight, bias) without the concatenated tensor: the up path's ``cat((x, skip))`` in front of a ResnetBlock
    (Diffusion_arch.py:620-630).  Forward: the kernel reads both sources (nd_src.p0 / p1).  Backward: one data gradient of c0 + c1 channels whose channel
    slices are the two inputs' gradients; the weight gradient per source, joined along cin."""

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, want_stats=False):
        a, b = _nhwc(x0), _nhwc(x1)
        ctx.save_for_backward(a, b, weight)
        return _conv3x3_forward(ctx, a, weight, bias, want_stats, x1=b)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, *unused):
        a, b, weight = ctx.saved_tensors
        if grad_out is None:
            return None, None, None, None, None
        g = _nhwc(grad_out)
        B, c0, H, W = a.shape
        c1, cout = b.shape[1], weight.shape[0]
        gx0 = gx1 = grad_w = grad_b = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            full = _conv3x3_nhwc(g, weight, None, dgrad=True)            # (B, c0 + c1, H, W) channels_last: the slices are views
            gx0, gx1 = (full[:, :c0] if ctx.needs_input_grad[0] else None), (full[:, c0:] if ctx.needs_input_grad[1] else None)
        want_b = ctx.has_bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2] and conv3x3_wgrad_cat_takes(B, H, W, c0, c1, cout):
            with _on(a.device):                                          # the Winograd-domain forms read a cin block from either source: ONE weight gradient
                grad_w = _empty((cout, c0 + c1, 3, 3), a.device)
                grad_b = _empty(cout, a.device) if want_b else None
                ws = _workspace("nd_conv3x3_wgrad_workspace_floats", a.device, B, H, W, c0 + c1, cout)
                L.call("nd_conv3x3_wgrad_cat_nhwc_f32", a.data_ptr(), c0, c0, b.data_ptr(), c1, c1, g.data_ptr(), cout, grad_w.data_ptr(),
                       L.ptr(grad_b), ws.data_ptr(), B, H, W, cout, _stream(a.device))
        elif ctx.needs_input_grad[2]:                                    # per source, joined along cin; the bias gradient from the first source's launch
            dw0, grad_b = _conv3x3_wgrad(a, g, cout, want_b)
            dw1, _ = _conv3x3_wgrad(b, g, cout, False)
            grad_w = torch.cat((dw0, dw1), dim=1)
        elif want_b:
            grad_b = g.sum(dim=(0, 2, 3))
        return gx0, gx1, grad_w, grad_b, None


def conv3x3_cat(x0: torch.Tensor, x1: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, with_stats: bool = False):
    """Differentiable F.conv2d(torch.cat((x0, x1), 1), weight, bias, padding=1) that never builds the concatenation (``cat_sources_ok`` says when);
    ``with_stats``: (y, (st, sc)) as conv3x3_with_stats."""
    if tuple(weight.shape[2:]) != (3, 3) or x0.shape[1] + x1.shape[1] != weight.shape[1] or not cat_sources_ok(x0, x1, weight.shape[0]):
        raise ValueError(f"conv3x3_cat: x0 {tuple(x0.shape)} + x1 {tuple(x1.shape)} / weight {tuple(weight.shape)}")
    if not with_stats:
        return Conv3x3CatFunction.apply(x0, x1, weight, bias)
    y, st, sc = Conv3x3CatFunction.apply(x0, x1, weight, bias, True)
    return y, (st, sc)


class GroupNormFunction(torch.autograd.Function):
    """nn.GroupNorm(groups, C) forward and backward on libnoisediff_hip (norm_train.hip), channels_last in and out."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps):
        xn = _nhwc(x)
        _need_gpu(xn)
        B, C_, H, W = xn.shape
        st = _stream(xn.device)
        with _on(xn.device):
            y = torch.empty_like(xn, memory_format=torch.channels_last)
            mean_rstd = _empty((B, groups, 2), xn.device)
            ws = _workspace("nd_groupnorm_train_workspace_floats", xn.device, B, H * W, C_)
            w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
            L.call("nd_groupnorm_train_forward_f32", xn.data_ptr(), C_, w32.data_ptr(), b32.data_ptr(), y.data_ptr(), C_, mean_rstd.data_ptr(),
                   ws.data_ptr(), B, H * W, C_, groups, float(eps), st)
        ctx.save_for_backward(xn, weight, mean_rstd)
        ctx.groups = groups
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xn, weight, mean_rstd = ctx.saved_tensors
        g = _nhwc(grad_out)
        B, C_, H, W = xn.shape
        with _on(xn.device):
            dx = torch.empty_like(xn, memory_format=torch.channels_last)
            dgamma = _empty(C_, xn.device)
            dbeta = _empty(C_, xn.device)
            ws = _workspace("nd_groupnorm_train_workspace_floats", xn.device, B, H * W, C_)
            w32 = weight.detach().float().contiguous()
            L.call("nd_groupnorm_train_backward_f32", g.data_ptr(), C_, xn.data_ptr(), C_, w32.data_ptr(), mean_rstd.data_ptr(), dx.data_ptr(), C_,
                   dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), B, H * W, C_, ctx.groups, _stream(xn.device))
        return dx, dgamma, dbeta, None, None


def group_norm(x: torch.Tensor, groups: int, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """Differentiable F.group_norm(x, groups, weight, bias, eps) for 4-D inputs on the HIP library."""
    if x.dim() != 4 or not group_norm_takes(x.shape[1], groups) or weight is None or bias is None:
        raise ValueError(f"group_norm: x {tuple(x.shape)}, groups {groups}: needs a 4-D input, channels and groups that nd_groupnorm_train_takes, affine parameters")
    return GroupNormFunction.apply(x, weight, bias, groups, eps)


class GroupNormSiLUFunction(torch.autograd.Function):
    """y = silu(GroupNorm(x) * (scale + 1) + shift) -- Block's tail (Diffusion_arch.py:137-143) -- as one operator on libnoisediff_hip
    (norm_train.hip); ``scale_shift`` is the (B, 2C) output of ResnetBlock.mlp (scale | shift) or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, scale_shift, res, groups, eps, st=None, sc=None):
        xn = _nhwc(x)
        rn = None if res is None else _nhwc(res)
        _need_gpu(xn)
        B, C_, H, W = xn.shape
        ss = None if scale_shift is None else scale_shift.detach().reshape(B, 2 * C_).float().contiguous()
        with _on(xn.device):
            y = torch.empty_like(xn, memory_format=torch.channels_last)
            mean_rstd = _empty((B, groups, 2), xn.device)
            mad = _empty((B, 3, C_), xn.device)
            ws = _workspace("nd_groupnorm_silu_train_workspace_floats", xn.device, B, H * W, C_)
            w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
            if st is not None:       # the convolution's statistics epilogue already holds the partial moments: finalize (saving mean / rstd) + one apply pass
                stp = _stream(xn.device)
                L.call("nd_groupnorm_finalize_train_f32", st.data_ptr(), sc.data_ptr(), st.shape[1], w32.data_ptr(), b32.data_ptr(),
                       None if ss is None else ss.data_ptr(), 2 * C_, mad.data_ptr(), mean_rstd.data_ptr(), B, C_, groups, float(eps), stp)
                L.call("nd_affine_silu_add_f32", xn.data_ptr(), C_, mad.data_ptr(), None if rn is None else rn.data_ptr(), C_, None, 0, y.data_ptr(), C_,
                       B, H * W, C_, stp)
            else:
                L.call("nd_groupnorm_silu_train_forward_f32", xn.data_ptr(), C_, w32.data_ptr(), b32.data_ptr(), None if ss is None else ss.data_ptr(),
                       None if rn is None else rn.data_ptr(), C_, y.data_ptr(), C_, mean_rstd.data_ptr(), mad.data_ptr(), ws.data_ptr(), B, H * W, C_, groups, float(eps), _stream(xn.device))
        ctx.save_for_backward(xn, weight, bias, mean_rstd, mad, ss if ss is not None else mean_rstd.new_empty(0))
        ctx.groups, ctx.has_ss, ctx.ss_shape = groups, ss is not None, None if scale_shift is None else scale_shift.shape
        ctx.has_res = res is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xn, weight, bias, mean_rstd, mad, ss = ctx.saved_tensors
        g = _nhwc(grad_out)
        B, C_, H, W = xn.shape
        with _on(xn.device):
            dx = torch.empty_like(xn, memory_format=torch.channels_last)
            dgamma = _empty(C_, xn.device)
            dbeta = _empty(C_, xn.device)
            dss = _empty((B, 2 * C_), xn.device) if ctx.has_ss else None
            ws = _workspace("nd_groupnorm_silu_train_workspace_floats", xn.device, B, H * W, C_)
            w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
            L.call("nd_groupnorm_silu_train_backward_f32", g.data_ptr(), C_, xn.data_ptr(), C_, w32.data_ptr(), b32.data_ptr(),
                   ss.data_ptr() if ctx.has_ss else None, mean_rstd.data_ptr(), mad.data_ptr(), dx.data_ptr(), C_, dgamma.data_ptr(), dbeta.data_ptr(),
                   dss.data_ptr() if ctx.has_ss else None, ws.data_ptr(), B, H * W, C_, ctx.groups, _stream(xn.device))
        return dx, dgamma, dbeta, (dss.view(ctx.ss_shape) if ctx.has_ss else None), (grad_out if ctx.has_res else None), None, None, None, None


def group_norm_silu(x: torch.Tensor, groups: int, weight: torch.Tensor, bias: torch.Tensor, scale_shift: Optional[torch.Tensor] = None,
                    eps: float = 1e-5, res: Optional[torch.Tensor] = None, conv_stats=None) -> torch.Tensor:
    """Differentiable silu(F.group_norm(x, groups, weight, bias, eps) * (scale + 1) + shift) (+ res), scale | shift = the halves of ``scale_shift``
    ((B, 2C) or (B, 2C, 1, 1)), on the HIP library; ``res`` (x's shape): the ResnetBlock's shortcut added in the same pass (Diffusion_arch.py:170)."""
    if x.dim() != 4 or not group_norm_takes(x.shape[1], groups) or weight is None or bias is None:
        raise ValueError(f"group_norm_silu: x {tuple(x.shape)}, groups {groups}: needs a 4-D input, channels and groups that nd_groupnorm_train_takes, affine parameters")
    if scale_shift is not None and scale_shift.numel() != x.shape[0] * 2 * x.shape[1]:
        raise ValueError(f"group_norm_silu: scale_shift {tuple(scale_shift.shape)} is not (B, 2C) for x {tuple(x.shape)}")
    if res is not None and res.shape != x.shape:
        raise ValueError(f"group_norm_silu: res {tuple(res.shape)} does not match x {tuple(x.shape)}")
    if conv_stats is not None:       # (st, sc) of conv3x3_with_stats for THIS x: the partial moments of the producing convolution's epilogue
        return GroupNormSiLUFunction.apply(x, weight, bias, scale_shift, res, groups, eps, conv_stats[0], conv_stats[1])
    return GroupNormSiLUFunction.apply(x, weight, bias, scale_shift, res, groups, eps)


class BroadcastAddFunction(torch.autograd.Function):
    """tokens (B, N, C) + vec (B, 1, C): AttnBlock's one-token cross attention adds the same vector to every token (Diffusion_arch.py:435-437).  The
    gradient of ``vec`` is a sum over the tokens: nd_token_sum_f32 (fixed order) instead of ATen's reduction over a middle dimension."""

    @staticmethod
    def forward(ctx, tokens, vec):
        ctx.vec_shape = vec.shape
        return tokens + vec

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        B, N, C_ = grad_out.shape
        g = grad_out if grad_out.is_contiguous() and grad_out.dtype == torch.float32 else grad_out.float().contiguous()
        grad_vec = None
        if ctx.needs_input_grad[1]:
            with _on(g.device):
                grad_vec = _empty((B, C_), g.device)
                ws = _workspace("nd_token_sum_workspace_floats", g.device, B, N, C_)
                L.call("nd_token_sum_f32", g.data_ptr(), C_, grad_vec.data_ptr(), ws.data_ptr(), B, N, C_, _stream(g.device))
            grad_vec = grad_vec.view(ctx.vec_shape)
        return grad_out, grad_vec


def broadcast_add(tokens: torch.Tensor, vec: torch.Tensor) -> torch.Tensor:
    """tokens (B, N, C) + vec (B, 1, C) with the token sum of the backward on the HIP library (a width that nd_token_sum_takes; CUDA tensors)."""
    if tokens.dim() != 3 or vec.shape != (tokens.shape[0], 1, tokens.shape[2]) or not token_sum_takes(tokens.shape[2]) or not tokens.is_cuda:
        return tokens + vec
    return BroadcastAddFunction.apply(tokens, vec)


class ModulateSiLUFunction(torch.autograd.Function):
    """y = silu(n * (scale + 1) + shift) with per-pixel maps (ResnetBlock2, Diffusion_arch.py:188-192): ``n`` (B, C, H, W) the GroupNorm's output,
    ``ss`` (B, 2C, H, W) = scale | shift as ResnetBlock2.mlp emits it; one pass forward, one backward (nd_modulate_silu_*_f32)."""

    @staticmethod
    def forward(ctx, n, ss):
        nn_, sn = _nhwc(n), _nhwc(ss)
        _need_gpu(nn_)
        B, C_, H, W = nn_.shape
        with _on(nn_.device):
            y = torch.empty_like(nn_, memory_format=torch.channels_last)
            L.call("nd_modulate_silu_forward_f32", nn_.data_ptr(), C_, sn.data_ptr(), 2 * C_, y.data_ptr(), C_, B * H * W, C_, _stream(nn_.device))
        ctx.save_for_backward(nn_, sn)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        nn_, sn = ctx.saved_tensors
        g = _nhwc(grad_out)
        B, C_, H, W = nn_.shape
        with _on(nn_.device):
            dn = torch.empty_like(nn_, memory_format=torch.channels_last)
            dss = torch.empty_like(sn, memory_format=torch.channels_last)
            L.call("nd_modulate_silu_backward_f32", g.data_ptr(), C_, nn_.data_ptr(), C_, sn.data_ptr(), 2 * C_, dn.data_ptr(), C_, dss.data_ptr(), 2 * C_,
                   B * H * W, C_, _stream(nn_.device))
        return dn, dss


def modulate_silu(n: torch.Tensor, scale_shift: torch.Tensor) -> torch.Tensor:
    """Differentiable silu(n * (scale + 1) + shift), scale | shift = the channel halves of the per-pixel map ``scale_shift`` (B, 2C, H, W)."""
    if n.dim() != 4 or scale_shift.dim() != 4 or scale_shift.shape != (n.shape[0], 2 * n.shape[1], n.shape[2], n.shape[3]) or n.shape[1] % 4:
        raise ValueError(f"modulate_silu: n {tuple(n.shape)} / scale_shift {tuple(scale_shift.shape)}: needs (B, C, H, W) and (B, 2C, H, W), C a multiple of 4")
    return ModulateSiLUFunction.apply(n, scale_shift)


def _eligible_norm(m: nn.Module) -> bool:
    return isinstance(m, nn.GroupNorm) and m.affine and group_norm_takes(m.num_channels, m.num_groups)


def _hip_norm_forward(self: nn.GroupNorm, x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 4:                                                     # (the reference applies GroupNorm to images only)
        return torch.nn.functional.group_norm(x, self.num_groups, self.weight, self.bias, self.eps)
    return group_norm(x, self.num_groups, self.weight, self.bias, self.eps)


# Output and data gradient of Linears / 1x1 convolutions: the sampling path's pointwise kernels (nd_pointwise_gemm_nhwc_f32), since r5 by default --
# no library GEMM (rocBLAS / hipBLASLt) is left in a training step.  The packed operands are cached per weight and refreshed when the parameter's
# version changes: ONE launch per optimizer step packs every stale weight (nd_pack_pointwise_weights_batch), where r3 packed per call (178 GEMMs,
# 0.77 ms of 4-microsecond launches per step -- that, not the GEMMs, was what lost to the library then).  ND_TRAIN_PW=0 (or train._PW_GEMM = False):
# the library GEMM, as an A/B knob.
_PW_GEMM = __import__("os").environ.get("ND_TRAIN_PW", "1") != "0"


class _PackEntry:
    """One cached packing: ``param`` the nn.Parameter it was packed from (held strongly: see _PackCache), ``buf`` the packed operand, ``version`` the
    parameter's version counter at the last packing (-1: stale), ``flag`` the data-gradient form, ``volatile``: packed while a stream was capturing."""
    __slots__ = ("param", "buf", "version", "cin", "cout", "flag", "volatile")

    def __init__(self, param: nn.Parameter, buf: torch.Tensor, cin: int, cout: int, flag: bool):
        self.param, self.buf, self.version, self.cin, self.cout, self.flag, self.volatile = param, buf, -1, cin, cout, flag, False


class _PackCache:
    """Packed operands of one device's weights: the Linear / 1x1 weights (kind "pw": nd_pack_pointwise_weight, ``flag`` = the transposed data-gradient
    packing) and the 3x3 weights on the F(4x4) kernels (kind "w4": nd_pack_conv3x3_wino4_weight, ``flag`` = the data-gradient form).  An entry belongs
    to an ``nn.Parameter`` (or a view of one: ``weight.flatten(1)`` of a 1x1 convolution): key (kind, data_ptr, shape, flag), valid while the parameter's
    version counter stands.  The first stale entry of a kind that a step meets repacks EVERY stale entry of that kind in one launch over a descriptor
    table kept in device memory.  Anything that is not a parameter (the per-step torch.cat of the stacked time projections, nn.DataParallel's
    broadcast copies, a padded temporary under no_grad) is packed per call and never cached.

    What the version counter does NOT see -- call ``train.invalidate_packs()`` after any of these, before the next eager forward:
      * writes through ``.data`` (``p.data.copy_ / lerp_ / normal_``: ema_pytorch's update of its shadow model, SID_arch's re-initialisation);
      * replays of a captured whole-step graph: the optimizer inside it moves the parameters without bumping a version.  Entries that were packed
        while a stream was capturing are flagged ``volatile`` and repacked on EVERY eager use from then on, so the sequence replay / eager forward /
        replay never computes with a packing from before the last update even without the call.
    An entry holds its parameter (as in r5): a deleted model's weights and packings stay in GPU memory until ``train.release_packs()`` is called (or 4096
    entries accumulate).  r6 tried weak references here: the full GPU suite then ended in a GPU memory access fault in a later test's backward
    pass on two of three runs -- freeing those models changes which pages of the caching allocator stay mapped, and some access of the training path (not
    found in the time of the round) reaches into them; with the r5 lifetime the suite is green as it was.  Entries whose parameter has MOVED (module.to(),
    p.data = ...) are dropped: their address is no longer the parameter's."""
    _FLOATS = {"pw": "nd_pack_pointwise_weight_floats", "w4": "nd_pack_conv3x3_wino4_weight_floats"}
    _BATCH = {"pw": "nd_pack_pointwise_weights_batch", "w4": "nd_pack_conv3x3_wino4_weights_batch"}

    def __init__(self, device: torch.device):
        self.device = device
        self._last_table: Dict[str, torch.Tensor] = {}       # the table of each kind's last batched repack: alive until the next one (the launch is asynchronous)
        self._reset()

    def _reset(self) -> None:
        self.entries: Dict[tuple, _PackEntry] = {}
        self.tables: Dict[str, Optional[torch.Tensor]] = {"pw": None, "w4": None}     # device copies of the nd_pack_item records, in the order of `order`
        self.order: Dict[str, list] = {"pw": [], "w4": []}

    @staticmethod
    def _base(w: torch.Tensor):
        """The nn.Parameter behind ``w``: itself, or the root of a view of it (``p.detach()``, ``p.flatten(1)``, ``p.detach().flatten(1)``); else None."""
        if isinstance(w, torch.nn.Parameter):
            return w
        b = w._base if w._is_view() else None
        return b if isinstance(b, torch.nn.Parameter) else None

    @staticmethod
    def cacheable(w: torch.Tensor) -> bool:
        return w.dtype == torch.float32 and w.is_contiguous() and w.is_cuda and _PackCache._base(w) is not None

    def _drop(self, key: tuple) -> None:
        self.entries.pop(key, None)
        kind = key[0]
        if key in self.order[kind]:
            self.order[kind].remove(key)
        self.tables[kind] = None

    def invalidate(self) -> None:
        for e in self.entries.values():
            e.version = -1

    def get(self, w: torch.Tensor, cin: int, cout: int, flag: bool, st, kind: str = "pw", base=None) -> int:
        """Device pointer of the packing of ``w`` (``base``: the parameter behind it where the caller has already detached ``w``)."""
        key = (kind, w.data_ptr(), tuple(w.shape), flag)
        base = base if base is not None else self._base(w)
        if base is None:
            raise L.HipError("_PackCache.get: not a parameter (check cacheable() first)")
        e = self.entries.get(key)
        if e is not None and e.param is not base:            # the parameter that owned this address is gone (or replaced): the entry goes with it
            self._drop(key)
            e = None
        if e is None:
            if len(self.entries) >= 4096:            # (a model is a few hundred weights: anything beyond is a leak -- start over)
                self._reset()
            e = self.entries[key] = _PackEntry(base, _workspace(self._FLOATS[kind], self.device, cin, cout), cin, cout, flag)
            self.order[kind].append(key)
            self.tables[kind] = None
        capturing = torch.cuda.is_current_stream_capturing()
        if e.version != base._version or (e.volatile and not capturing):
            if e.volatile and not capturing:
                e.version = -1                       # packed inside a captured graph: replays may have moved the weight since, unseen by the version counter
            self._repack_stale(kind, st)
        return e.buf.data_ptr()

    def _pack_one(self, kind: str, key, e: _PackEntry, st) -> None:
        if kind == "pw":
            _pack_pointwise(key[1], e.buf.data_ptr(), e.cin, e.cout, e.flag, st)
        else:
            _pack_conv3x3("wino4", key[1], e.buf.data_ptr(), e.cin, e.cout, e.flag, st)

    def _repack_stale(self, kind: str, st) -> None:
        def gone(k):
            # the parameter's storage has moved (module.to(), p.data = ...) and the address this entry was keyed on is no longer inside it: the entry must
            # not be repacked from that address
            base = self.entries[k].param
            lo = base.data_ptr()
            return not (lo <= k[1] < lo + max(base.numel(), 1) * base.element_size())
        for k in [k for k in self.order[kind] if gone(k)]:
            self._drop(k)
        order = self.order[kind]
        stale = [k for k in order if self.entries[k].version != self.entries[k].param._version]
        capturing = torch.cuda.is_current_stream_capturing()
        if (self.tables[kind] is None or len(stale) != len(order)) and capturing:
            # a new descriptor table would need a host-to-device copy, which a capturing stream refuses: one capturable launch per stale weight instead
            for k in stale:
                e = self.entries[k]
                self._pack_one(kind, k, e, st)
                e.version, e.volatile = e.param._version, True
            return
        if self.tables[kind] is None or len(stale) != len(order):
            # first use, or only part of the table is stale (a partially frozen model): a table of the stale entries only
            items = (L.PackItem * len(stale))()
            for i, k in enumerate(stale):
                e = self.entries[k]
                items[i].w, items[i].packed, items[i].cin, items[i].cout, items[i].transposed = k[1], e.buf.data_ptr(), e.cin, e.cout, int(e.flag)
            host = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
            table = host.to(self.device)                     # (synchronous copy of a few KB)
            if len(stale) == len(order):
                self.tables[kind] = table
        else:
            table = self.tables[kind]
        L.call(self._BATCH[kind], table.data_ptr(), len(stale), st)
        self._last_table[kind] = table
        for k in stale:
            e = self.entries[k]
            e.version = e.param._version
            if capturing:
                e.volatile = True


_PACK_CACHES: Dict[int, _PackCache] = {}


def _pack_cache(device: torch.device) -> _PackCache:
    cache = _PACK_CACHES.get(device.index)
    if cache is None:
        cache = _PACK_CACHES[device.index] = _PackCache(device)
    return cache


def release_packs(device: Optional[torch.device] = None) -> None:
    """Drop every cached packing (and the references to their parameters) of one device, or of all: call it when models are deleted, so that their weights
    and packings leave GPU memory; live models repack on their next forward."""
    for idx in list(_PACK_CACHES):
        if device is None or device.index == idx:
            del _PACK_CACHES[idx]


def invalidate_packs(device: Optional[torch.device] = None) -> None:
    """Mark every cached weight packing (of one device, or of all) stale: the next forward repacks them in one launch per kind.  Needed after writes the
    parameters' version counters do not see -- ``p.data.copy_ / lerp_ / normal_`` (ema_pytorch's shadow-model update, SID_arch's initialisation) -- and after
    replays of a captured whole-step graph (see _PackCache).  ``train.EMA.update()`` bumps the shadow tensors' versions itself and needs no call."""
    for idx, cache in _PACK_CACHES.items():
        if device is None or device.index == idx:
            cache.invalidate()


def _tokens(t: torch.Tensor, c: int) -> torch.Tensor:
    t = t.reshape(-1, c)
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


def _pointwise_gemm(x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], transposed: bool, x2b: Optional[torch.Tensor] = None,
                    res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[N, cout] = x2[N, cin] @ W^T (+ bias) (+ res[N, cout]) on nd_pointwise_gemm_nhwc_f32 (pointwise.hip: the sampling path's 1x1 / Linear kernels, exact-fp32
    MFMA), W = ``w`` (cout, cin); ``transposed``: W^T = ``w`` -- the forward weight of the layer whose data gradient dx = dy @ w this is (packed
    in place by nd_pack_pointwise_weight_t).  ``res``: a residual added in the kernel's epilogue (the sampling engine's res0)."""
    N, cin = x2.shape
    c0 = cin
    if x2b is not None:                                                  # tokens of a second source: the virtual concatenation cat((x2, x2b), -1)
        cin = c0 + x2b.shape[1]
    cout = w.shape[1] if transposed else w.shape[0]
    st = _stream(x2.device)
    with _on(x2.device):
        y = _empty((N, cout), x2.device)
        if _PackCache.cacheable(w):                   # a parameter (or a view of one): its packing is cached until the optimizer changes it
            wptr = _pack_cache(x2.device).get(w, cin, cout, transposed, st)
        else:
            wp = _workspace("nd_pack_pointwise_weight_floats", x2.device, cin, cout)
            w32 = w.detach().float().contiguous()
            _pack_pointwise(w32.data_ptr(), wp.data_ptr(), cin, cout, transposed, st)
            wptr = wp.data_ptr()
        b32 = None if bias is None else bias.detach().float().contiguous()
        d = L.pointwise(L.src(x2, x2b, L.PRO_NONE, c0, c0, 0, cin - c0, cin - c0), wptr, b32, y, 1, N, 1, cin, cout, res0=res, ldr0=cout)
        L.call("nd_pointwise_gemm_nhwc_f32", C.byref(d), st)
    return y


def _pw_takes(N: int, cin: int, cout: int) -> bool:
    """The GEMM of a Linear on the library's 1x1 kernel: the knob, widths the entry takes, a token count of 32 bits."""
    return _PW_GEMM and pointwise_takes(cin, cout) and 0 < N < (1 << 31) and N * max(cin, cout) * 4 < (1 << 40)


def _linear_wgrad(x2: torch.Tensor, g2: torch.Tensor, want_b: bool):
    """(dW (cout, cin), db or None) of a Linear from its input tokens ``x2`` (N, cin) and its output gradient ``g2`` (N, cout) on nd_linear_wgrad_f32
    (fixed summation order); the bias gradient is the same pass's column sums of ``g2``."""
    _need_gpu(x2)
    (N, cin), cout, dev = x2.shape, g2.shape[1], x2.device
    with _on(dev):
        dw = _empty((cout, cin), dev)
        db = _empty(cout, dev) if want_b else None
        ws = _workspace("nd_linear_wgrad_workspace_floats", dev, N, cin, cout)
        L.call("nd_linear_wgrad_f32", x2.data_ptr(), cin, g2.data_ptr(), cout, dw.data_ptr(), L.ptr(db), ws.data_ptr(), N, cin, cout, _stream(dev))
    return dw, db


def _linear_wgrad_cat(t0: torch.Tensor, t1: torch.Tensor, g2: torch.Tensor, want_b: bool):
    """_linear_wgrad of a Linear over cat((t0, t1), -1): per source, joined along cin; the bias gradient from the first source's launch only."""
    dw0, db = _linear_wgrad(_tokens(t0, t0.shape[-1]), g2, want_b)
    dw1, _ = _linear_wgrad(_tokens(t1, t1.shape[-1]), g2, False)
    return torch.cat((dw0, dw1), dim=1), db


class LinearFunction(torch.autograd.Function):
    """y = x @ W^T + b over tokens (x: (..., cin) with the tokens contiguous).  Output and data gradient are plain GEMMs (the library's; with
    ND_TRAIN_PW=1 the sampling path's pointwise kernels, nd_pointwise_gemm_nhwc_f32, the data gradient's weight packed straight from the forward
    weight); the weight and bias gradients -- a reduction over 10^5..10^6 tokens into a 64..1024-wide matrix, where library GEMMs run at a tenth of HBM speed --
    come from nd_linear_wgrad_f32 (linear_wgrad.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, res=None):
        """``res`` (optional, the shape of the output): y = x @ W^T + b + res with the addition in the GEMM's epilogue (the residual connections around the
        AttnBlock's feed-forward and ``proj_out``, Diffusion_arch.py:440-443); its gradient is the output's."""
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        cout, cin = weight.shape
        if x.is_cuda and _pw_takes(x.numel() // cin, cin, cout):
            r2 = _tokens(res, cout) if res is not None else None
            return _pointwise_gemm(_tokens(x, cin), weight, bias, False, res=r2).view(*x.shape[:-1], cout)
        y = torch.nn.functional.linear(x, weight, bias)
        return y if res is None else y + res

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        cout, cin = weight.shape
        grad_x = grad_w = grad_b = None
        g2 = _tokens(grad_out, cout)
        if ctx.needs_input_grad[0]:
            if g2.is_cuda and _pw_takes(g2.shape[0], cout, cin):
                grad_x = _pointwise_gemm(g2, weight, None, True).view(x.shape)
            else:
                grad_x = grad_out @ weight
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            grad_w, grad_b = _linear_wgrad(_tokens(x, cin), g2, ctx.has_bias)
        return grad_x, grad_w, grad_b, (grad_out if len(ctx.needs_input_grad) > 3 and ctx.needs_input_grad[3] else None)


class LinearCatFunction(torch.autograd.Function):
    """linear(torch.cat((t0, t1), -1), weight, bias) over tokens without the concatenated tensor (the 1x1 ``res_conv`` of the up path's ResnetBlocks on
    ``cat((x, skip))``): forward with two sources, one data gradient whose channel slices are the inputs' gradients, the weight gradient per source."""

    @staticmethod
    def forward(ctx, t0, t1, weight, bias):
        ctx.save_for_backward(t0, t1, weight)
        ctx.has_bias = bias is not None
        cout = weight.shape[0]
        c0, c1 = t0.shape[-1], t1.shape[-1]
        return _pointwise_gemm(_tokens(t0, c0), weight, bias, False, _tokens(t1, c1)).view(*t0.shape[:-1], cout)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        t0, t1, weight = ctx.saved_tensors
        cout, cin = weight.shape
        c0 = t0.shape[-1]
        g0 = g1 = grad_w = grad_b = None
        g2 = _tokens(grad_out, cout)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            full = _pointwise_gemm(g2, weight, None, True).view(*t0.shape[:-1], cin)
            g0, g1 = (full[..., :c0] if ctx.needs_input_grad[0] else None), (full[..., c0:] if ctx.needs_input_grad[1] else None)
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            grad_w, grad_b = _linear_wgrad_cat(t0, t1, g2, ctx.has_bias)
        return g0, g1, grad_w, grad_b


def _cat_tokens(op: str, x0: torch.Tensor, x1: torch.Tensor, weight: torch.Tensor):
    """The argument check of the 1x1 convolutions over cat((x0, x1), 1), and the two sources as contiguous NHWC tokens (views when channels_last)."""
    if x0.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or x0.shape[1] + x1.shape[1] != weight.shape[1] \
            or not pointwise_takes(weight.shape[1], weight.shape[0], x1.shape[1]) or not (x0.is_cuda and x1.is_cuda):
        raise ValueError(f"{op}: x0 {tuple(x0.shape)} + x1 {tuple(x1.shape)} / weight {tuple(weight.shape)}")
    t0, t1 = x0.permute(0, 2, 3, 1), x1.permute(0, 2, 3, 1)
    return (t0 if t0.is_contiguous() else t0.contiguous()), (t1 if t1.is_contiguous() else t1.contiguous())


def conv1x1_cat(x0: torch.Tensor, x1: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable F.conv2d(torch.cat((x0, x1), 1), weight, bias) for 1x1 kernels that never builds the concatenation (channels_last in and out; both
    channel counts nd_pointwise_gemm_takes)."""
    t0, t1 = _cat_tokens("conv1x1_cat", x0, x1, weight)
    return LinearCatFunction.apply(t0, t1, weight.flatten(1), bias).permute(0, 3, 1, 2)


class ShortcutCatFunction(torch.autograd.Function):
    """ResnetBlock.res_conv on ``cat((t0, t1), -1)`` (tokens) AND the hand-over of the two inputs to the block's first convolution: returns (t0, t1, r =
    linear(cat(t0, t1), weight, bias)).  The block reads the returned aliases, so the convolution's data gradient arrives HERE instead of being added to the
    shortcut's by autograd (one elementwise pass over a block input per source: 18 of a step's additions, 6 of them full resolution): the shortcut's own data
    gradient dr @ W takes it as the residual of its GEMM epilogue.  Diffusion_arch.py:163-170 (h + res_conv(x)) on the up path's concatenations (:620-630)."""

    @staticmethod
    def forward(ctx, t0, t1, weight, bias):
        ctx.save_for_backward(t0, t1, weight)
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        cout = weight.shape[0]
        c0, c1 = t0.shape[-1], t1.shape[-1]
        r = _pointwise_gemm(_tokens(t0, c0), weight, bias, False, _tokens(t1, c1)).view(*t0.shape[:-1], cout)
        return t0.view_as(t0), t1.view_as(t1), r

    @staticmethod
    @once_differentiable
    def backward(ctx, d0, d1, dr):
        t0, t1, weight = ctx.saved_tensors
        cout, cin = weight.shape
        c0 = t0.shape[-1]
        if dr is None:
            return d0, d1, None, None
        g2 = _tokens(dr, cout)
        g0 = g1 = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # the convolution's gradients are the two channel slices of ONE (tokens, c0 + c1) tensor (Conv3x3CatFunction.backward): the residual of the epilogue
            want, acc = [], 1                                            # strides of a contiguous (..., cin) tensor: what both slices must sit in
            for n in (cin,) + tuple(reversed(t0.shape[:-1])):
                want.insert(0, acc)
                acc *= n
            joined = (d0 is not None and d1 is not None and d0.dtype == torch.float32 and d1.dtype == torch.float32 and d0.shape == t0.shape and d1.shape == t1.shape
                      and list(d0.stride()) == want and list(d1.stride()) == want and d0.data_ptr() + 4 * c0 == d1.data_ptr() and d0.data_ptr() % 16 == 0)
            if joined:
                res = torch.as_strided(d0, (g2.shape[0], cin), (cin, 1))
                full = _pointwise_gemm(g2, weight, None, True, res=res).view(*t0.shape[:-1], cin)
                g0, g1 = full[..., :c0], full[..., c0:]
            else:
                full = _pointwise_gemm(g2, weight, None, True).view(*t0.shape[:-1], cin)
                g0 = full[..., :c0] if d0 is None else full[..., :c0] + d0
                g1 = full[..., c0:] if d1 is None else full[..., c0:] + d1
        grad_w = grad_b = None
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            grad_w, grad_b = _linear_wgrad_cat(t0, t1, g2, ctx.has_bias)
        return g0, g1, grad_w, grad_b


def conv1x1_shortcut_cat(x0: torch.Tensor, x1: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """(x0', x1', F.conv2d(torch.cat((x0, x1), 1), weight, bias)) for a ResnetBlock whose shortcut is a 1x1 convolution of a concatenation: x0' / x1' are the inputs
    again, to be read by the block's first convolution, whose data gradient then joins the shortcut's inside one GEMM (ShortcutCatFunction)."""
    t0, t1 = _cat_tokens("conv1x1_shortcut_cat", x0, x1, weight)
    a0, a1, r = ShortcutCatFunction.apply(t0, t1, weight.flatten(1), bias)
    return a0.permute(0, 3, 1, 2), a1.permute(0, 3, 1, 2), r.permute(0, 3, 1, 2)


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable F.linear(x, weight, bias) (+ res, added in the GEMM's epilogue) with the weight / bias gradient on the HIP library (widths that nd_pointwise_gemm_takes;
    nd_linear_wgrad_f32 takes the same)."""
    if weight.dim() != 2 or x.shape[-1] != weight.shape[1] or not pointwise_takes(weight.shape[1], weight.shape[0]):
        raise ValueError(f"linear: x {tuple(x.shape)} / weight {tuple(weight.shape)}: needs a 2-D weight with channel counts the library's 1x1 kernels take (nd_pointwise_gemm_takes)")
    if res is None:
        return LinearFunction.apply(x, weight, bias)
    if tuple(res.shape) != tuple(x.shape[:-1]) + (weight.shape[0],):
        raise ValueError(f"linear: residual {tuple(res.shape)} is not the output's shape {tuple(x.shape[:-1]) + (weight.shape[0],)}")
    return LinearFunction.apply(x, weight, bias, res)


def conv1x1(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable F.conv2d(x, weight, bias) (+ res, NCHW-shaped like the output) for 1x1 kernels as a Linear over the pixels (NHWC tokens; channels_last in and out)."""
    if x.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or x.shape[1] != weight.shape[1]:
        raise ValueError(f"conv1x1: x {tuple(x.shape)} / weight {tuple(weight.shape)} is not a 1x1 convolution")
    t = x.permute(0, 2, 3, 1)                                              # a view; contiguous when x is channels_last
    r = res.permute(0, 2, 3, 1) if res is not None else None
    y = linear(t if t.is_contiguous() else t.contiguous(), weight.flatten(1), bias, r)
    return y.permute(0, 3, 1, 2)                                           # NCHW-shaped, channels_last in memory


class Conv7x7Function(torch.autograd.Function):
    """The 7x7 stem over a 4-channel image (init_conv / cond_init_conv: Diffusion_arch.py:478, others_arch.py:394-398): forward on nd_conv7x7_c4_f32 (the sampling
    path's kernel), weight and bias gradient on nd_conv7x7_c4_wgrad_f32 (H % 4 == 0, W % 32 == 0, cout in {32, 48, 64, 96, 128}; r5) or, for other
    shapes, as the Linear weight gradient of the unfolded image -- dW[co, (ci, ky, kx)] = sum over the pixels of dy[pixel, co] * patch[pixel, (ci, ky, kx)] on
    nd_linear_wgrad_f32 (both: fixed summation order).  The input is an image, not an activation: its gradient is asked for
    only by callers outside the reference's training loop and then comes from PyTorch's transposed convolution."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, cin, H, W = x.shape
        cout = weight.shape[0]
        xn = x.detach().permute(0, 2, 3, 1).contiguous().float()          # NHWC, 4 channels
        st = _stream(x.device)
        with _on(x.device):
            wp = _empty(196 * cout, x.device)
            w32 = weight.detach().float().contiguous()
            L.call("nd_pack_conv7x7_weight", w32.data_ptr(), wp.data_ptr(), cout, st)
            b32 = bias.detach().float().contiguous() if bias is not None else torch.zeros(cout, dtype=torch.float32, device=x.device)
            y = _empty((B, H, W, cout), x.device)
            L.call("nd_conv7x7_c4_f32", xn.data_ptr(), wp.data_ptr(), b32.data_ptr(), y.data_ptr(), cout, B, H, W, cout, st)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y.permute(0, 3, 1, 2)                                       # NCHW-shaped, channels_last in memory

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        B, cin, H, W = x.shape
        cout = weight.shape[0]
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = torch.nn.grad.conv2d_input(x.shape, weight, grad_out, padding=3)
        want_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        ws_floats = int(L.load().nd_conv7x7_c4_wgrad_workspace_floats(B, H, W, cout)) if want_w and cin == 4 else -1      # (negative: not a shape of the kernel)
        if ws_floats >= 0:
            # nd_conv7x7_c4_wgrad_f32: the GEMM over the pixels straight from halo tiles (no unfolded image: 205 MB and two copies at B = 4, 256 x 256)
            g = _tokens(grad_out.permute(0, 2, 3, 1), cout)                 # (pixels, cout)
            xn = x.detach().permute(0, 2, 3, 1).contiguous().float()
            with _on(xn.device):
                grad_w = _empty(weight.shape, xn.device)
                grad_b = _empty(cout, xn.device) if ctx.has_bias else None
                ws = _empty(ws_floats, xn.device)
                L.call("nd_conv7x7_c4_wgrad_f32", xn.data_ptr(), g.data_ptr(), cout, grad_w.data_ptr(), L.ptr(grad_b), ws.data_ptr(), B, H, W, cout,
                       _stream(xn.device))
        elif want_w:
            g2 = _tokens(grad_out.permute(0, 2, 3, 1), cout)                # (pixels, cout)
            cols = torch.nn.functional.unfold(x.detach().float(), kernel_size=7, padding=3)      # (B, cin * 49, H W): index ci * 49 + ky * 7 + kx == weight.flatten(1)'s
            gw, grad_b = _linear_wgrad(cols.transpose(1, 2).reshape(B * H * W, cin * 49).contiguous(), g2, ctx.has_bias)
            grad_w = gw.view(weight.shape)
        return grad_x, grad_w, grad_b


def conv7x7_c4(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable F.conv2d(x, weight, bias, padding=3) for the 7x7 stem of a 4-channel image (cout a multiple of 4) on the HIP library."""
    if x.dim() != 4 or tuple(weight.shape[1:]) != (4, 7, 7) or x.shape[1] != 4 or weight.shape[0] % 4:
        raise ValueError(f"conv7x7_c4: x {tuple(x.shape)} / weight {tuple(weight.shape)}: a 7x7 convolution of a 4-channel image, cout a multiple of 4")
    return Conv7x7Function.apply(x, weight, bias)


def _eligible_linear(m: nn.Module) -> bool:
    if isinstance(m, nn.Linear):
        return pointwise_takes(m.in_features, m.out_features)
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0) and m.groups == 1
            and pointwise_takes(m.in_channels, m.out_channels))


def _hip_linear_forward(self, x: torch.Tensor) -> torch.Tensor:
    if isinstance(self, nn.Linear):
        return linear(x, self.weight, self.bias)
    return conv1x1(x, self.weight, self.bias)


class LayerNormFunction(torch.autograd.Function):
    """nn.LayerNorm(C) over the last dimension of contiguous tokens, forward and backward on libnoisediff_hip (norm_train.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x2 = _tokens(x, x.shape[-1])
        _need_gpu(x2)
        N, C_ = x2.shape
        with _on(x2.device):
            y = torch.empty_like(x2)
            stats = _empty((N, 2), x2.device)
            w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
            L.call("nd_layernorm_train_forward_f32", x2.data_ptr(), C_, w32.data_ptr(), b32.data_ptr(), y.data_ptr(), C_, stats.data_ptr(),
                   N, C_, float(eps), _stream(x2.device))
        ctx.save_for_backward(x2, weight, stats)
        ctx.shape = x.shape
        return y.view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x2, weight, stats = ctx.saved_tensors
        N, C_ = x2.shape
        g2 = _tokens(grad_out, C_)
        with _on(x2.device):
            dx = torch.empty_like(x2)
            dgamma = _empty(C_, x2.device)
            dbeta = _empty(C_, x2.device)
            ws = _workspace("nd_layernorm_train_workspace_floats", x2.device, N, C_)
            w32 = weight.detach().float().contiguous()
            L.call("nd_layernorm_train_backward_f32", g2.data_ptr(), C_, x2.data_ptr(), C_, w32.data_ptr(), stats.data_ptr(), dx.data_ptr(), C_,
                   dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), N, C_, _stream(x2.device))
        return dx.view(ctx.shape), dgamma, dbeta, None


def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """Differentiable F.layer_norm(x, (C,), weight, bias, eps) over the last dimension on the HIP library (a width that nd_layernorm_train_takes: the d = 48
    network's 48 / 96 / 192 / 384 included)."""
    if weight is None or bias is None or not layer_norm_takes(x.shape[-1]) or weight.shape != (x.shape[-1],):
        raise ValueError(f"layer_norm: x {tuple(x.shape)}: needs affine parameters and a width that nd_layernorm_train_takes")
    return LayerNormFunction.apply(x, weight, bias, eps)


# ---- the attention modules (Diffusion_arch.py:84-90, 198-266): cores and RMSNorm forward and backward on the library (attention.hip, linattn.hip,
#      norm.hip, attn_train.hip).  fp32, fixed summation order: a repeated step gives the same bits, and every launch can be captured.
ATTN_DIM_HEAD = 32          # the head width the attention kernels are built for


def _check_qkv(op: str, qkv: torch.Tensor, heads: int) -> None:
    if qkv.dim() != 4 or heads <= 0 or qkv.shape[1] != 3 * heads * ATTN_DIM_HEAD:
        raise ValueError(f"{op}: qkv {tuple(qkv.shape)} is not (B, 3 * {heads} heads * {ATTN_DIM_HEAD}, H, W)")


class AttentionCoreFunction(torch.autograd.Function):
    """softmax(q k^T / sqrt(dh)) v per (sample, head) on to_qkv's output as it stands (Attention.forward with Attend's explicit path: Diffusion_arch.py:255-266,
    models/attend.py:101-116): nd_attention_train_forward_f32 (the sampling path's kernel, plus the log-sum-exp rows) and the flash-style
    nd_attention_backward_f32, whose dqkv has qkv's layout."""

    @staticmethod
    def forward(ctx, qkv, heads):
        qn = _nhwc(qkv)
        _need_gpu(qn)
        B, C3, H, W = qn.shape
        hid, N = C3 // 3, H * W
        with _on(qn.device):
            out = _empty((B, hid, H, W), qn.device, memory_format=torch.channels_last)
            lse = _empty((B, heads, N), qn.device)
            L.call("nd_attention_train_forward_f32", qn.data_ptr(), C3, out.data_ptr(), hid, lse.data_ptr(), B, N, heads, hid // heads, _stream(qn.device))
        ctx.save_for_backward(qn, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qn, out, lse = ctx.saved_tensors
        g = _nhwc(grad_out)
        B, C3, H, W = qn.shape
        hid, N, heads = C3 // 3, H * W, ctx.heads
        with _on(qn.device):
            dqkv = torch.empty_like(qn, memory_format=torch.channels_last)
            ws = _workspace("nd_attention_backward_workspace_floats", qn.device, B, N, heads)
            L.call("nd_attention_backward_f32", qn.data_ptr(), C3, out.data_ptr(), hid, g.data_ptr(), hid, lse.data_ptr(), dqkv.data_ptr(), C3, ws.data_ptr(),
                   B, N, heads, hid // heads, _stream(qn.device))
        return dqkv, None


def attention_core(qkv: torch.Tensor, heads: int = 4) -> torch.Tensor:
    """Differentiable full-attention core on the HIP library: qkv (B, 3 * heads * 32, H, W), q | k | v thirds as ``to_qkv`` emits them, -> (B, heads * 32, H, W);
    channels_last in and out."""
    _check_qkv("attention_core", qkv, heads)
    return AttentionCoreFunction.apply(qkv, heads)


class LinearAttentionCoreFunction(torch.autograd.Function):
    """LinearAttention's core (Diffusion_arch.py:218-235): nd_linear_attention_f32, whose workspace (the key statistics and the per-chunk context
    partials) is the saved state of nd_linear_attention_backward_f32."""

    @staticmethod
    def forward(ctx, qkv, heads):
        qn = _nhwc(qkv)
        _need_gpu(qn)
        B, C3, H, W = qn.shape
        hid, N = C3 // 3, H * W
        with _on(qn.device):
            out = _empty((B, hid, H, W), qn.device, memory_format=torch.channels_last)
            ws = _workspace("nd_linear_attention_workspace_floats", qn.device, B, N, heads)
            L.call("nd_linear_attention_f32", qn.data_ptr(), C3, out.data_ptr(), hid, ws.data_ptr(), B, N, heads, hid // heads, _stream(qn.device))
        ctx.save_for_backward(qn, ws)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qn, fwd_ws = ctx.saved_tensors
        g = _nhwc(grad_out)
        B, C3, H, W = qn.shape
        hid, N, heads = C3 // 3, H * W, ctx.heads
        with _on(qn.device):
            dqkv = torch.empty_like(qn, memory_format=torch.channels_last)
            ws = _workspace("nd_linear_attention_backward_workspace_floats", qn.device, B, N, heads)
            L.call("nd_linear_attention_backward_f32", qn.data_ptr(), C3, g.data_ptr(), hid, fwd_ws.data_ptr(), dqkv.data_ptr(), C3, ws.data_ptr(),
                   B, N, heads, hid // heads, _stream(qn.device))
        return dqkv, None


def linear_attention_core(qkv: torch.Tensor, heads: int = 4) -> torch.Tensor:
    """Differentiable LinearAttention core on the HIP library: the shapes of ``attention_core``."""
    _check_qkv("linear_attention_core", qkv, heads)
    return LinearAttentionCoreFunction.apply(qkv, heads)


class RMSNormFunction(torch.autograd.Function):
    """RMSNorm (Diffusion_arch.py:84-90): F.normalize(x, dim=1) * g * sqrt(C) (+ res, added in the forward kernel) on nd_rmsnorm(_add)_nhwc_f32 and
    nd_rmsnorm_backward_f32; the residual's gradient is the output's."""

    @staticmethod
    def forward(ctx, x, g, res):
        xn = _nhwc(x)
        _need_gpu(xn)
        B, C_, H, W = xn.shape
        g32 = g.detach().float().reshape(-1).contiguous()
        with _on(xn.device):
            y = torch.empty_like(xn, memory_format=torch.channels_last)
            if res is None:
                L.call("nd_rmsnorm_nhwc_f32", xn.data_ptr(), C_, g32.data_ptr(), y.data_ptr(), C_, B, H * W, C_, _stream(xn.device))
            else:
                rn = _nhwc(res)
                L.call("nd_rmsnorm_add_nhwc_f32", xn.data_ptr(), C_, g32.data_ptr(), rn.data_ptr(), C_, y.data_ptr(), C_, B, H * W, C_, _stream(xn.device))
        ctx.save_for_backward(xn, g)
        ctx.has_res = res is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xn, g = ctx.saved_tensors
        gn = _nhwc(grad_out)
        B, C_, H, W = xn.shape
        g32 = g.detach().float().reshape(-1).contiguous()
        with _on(xn.device):
            dx = torch.empty_like(xn, memory_format=torch.channels_last)
            dg = _empty(C_, xn.device)
            ws = _workspace("nd_rmsnorm_backward_workspace_floats", xn.device, B * H * W, C_)
            L.call("nd_rmsnorm_backward_f32", gn.data_ptr(), C_, xn.data_ptr(), C_, g32.data_ptr(), dx.data_ptr(), C_, dg.data_ptr(), ws.data_ptr(),
                   B, H * W, C_, _stream(xn.device))
        return dx, dg.view(g.shape), (grad_out if ctx.has_res else None)


def rms_norm(x: torch.Tensor, g: torch.Tensor, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable RMSNorm over the channels of a 4-D tensor on the HIP library: ``g`` (1, C, 1, 1) as the reference stores it (a width that nd_rmsnorm_train_takes);
    ``res`` (x's shape) is added in the forward kernel."""
    if x.dim() != 4 or not rms_norm_takes(x.shape[1]) or g.numel() != x.shape[1]:
        raise ValueError(f"rms_norm: x {tuple(x.shape)} / g {tuple(g.shape)}: needs a 4-D input, a width that nd_rmsnorm_train_takes and C gains")
    if res is not None and res.shape != x.shape:
        raise ValueError(f"rms_norm: res {tuple(res.shape)} does not match x {tuple(x.shape)}")
    return RMSNormFunction.apply(x, g, res)


def _eligible_layer_norm(m: nn.Module) -> bool:
    return (isinstance(m, nn.LayerNorm) and len(m.normalized_shape) == 1 and m.elementwise_affine and m.bias is not None
            and layer_norm_takes(m.normalized_shape[0]))


def _hip_layer_norm_forward(self: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    return layer_norm(x, self.weight, self.bias, self.eps)


def _eligible_block(m: nn.Module) -> bool:
    """A module shaped like the reference's ``Block`` (Diffusion_arch.py:128-144): children proj (conv), norm (affine GroupNorm), act (SiLU)
    applied in that order with an optional (scale, shift) modulation in between -- recognised by structure, not by import."""
    proj, norm, act = getattr(m, "proj", None), getattr(m, "norm", None), getattr(m, "act", None)
    return (isinstance(proj, nn.Conv2d) and isinstance(norm, nn.GroupNorm) and isinstance(act, nn.SiLU) and _eligible_norm(norm)
            and len(list(m.children())) == 3 and type(m).__name__ == "Block")


def _hip_block_forward(self, x: torch.Tensor, scale_shift=None) -> torch.Tensor:
    """Block.forward with the norm, the per-sample modulation and the activation as one operator (train.group_norm_silu)."""
    x = self.proj(x)
    n = self.norm
    if scale_shift is None:
        return group_norm_silu(x, n.num_groups, n.weight, n.bias, None, n.eps)
    scale, shift = scale_shift
    if scale.numel() == x.shape[0] * x.shape[1] and shift.numel() == scale.numel():              # (B, C, 1, 1): the time embedding's
        return group_norm_silu(x, n.num_groups, n.weight, n.bias, torch.cat((scale.reshape(x.shape[0], -1), shift.reshape(x.shape[0], -1)), 1), n.eps)
    return self.act(self.norm(x) * (scale + 1) + shift)                                           # per-pixel maps (ResnetBlock2): unfused here; trainable.py fuses them (modulate_silu)


def _eligible(m: nn.Module) -> bool:
    return (isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
            and m.groups == 1 and m.padding_mode == "zeros" and conv3x3_trains(m.in_channels, m.out_channels))


def _hip_conv_forward(self: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    return conv3x3(x, self.weight, self.bias)


def accelerate(model: nn.Module, norms: bool = True, linears: bool = True) -> int:
    """Route every eligible 3x3 convolution of ``model`` (stride 1, padding 1, channel counts multiples of 8) and -- unless
    ``norms=False`` / ``linears=False`` -- every affine nn.GroupNorm (C a multiple of 4) and nn.LayerNorm (C = 64, 128, 256 k) and the weight / bias gradient of every
    nn.Linear and 1x1 nn.Conv2d (channel counts multiples of 4) through the HIP library, forward and backward; modules shaped like the
    reference's ``Block`` (proj / norm / act) get their norm + modulation + SiLU tail as one operator.  Parameters,
    module tree and state dict are untouched.  The replacement is made on the module's CLASS (a cached subclass of its own type
    whose ``forward`` is the HIP version), not as an instance attribute: ``copy.deepcopy`` (the trainer's EMA) and
    ``nn.DataParallel`` replicas (``define_G`` wraps the net, models/modules.py:81; a replica copies ``__dict__``, so an instance-bound
    method would keep running on the ORIGINAL module's cuda:0 parameters) resolve ``forward`` through their own ``self``.
    Returns the number of convolutions taken."""
    n = 0
    for m in model.modules():
        if _eligible(m) and getattr(m.forward, "__func__", None) is not _hip_conv_forward:
            _retarget(m, _hip_conv_forward)
            n += 1
        elif norms and _eligible_norm(m) and getattr(m.forward, "__func__", None) is not _hip_norm_forward:
            _retarget(m, _hip_norm_forward)
        elif norms and _eligible_layer_norm(m) and getattr(m.forward, "__func__", None) is not _hip_layer_norm_forward:
            _retarget(m, _hip_layer_norm_forward)
        elif linears and _eligible_linear(m) and getattr(m.forward, "__func__", None) is not _hip_linear_forward:
            _retarget(m, _hip_linear_forward)
        elif norms and _eligible_block(m) and getattr(m.forward, "__func__", None) is not _hip_block_forward:
            _retarget(m, _hip_block_forward)
    return n


_RETARGETED: Dict[tuple, type] = {}


def _rebuild_retargeted(base: type, fn_name: str, state):
    """pickle support (torch.save(model), mp.spawn arguments): the dynamic subclass is not importable by name, so an accelerated
    module is pickled as (its base class, the name of the HIP forward) and re-targeted when it is loaded."""
    m = base.__new__(base)
    m.__dict__.update(state)
    _retarget(m, globals()[fn_name])
    return m


def _reduce_retargeted(self):
    return _rebuild_retargeted, (type(self)._nd_accelerated_base, type(self).forward.__name__, self.__dict__.copy())


def _retarget(m: nn.Module, fn) -> None:
    """m.__class__ <- the cached subclass of type(m) whose forward is ``fn`` (same name / module / qualname, so structural
    checks by class name and ``isinstance`` keep working)."""
    base = getattr(type(m), "_nd_accelerated_base", type(m))
    cls = _RETARGETED.get((base, fn))
    if cls is None:
        cls = type(base.__name__, (base,), {"forward": fn, "__module__": base.__module__, "__qualname__": base.__qualname__,
                                             "__doc__": base.__doc__, "_nd_accelerated_base": base, "__reduce__": _reduce_retargeted})
        _RETARGETED[(base, fn)] = cls
    m.__dict__.pop("forward", None)          # an instance attribute (older accelerate(), user patches) would shadow the class
    m.__class__ = cls


class Adam(torch.optim.Adam):
    """``torch.optim.Adam`` (the reference's optimizer: models/trainer_diffusion.py:94, models/denoising_diffusion_pytorch.py:22) whose ``step`` updates
    all parameters of a group in ONE launch of nd_adam_step_f32 (adam.hip) instead of PyTorch's ~10 foreach passes: 1.14 -> 0.3 ms of the d = 64
    network's 28 ms step.  Same constructor, same state (``step`` -- a CPU tensor per parameter --, ``exp_avg``, ``exp_avg_sq``), so state dicts move
    between the two classes (``--resume_optim``); the same update in fp32 up to the rounding of one fused pass.  What the kernel does not do is refused:
    amsgrad, maximize, differentiable, sparse gradients, parameters that are not fp32 on a GPU.  ``capturable=True`` (PyTorch's flag): the step counters live on
    the device and nothing is computed on the host per step (nd_adam_step_capturable_f32) -- the form a training step captured as ONE CUDA graph needs
    (tools/train_graph_bench.py); run one step before the capture.  With ``capturable=True`` the group's ``lr`` may be a one-element fp32 tensor on the
    parameters' device (PyTorch's tensor lr, which its schedulers ``fill_`` in place): the kernel reads it there (nd_adam_step_capturable_lr_f32), so a
    captured step follows ``set_lr`` / a scheduler without a new capture."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **kw):
        for k in ("amsgrad", "maximize", "differentiable", "fused"):
            if kw.get(k):
                raise NotImplementedError(f"noisediff_amd.train.Adam: {k}=True is not built (use torch.optim.Adam)")
        kw.pop("foreach", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, **{k: v for k, v in kw.items() if k != "fused"})
        self._nd_init_caches()

    def _nd_init_caches(self) -> None:
        """Everything the instance keeps besides torch.optim.Adam's own defaults / state / param_groups."""
        self._nd_tables: Dict[tuple, tuple] = {}     # (group index, capturable, parameter data_ptrs) -> the group's laid-out table (_nd_table)
        self._nd_captured_lr: Dict[int, object] = {} # id(group) -> the learning rate its captured step was recorded with: a float, or THE tensor it reads
        self._nd_captured: list = []                 # tables of captured steps: a replay reads them, so they live as long as the optimizer
        self._nd_keep = None                         # tables of the last step: alive until the next one (the launch is asynchronous)

    def __setstate__(self, state) -> None:
        """torch.optim.Optimizer.__getstate__ keeps only defaults / state / param_groups: a deep copy or an unpickled optimizer arrives here without the
        caches (load_state_dict comes through here too, with them: its tables are checked against the new state tensors in _nd_table)."""
        super().__setstate__(state)
        if "_nd_tables" not in self.__dict__:
            self._nd_init_caches()

    def check_captured_lr(self) -> None:
        """Call before replaying a captured training step: a captured ``capturable=True`` step carries the learning rate it was captured with (a launch
        argument).  Raises if a scheduler or the caller has changed ``group['lr']`` since -- re-capture the step then.  A step captured with
        a tensor lr reads that tensor at every replay: it passes whatever the value, while the group still holds that same tensor."""
        for group in self.param_groups:
            lr0, now = self._nd_captured_lr.get(id(group)), group["lr"]
            if lr0 is None:
                continue
            if isinstance(lr0, torch.Tensor):
                if now is not lr0:
                    raise RuntimeError("noisediff_amd.train.Adam: the captured step reads its learning rate from the tensor the group held at the capture; "
                                       "group['lr'] has been replaced since and a replay would ignore it: use set_lr() (fill_ in place), or capture the step again")
            elif isinstance(now, torch.Tensor) or float(now) != lr0:
                raise RuntimeError(f"noisediff_amd.train.Adam: the captured step was recorded with lr={lr0:g}, the group now has lr={float(now):g}: "
                                   "a replay would ignore the change; capture the step again")

    def set_lr(self, value, group: int = 0) -> None:
        """``param_groups[group]['lr'] = value`` (the reference's hand-written schedule, models/trainer_denoising.py:185-188) in the form a captured step
        follows: ``fill_`` on a tensor lr, plain assignment otherwise."""
        g = self.param_groups[group]
        if isinstance(g["lr"], torch.Tensor):
            g["lr"].fill_(float(value))
        else:
            g["lr"] = value

    def _nd_table(self, gi: int, group: dict, ps: list, capturing: bool) -> tuple:
        """Validate group ``gi``'s parameters ``ps`` (those with a gradient) and lay out what does not change from step to step: (nd_adam_item records
        without the gradient pointers and step sizes, chunk table on the device, number of chunks, exp_avg, exp_avg_sq and step tensors).  Checked and
        laid out once per set of parameters (the host side of a step is ~1 ms this way, 4.4 per parameter)."""
        dev = ps[0].device
        cap = bool(group.get("capturable"))                              # step counters on the device, nothing computed on the host (nd_adam_step_capturable_f32)
        key = (gi, cap, tuple(p.data_ptr() for p in ps))
        ent = self._nd_tables.get(key)
        if ent is not None:
            # load_state_dict (or anything else) replaced the state tensors: lay the table out again (compared by object, not by id() of a dict that
            # may have been freed and its id reused)
            _, _, _, ms0, vs0, steps0, _ = ent
            for p, m0, v0, t0 in zip(ps, ms0, vs0, steps0):
                st = self.state[p]
                if st.get("exp_avg") is not m0 or st.get("exp_avg_sq") is not v0 or st.get("step") is not t0:
                    ent = None
                    break
        if ent is not None:
            return ent
        if capturing:
            raise RuntimeError("noisediff_amd.train.Adam: run a step with the same parameters before the capture (state and tables are built on the first step)")
        if len(self._nd_tables) > 64:
            self._nd_tables.clear()
        for p in ps:
            if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda or p.device != dev or not p.is_contiguous():
                raise NotImplementedError("noisediff_amd.train.Adam updates dense, contiguous fp32 parameters of one GPU per group")
            st = self.state[p]
            if len(st) == 0:                                             # torch.optim.Adam._init_group's state
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if cap else torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous()) or m.device != dev or v.device != dev:
                raise NotImplementedError("noisediff_amd.train.Adam: optimizer state must be contiguous and on the parameter's device")
            if cap and not (st["step"].is_cuda and st["step"].dtype == torch.float32):
                raise NotImplementedError("noisediff_amd.train.Adam(capturable=True): the step counters must be fp32 tensors on the parameter's device")
            if not cap and st["step"].is_cuda:
                raise NotImplementedError("noisediff_amd.train.Adam: step counters on the device need capturable=True")
        items = np.zeros(len(ps), dtype=np.dtype(L.AdamItem))            # nd_adam_item
        ms, vs, steps = [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps], [self.state[p]["step"] for p in ps]
        items["p"] = [p.data_ptr() for p in ps]
        items["m"] = [t.data_ptr() for t in ms]
        items["v"] = [t.data_ptr() for t in vs]
        items["n"] = [p.numel() for p in ps]
        if cap:
            items["step"] = [t.data_ptr() for t in steps]
        per = int(L.load().nd_adam_chunk_elements())
        pairs = [(i, c) for i, p in enumerate(ps) for c in range((p.numel() + per - 1) // per)]
        chunks = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev)
        # a capturable group keeps one pinned staging buffer for its first capture: pinned memory cannot be allocated while a stream captures, and the
        # host allocator has a free block then only by luck (it hands a block back after a LATER allocation has seen its copy finished)
        spare = [torch.empty(items.nbytes, dtype=torch.uint8).pin_memory()] if cap else []
        ent = self._nd_tables[key] = (items, chunks, len(pairs), ms, vs, steps, spare)
        return ent

    def _nd_launch(self, group: dict, ps: list, ent: tuple, capturing: bool) -> None:
        """One launch for group's parameters ``ps`` over its table ``ent`` (_nd_table) with this step's gradient pointers and step sizes."""
        dev, cap = ps[0].device, bool(group.get("capturable"))
        beta1, beta2 = group["betas"]
        lr_dev = group["lr"] if cap and isinstance(group["lr"], torch.Tensor) else None
        if lr_dev is not None:
            if lr_dev.numel() != 1 or lr_dev.dtype != torch.float32 or lr_dev.device != dev:
                raise NotImplementedError("noisediff_amd.train.Adam(capturable=True): a tensor lr must be one fp32 element on the parameters' device")
        else:
            lr = float(group["lr"])                                      # (capturable=False reads a tensor lr on the host, as torch does)
        if cap and capturing:
            # a float learning rate is a launch argument: a captured step replays with the value it was captured with (the reference's CosineAnnealingLR
            # and its hand-written group['lr'] = ..., trainer_diffusion.py:95,104-105, do not reach a replayed graph) -- refuse a silent mismatch.  A
            # tensor lr is read by the kernel at every replay: what must not change is WHICH tensor the group holds.
            self._nd_captured_lr[id(group)] = lr if lr_dev is None else lr_dev
        items, chunks, n_chunks, ms, vs, steps, spare = ent
        gs = [p.grad for p in ps]
        if not all(g.is_contiguous() and g.dtype == torch.float32 and not g.is_sparse for g in gs):
            gs = [g.contiguous() if not g.is_sparse and g.dtype == torch.float32 else None for g in gs]
            if any(g is None for g in gs):
                raise NotImplementedError("noisediff_amd.train.Adam updates from dense fp32 gradients")
        items = items.copy()
        items["g"] = [g.data_ptr() for g in gs]
        items["vec4"] = ((items["p"] | items["g"] | items["m"] | items["v"]) & 15) == 0
        if not cap:
            torch._foreach_add_(steps, 1.0)                              # (CPU scalars: one C++ loop)
            # every parameter's OWN step count (a cheap loop over CPU scalars): parameters that were stepped under another set -- grad None on some
            # steps -- carry different counts, and each gets its own bias correction
            ts = np.array([float(t) for t in steps], dtype=np.float64)
            items["step_size"] = lr / (1.0 - beta1 ** ts)
            items["bias2_sqrt"] = np.sqrt(1.0 - beta2 ** ts)
        # pointers and step sizes of this step (a few KB): pinned + asynchronous, so the host keeps running ahead of the device
        if capturing and spare:
            host_table = spare.pop()
            host_table.copy_(torch.from_numpy(items.view(np.uint8)))
        else:
            host_table = torch.from_numpy(items.view(np.uint8)).pin_memory()
        table = host_table.to(dev, non_blocking=True)
        with _on(dev):
            if lr_dev is not None:
                L.call("nd_adam_step_capturable_lr_f32", table.data_ptr(), len(ps), chunks.data_ptr(), n_chunks, lr_dev.data_ptr(), float(beta1), float(beta2),
                       float(group["eps"]), float(group["weight_decay"]), _stream(dev))
            elif cap:
                L.call("nd_adam_step_capturable_f32", table.data_ptr(), len(ps), chunks.data_ptr(), n_chunks, lr, float(beta1), float(beta2),
                       float(group["eps"]), float(group["weight_decay"]), _stream(dev))
            else:
                L.call("nd_adam_step_f32", table.data_ptr(), len(ps), chunks.data_ptr(), n_chunks, float(beta1), float(beta2), float(group["eps"]),
                       float(group["weight_decay"]), _stream(dev))
        if capturing:                                                    # a captured step replays with these tables: they live as long as the optimizer
            self._nd_captured.append((table, host_table, gs, lr_dev))
        self._nd_keep = (table, gs)
        # the kernel wrote through raw pointers: tell autograd (and the packing caches, which compare version counters) that these tensors changed
        torch.autograd.graph.increment_version(ps)
        torch.autograd.graph.increment_version(ms)
        torch.autograd.graph.increment_version(vs)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if capturing and not all(g.get("capturable") for g in self.param_groups):
            raise RuntimeError("noisediff_amd.train.Adam computes its step sizes on the host unless built with capturable=True: this step cannot be captured "
                               "into a CUDA graph")
        L.load()
        # EVERY group's table is validated before ANY group is launched (a rebuild in the middle used to re-run the whole step and move the
        # groups already updated twice)
        work = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if ps:
                work.append((group, ps, self._nd_table(gi, group, ps, capturing)))
        for group, ps, ent in work:
            self._nd_launch(group, ps, ent, capturing)
        return loss


# ---------------------------------------------------------------------------------------------------------------- the shadow model of a training run
EMA_SKIP, EMA_COPY, EMA_LERP, EMA_COPY_LERP = 0, 1, 2, 3          # the `action` of an update's plan (ema.hip)


def ema_plan(s: int, initted: bool, beta: float, update_after_step: int, update_every: int, inv_gamma: float = 1.0, power: float = 2.0 / 3.0,
             min_value: float = 0.0) -> tuple:
    """What the ``update()`` call that finds the step counter at ``s`` does: ``(action, weight)`` -- ema_pytorch's rule as ema.hip's plan kernel computes
    it, here on the host (the CPU path of ``EMA`` and the tests): fp64 arithmetic, the weight ``1 - decay`` rounded to fp32 once.  EMA_COPY_LERP sets
    ``initted``; the counter becomes ``s + 1`` in every case."""
    if s % update_every != 0:
        return EMA_SKIP, 0.0
    if s <= update_after_step:
        return EMA_COPY, 0.0
    e = max(s + 1 - update_after_step - 1, 0)                         # (the package reads the counter after its increment)
    decay = 0.0 if e <= 0 else min(max(1.0 - (1.0 + e / inv_gamma) ** -power, min_value), beta)
    return (EMA_LERP if initted else EMA_COPY_LERP), float(np.float32(1.0 - decay))


class EMA(nn.Module):
    """``ema_pytorch.EMA`` as the reference uses it (models/trainer_diffusion.py:63-69,191; ``ema_model`` is what ``save_networks('ema', ...)`` ships):
    ``.ema_model`` (a deep copy of ``model``, ``requires_grad_(False)``), ``.online_model``, ``.update()``, ``.to()``, ``forward`` -> ``ema_model``,
    ``copy_params_from_model_to_ema()``, ``get_current_decay()``, buffers ``step`` (int64[1]) and ``initted`` (bool[1]); state-dict keys ``initted``,
    ``step``, ``online_model.*``, ``ema_model.*``.  Keywords of the package that are not in the signature raise NotImplementedError.

    ``update()`` on GPU tensors is ONE call of nd_ema_update_f32 (ema.hip) over all fp32 parameters and fp32 buffers, matched by name: the step
    counter, the warm-up flag and the decision (skip / copy / lerp and its weight) live in device memory, so there is no host read -- the package's
    ``self.step.item()`` is a sync per training step -- and the call can be captured into the training step's graph: run one ``update()`` before the
    capture (the tables are laid out then; captured tables live as long as the object).  Non-floating tensors are left alone, as the package leaves
    them; fp16 / bf16 (anything floating but fp32), non-contiguous tensors and tensors on more than one device raise NotImplementedError.  CPU modules
    run the same schedule with ``copy_`` / ``lerp_``.  The decay is computed in fp64 (the package: fp32 tensor arithmetic).

    Every eager ``update()`` on GPU tensors bumps the version counters of the shadow tensors, so the next forward of ``ema_model`` repacks its weights
    without ``invalidate_packs()``.  REPLAYS of a captured graph bump nothing -- the rule of ``_PackCache``'s docstring holds unchanged: packings made
    while capturing are repacked on every eager use; after replays, call ``train.invalidate_packs()`` before an eager forward of ``ema_model`` whose
    packings were made eagerly.

    ``last_plan()`` -> (action, weight) of the last call and ``get_current_decay()`` read the device: for tests and logs."""

    def __init__(self, model: nn.Module, ema_model: Optional[nn.Module] = None, beta: float = 0.9999, update_after_step: int = 100, update_every: int = 10,
                 inv_gamma: float = 1.0, power: float = 2.0 / 3.0, min_value: float = 0.0, param_or_buffer_names_no_ema=(), **kw):
        for k in kw:
            raise NotImplementedError(f"noisediff_amd.train.EMA: {k} is not built (use ema_pytorch.EMA)")
        if not (0.0 <= beta <= 1.0) or update_every < 1 or not inv_gamma > 0.0:
            raise ValueError(f"noisediff_amd.train.EMA: beta={beta} must lie in [0, 1], update_every={update_every} must be at least 1, inv_gamma={inv_gamma} positive")
        super().__init__()
        import copy
        self.online_model = model
        self.ema_model = copy.deepcopy(model) if ema_model is None else ema_model
        self.ema_model.requires_grad_(False)
        self.beta, self.update_after_step, self.update_every = float(beta), int(update_after_step), int(update_every)
        self.inv_gamma, self.power, self.min_value = float(inv_gamma), float(power), float(min_value)
        self.param_or_buffer_names_no_ema = set(param_or_buffer_names_no_ema)
        self.register_buffer("initted", torch.tensor([False]))
        self.register_buffer("step", torch.tensor([0], dtype=torch.int64))
        self._nd_init_caches()

    def _nd_init_caches(self) -> None:
        self._nd_tables: Dict[tuple, tuple] = {}     # data_ptrs of the (shadow, online) pairs -> the laid-out tables (_nd_table)
        self._nd_captured: list = []                 # tables of captured updates: a replay reads them, so they live as long as the object
        self._nd_last = None                         # (action, weight) of the last update on the CPU, or the device plan record of the last one on a GPU
        self._nd_kept = None                         # (pairs, holders) of the last walk over both module trees (_nd_pairs)

    def __getstate__(self):
        """Deep copies and pickles carry their own counters (the buffers) and none of the tables, which hold the original's addresses."""
        return {k: v for k, v in self.__dict__.items() if not k.startswith("_nd_")}

    def __setstate__(self, state) -> None:
        super().__setstate__(state)
        self._nd_init_caches()

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)

    @staticmethod
    def _nd_holders(model: nn.Module) -> dict:
        """name -> (the module's own ``_parameters`` / ``_buffers`` dict, key, tensor) for every parameter and buffer, each tensor once (as
        ``named_parameters`` / ``named_buffers`` name them)."""
        out, seen = {}, set()
        for prefix, mod in model.named_modules():
            for store in (mod._parameters, mod._buffers):
                for k, t in store.items():
                    if t is not None and id(t) not in seen:
                        seen.add(id(t))
                        out[(prefix + "." if prefix else "") + k] = (store, k, t)
        return out

    def _nd_pairs(self) -> list:
        """(name, shadow tensor, online tensor) of every floating parameter and buffer, matched by name.  Walking both module trees costs more than
        the whole pass, so the list is kept and only checked per call: every tensor must still be the one its module holds (``.to()`` replaces
        buffers, an assignment replaces a parameter); modules ADDED after the first update() are seen after ``copy_params_from_model_to_ema()``,
        ``load_state_dict()`` or ``.to()``, which read the trees again."""
        kept = self._nd_kept
        if kept is not None and all(store.get(k) is t for store, k, t in kept[1]):
            return kept[0]
        src = self._nd_holders(self.online_model)
        pairs, holders = [], []
        for name, (store, k, e) in self._nd_holders(self.ema_model).items():
            if name not in src:
                raise RuntimeError(f"noisediff_amd.train.EMA: the online model has no tensor named {name}")
            if e.is_floating_point() or e.is_complex():
                pairs.append((name, e, src[name][2]))
                holders += [(store, k, e), src[name]]
        self._nd_kept = (pairs, holders)
        return pairs

    def _apply(self, fn, *args, **kwargs):
        self._nd_kept = None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._nd_kept = None
        return super().load_state_dict(*args, **kwargs)

    def _nd_check(self, pairs: list) -> torch.device:
        """The one device of the pairs and the two counters; refuses what the pass does not do."""
        devices = {self.step.device, self.initted.device}
        for name, e, s in pairs:
            if e.dtype != torch.float32 or s.dtype != torch.float32:
                raise NotImplementedError(f"noisediff_amd.train.EMA averages fp32 tensors: {name} is {e.dtype} / {s.dtype}")
            if e.shape != s.shape or not e.is_contiguous() or not s.is_contiguous():
                raise NotImplementedError(f"noisediff_amd.train.EMA: {name} must be contiguous and of one shape in both models")
            devices |= {e.device, s.device}
        if len(devices) != 1:
            raise NotImplementedError(f"noisediff_amd.train.EMA: both models and the counters must be on one device (call .to(device)), found {sorted(map(str, devices))}")
        if self.step.dtype != torch.int64 or self.initted.dtype != torch.bool or self.step.numel() != 1 or self.initted.numel() != 1:
            raise NotImplementedError("noisediff_amd.train.EMA: step must be one int64 and initted one bool")
        return devices.pop()

    def _nd_table(self, pairs: list, dev: torch.device, capturing: bool) -> tuple:
        """Laid out once per set of tensors (keyed on their addresses): (nd_ema_item table and chunk table on the device, number of items and chunks,
        the plan record, the shadow tensors, the online tensors -- held so that the addresses stay theirs)."""
        key = (self.step.data_ptr(), self.initted.data_ptr()) + tuple(t.data_ptr() for _, e, s in pairs for t in (e, s))
        ent = self._nd_tables.get(key)
        if ent is not None:
            return ent
        if capturing:
            raise RuntimeError("noisediff_amd.train.EMA: run update() once with the same tensors before the capture (the tables are laid out on the first call)")
        self._nd_check(pairs)
        if len(self._nd_tables) > 16:
            self._nd_tables.clear()
        items = np.zeros(len(pairs), dtype=np.dtype(L.EmaItem))          # nd_ema_item
        items["ema"] = [e.data_ptr() for _, e, _ in pairs]
        items["src"] = [s.data_ptr() for _, _, s in pairs]
        items["n"] = [e.numel() for _, e, _ in pairs]
        items["vec4"] = ((items["ema"] | items["src"]) & 15) == 0
        items["no_ema"] = [name in self.param_or_buffer_names_no_ema for name, _, _ in pairs]
        per = int(L.load().nd_ema_chunk_elements())
        chunk_pairs = [(i, c) for i, (_, e, _) in enumerate(pairs) for c in range((e.numel() + per - 1) // per)]
        # the addresses do not change from call to call (Adam's gradient pointers do): both tables are uploaded here, once (synchronous copies of a
        # few KB), and a captured update copies nothing -- no staging memory is needed while a stream captures
        table = torch.from_numpy(items.view(np.uint8)).to(dev)
        chunks = torch.tensor(chunk_pairs, dtype=torch.int32).reshape(-1, 2).to(dev)
        plan = torch.zeros(2, dtype=torch.int32, device=dev)             # {int32 action; float weight}
        ent = self._nd_tables[key] = (table, chunks, len(pairs), len(chunk_pairs), plan, [e for _, e, _ in pairs], [s for _, _, s in pairs])
        return ent

    @torch.no_grad()
    def update(self) -> None:
        pairs = self._nd_pairs()
        if not pairs:
            self.step += 1
            return
        if not pairs[0][1].is_cuda:
            return self._update_cpu(pairs)
        capturing = torch.cuda.is_current_stream_capturing()
        dev = pairs[0][1].device
        table, chunks, n_items, n_chunks, plan, emas, _ = ent = self._nd_table(pairs, dev, capturing)
        with _on(dev):
            L.call("nd_ema_update_f32", table.data_ptr(), n_items, chunks.data_ptr(), n_chunks, self.step.data_ptr(), self.initted.data_ptr(), plan.data_ptr(),
                   self.beta, self.update_after_step, self.update_every, self.inv_gamma, self.power, self.min_value, _stream(dev))
        if capturing:
            self._nd_captured.append(ent)
        self._nd_last = plan
        # the kernel wrote through raw pointers: tell autograd and the packing caches (which compare version counters) that the shadow changed
        torch.autograd.graph.increment_version(emas)
        torch.autograd.graph.increment_version([self.step, self.initted])

    def _update_cpu(self, pairs: list) -> None:
        """The same schedule on CPU modules: the plan on the host, ``copy_`` / ``lerp_`` per tensor."""
        if self._nd_check(pairs).type != "cpu":
            raise NotImplementedError("noisediff_amd.train.EMA: both models and the counters must be on one device")
        action, weight = ema_plan(int(self.step), bool(self.initted), self.beta, self.update_after_step, self.update_every, self.inv_gamma, self.power,
                                  self.min_value)
        self.step += 1
        self._nd_last = (action, weight)
        if action == EMA_SKIP:
            return
        if action == EMA_COPY_LERP:
            self.initted.fill_(True)
        for name, e, s in pairs:
            if action != EMA_LERP or name in self.param_or_buffer_names_no_ema:
                e.copy_(s)
            if action != EMA_COPY and name not in self.param_or_buffer_names_no_ema:
                e.lerp_(s, weight)

    @torch.no_grad()
    def copy_params_from_model_to_ema(self) -> None:
        self._nd_kept = None
        for _, e, s in self._nd_pairs():
            e.copy_(s)

    def get_current_decay(self) -> float:
        """The decay the next averaging call would use (the package's method: it reads ``step``, on a GPU a sync -- for logging only)."""
        e = max(int(self.step) - self.update_after_step - 1, 0)
        return 0.0 if e <= 0 else min(max(1.0 - (1.0 + e / self.inv_gamma) ** -self.power, self.min_value), self.beta)

    def last_plan(self) -> tuple:
        """(action, weight) of the last ``update()``: EMA_SKIP / EMA_COPY / EMA_LERP / EMA_COPY_LERP and the lerp weight ``1 - decay`` (0 where nothing
        is averaged).  On a GPU this reads the device's plan record: for tests and logs."""
        if self._nd_last is None:
            raise RuntimeError("noisediff_amd.train.EMA.last_plan: no update() yet")
        if isinstance(self._nd_last, tuple):
            return self._nd_last
        rec = self._nd_last.cpu()
        return int(rec[0]), float(rec[1:].view(torch.float32)[0])


# ---------------------------------------------------------------------------------------------------------------- the two ends of a diffusion training step
def _check_ends(op: str, x: torch.Tensor, what: str) -> None:
    _need_gpu(x)
    if x.dim() != 4 or x.shape[1] % 4 != 0 or x.dtype != torch.float32:
        raise ValueError(f"{op}: {what} {tuple(x.shape)} {x.dtype}: needs a 4-D fp32 tensor whose channel count is a multiple of 4 (there is no fallback)")


def diffusion_noising(x0: torch.Tensor, sqrt_alphas_cumprod: torch.Tensor, sqrt_one_minus_alphas_cumprod: torch.Tensor, *, objective: str,
                      auto_normalize: bool = False, offset_strength: float = 0.0, seed: int = 0, first_sample: int = 0, draw: int = 0,
                      rng: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                      offset: Optional[torch.Tensor] = None, return_draws: bool = False):
    """``GaussianDiffusion.forward``'s timestep draw, ``normalize``, the offset noise, ``q_sample`` and the objective's target in ONE launch
    (nd_diffusion_noising_f32): ``(t, x_t, target)``, the two images (B, C, H, W) in channels_last memory; with ``return_draws`` also the element noise
    (before the offset is added) and the offset (B, C), so that a step can be replayed with explicit draws.  ``x0``: fp32, NCHW-contiguous or channels_last
    (read as it lies), C % 4 == 0.  ``t`` / ``noise`` / ``offset`` given: used as they are -- the outputs are then bit for bit the reference's.  Otherwise
    they come from the counter-based Philox stream keyed (seed, first_sample + row, draw): ``rng`` (int64[3] on the device: seed, first_sample, draw)
    overrides the three scalars, so a captured graph draws anew on every replay.  Nothing here is differentiable: the outputs carry no gradient."""
    _check_ends("diffusion_noising", x0, "x0")
    B, C_, H, W = x0.shape
    dev = x0.device
    x0 = x0.detach()
    if x0.is_contiguous():
        last = 0
    else:
        x0, last = x0.contiguous(memory_format=torch.channels_last), 1
    tabs = [sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod]
    if any(s.dtype != torch.float32 or s.device != dev or s.dim() != 1 or s.numel() != tabs[0].numel() for s in tabs):
        raise ValueError("diffusion_noising: the two schedule tables must be fp32 vectors of one length on x0's device")
    tabs = [s.detach().contiguous() for s in tabs]
    p = L.DiffusionNoising()
    keep = [x0] + tabs
    if noise is not None:
        if noise.shape != x0.shape:
            raise ValueError(f"diffusion_noising: noise {tuple(noise.shape)} does not match x0 {tuple(x0.shape)}")
        keep.append(_nhwc(noise.detach().to(dev)))
        p.noise = keep[-1].data_ptr()
    if offset is not None:
        if tuple(offset.shape) != (B, C_):
            raise ValueError(f"diffusion_noising: offset {tuple(offset.shape)} must be {(B, C_)}")
        keep.append(offset.detach().to(dev, torch.float32).contiguous())
        p.offset = keep[-1].data_ptr()
    if t is not None:
        if tuple(t.shape) != (B,):
            raise ValueError(f"diffusion_noising: t {tuple(t.shape)} must be {(B,)}")
        keep.append(t.detach().to(dev, torch.int64).contiguous())
        p.t_in = keep[-1].data_ptr()
    if rng is not None:
        if rng.dtype != torch.int64 or rng.device != dev or rng.numel() != 3 or not rng.is_contiguous():
            raise ValueError("diffusion_noising: rng must be a contiguous int64[3] tensor {seed, first_sample, draw} on x0's device")
        p.rng = rng.data_ptr()
    with _on(dev), torch.no_grad():
        t_out = torch.empty(B, dtype=torch.int64, device=dev)
        x_t = torch.empty((B, C_, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        target = torch.empty_like(x_t, memory_format=torch.channels_last)
        noise_out = torch.empty_like(x_t, memory_format=torch.channels_last) if return_draws else None
        offset_out = _empty((B, C_), dev) if return_draws else None
        p.x0, p.sqrt_alphas_cumprod, p.sqrt_one_minus_alphas_cumprod = x0.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr()
        p.t_out, p.x_t, p.target, p.noise_out, p.offset_out = t_out.data_ptr(), x_t.data_ptr(), target.data_ptr(), L.ptr(noise_out), L.ptr(offset_out)
        p.seed, p.first_sample, p.draw, p.offset_strength = int(seed) & (2 ** 64 - 1), int(first_sample), int(draw), float(offset_strength)
        p.B, p.C, p.H, p.W, p.T = B, C_, H, W, tabs[0].numel()
        p.objective, p.auto_normalize, p.x0_channels_last = L.OBJECTIVES[objective], int(bool(auto_normalize)), last
        L.call("nd_diffusion_noising_f32", C.byref(p), _stream(dev))
    return (t_out, x_t, target, noise_out, offset_out) if return_draws else (t_out, x_t, target)


class DiffusionLossFunction(torch.autograd.Function):
    """``p_losses``' tail (:514-528): mean_b(mean_elems((out - target)^2) loss_weight[t_b]) [+ the mean-intensity term of pred_x0] on nd_diffusion_loss_f32
    (fp64 sums in a fixed order) and nd_diffusion_loss_backward_f32 (one pass, the upstream gradient read on the device).  The workspace -- the slices'
    partials and the signs the backward reads -- is a saved tensor allocated here, so a captured graph owns it."""

    @staticmethod
    def forward(ctx, model_out, target, t, loss_weight, x0_term):
        mo, tg = _nhwc(model_out), _nhwc(target)
        B, C_, H, W = mo.shape
        dev = mo.device
        t64, lw = t.to(dev, torch.int64).contiguous(), loss_weight.detach().to(dev, torch.float32).contiguous()
        with _on(dev):
            ws = torch.empty(int(L.call("nd_diffusion_loss_workspace_bytes", B, C_, H * W)), dtype=torch.uint8, device=dev)
            loss = _empty((), dev)
            L.call("nd_diffusion_loss_f32", mo.data_ptr(), tg.data_ptr(), t64.data_ptr(), lw.data_ptr(), B, C_, H * W, lw.numel(), int(x0_term),
                   ws.data_ptr(), loss.data_ptr(), None, _stream(dev))
        ctx.save_for_backward(mo, tg, t64, lw, ws)
        ctx.x0_term = int(x0_term)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        mo, tg, t64, lw, ws = ctx.saved_tensors
        B, C_, H, W = mo.shape
        dev = mo.device
        g = grad_loss.to(dev, torch.float32).reshape(1).contiguous()
        with _on(dev):
            grad = torch.empty_like(mo, memory_format=torch.channels_last)
            L.call("nd_diffusion_loss_backward_f32", mo.data_ptr(), tg.data_ptr(), t64.data_ptr(), lw.data_ptr(), g.data_ptr(), ws.data_ptr(), grad.data_ptr(),
                   B, C_, H * W, lw.numel(), ctx.x0_term, _stream(dev))
        return grad, None, None, None, None


def diffusion_loss(model_out: torch.Tensor, target: torch.Tensor, t: torch.Tensor, loss_weight: torch.Tensor, x0_term: bool = False) -> torch.Tensor:
    """The diffusion training loss of a batch on the HIP library, differentiable in ``model_out`` only: a ``target`` that requires grad, a CPU tensor, a
    dtype other than fp32 or a channel count that is no multiple of 4 raises (with ``x0_term``: C a power of two up to 256)."""
    _check_ends("diffusion_loss", model_out, "model_out")
    _check_ends("diffusion_loss", target, "target")
    if target.shape != model_out.shape or tuple(t.shape) != (model_out.shape[0],):
        raise ValueError(f"diffusion_loss: model_out {tuple(model_out.shape)}, target {tuple(target.shape)}, t {tuple(t.shape)} do not belong together")
    if target.requires_grad:
        raise ValueError("diffusion_loss: no gradient is produced for target; detach it")
    return DiffusionLossFunction.apply(model_out, target, t, loss_weight, bool(x0_term))


# ---------------------------------------------------------------------------------------------------------------- the end of a denoiser training step
def _check_lambdas(op: str, l1: float, mse: float) -> None:
    if not (0.0 <= l1 < float("inf") and 0.0 <= mse < float("inf")) or (l1 == 0.0 and mse == 0.0):
        raise ValueError(f"{op}: l1={l1} and mse={mse} must be finite, not negative and not both zero")


def _denoise_loss_launch(out: torch.Tensor, layout: int, target: torch.Tensor, l1: float, mse: float):
    """nd_denoise_loss_f32 on ``out`` ((B, C, H, W) for LAYOUT_NCHW, (B, H, W, 4) for LAYOUT_NHWC) against the NCHW ``target``: (terms [3], sample terms
    [B, 2], the workspace), all allocated here on the current stream -- the caller keeps the workspace for as long as the launch may be replayed."""
    B, C_, H, W = target.shape
    dev = target.device
    with _on(dev):
        ws = torch.empty(int(L.call("nd_denoise_loss_workspace_bytes", B, C_, H * W)), dtype=torch.uint8, device=dev)
        terms, sample = _empty((3,), dev), _empty((B, 2), dev)
        L.call("nd_denoise_loss_f32", out.data_ptr(), layout, target.data_ptr(), B, C_, H * W, l1, mse, ws.data_ptr(), terms.data_ptr(), sample.data_ptr(),
               _stream(dev))
    return terms, sample, ws


def _denoise_loss_grad(out: torch.Tensor, layout: int, target: torch.Tensor, grad_loss: torch.Tensor, l1: float, mse: float) -> torch.Tensor:
    """nd_denoise_loss_backward_f32: the gradient of the loss with respect to ``out``, in ``out``'s layout; ``grad_loss`` is read on the device."""
    B, C_, H, W = target.shape
    dev = target.device
    g = grad_loss.to(dev, torch.float32).reshape(1).contiguous()
    with _on(dev):
        grad = torch.empty_like(out)
        L.call("nd_denoise_loss_backward_f32", out.data_ptr(), layout, target.data_ptr(), g.data_ptr(), grad.data_ptr(), B, C_, H * W, l1, mse, _stream(dev))
    return grad


def _loss_details(terms: torch.Tensor, sample: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The log line's tensors (models/trainer_denoising.py:225-235 logs both terms on every step): views of the kernel's outputs, on the device."""
    return {"l1": terms[1], "mse": terms[2], "sample_l1": sample[:, 0], "sample_mse": sample[:, 1]}


class DenoiseLossFunction(torch.autograd.Function):
    """``mse * F.mse_loss(output, target) + l1 * F.l1_loss(output, target)`` on nd_denoise_loss_f32 (fp64 sums in a fixed order) and
    nd_denoise_loss_backward_f32 (one pass, the upstream gradient read on the device).  Returns (loss, terms [3], sample terms [B, 2]); only the loss is
    differentiable.  The workspace is allocated here on the current stream and saved, so a captured graph owns it."""

    @staticmethod
    def forward(ctx, output, target, l1, mse):
        terms, sample, ws = _denoise_loss_launch(output, L.LAYOUT_NCHW, target, l1, mse)
        ctx.save_for_backward(output, target, ws)
        ctx.lambdas = (l1, mse)
        ctx.mark_non_differentiable(terms, sample)
        ctx.set_materialize_grads(False)                     # (no zero tensors -- two fill launches -- for the outputs nobody differentiates)
        return terms[0], terms, sample

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *unused):
        if grad_loss is None:
            return None, None, None, None
        output, target, _ws = ctx.saved_tensors
        return _denoise_loss_grad(output, L.LAYOUT_NCHW, target, grad_loss, *ctx.lambdas), None, None, None


def _check_denoise_pair(op: str, output: torch.Tensor, target: torch.Tensor) -> None:
    for what, x in (("output", output), ("target", target)):
        _need_gpu(x)
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"{op}: {what} {tuple(x.shape)} {x.dtype}: needs a contiguous 4-D (NCHW) fp32 tensor (there is no fallback)")
    if target.shape != output.shape or target.device != output.device:
        raise ValueError(f"{op}: output {tuple(output.shape)} on {output.device} and target {tuple(target.shape)} on {target.device} do not belong together")
    if target.requires_grad:
        raise ValueError(f"{op}: no gradient is produced for target; detach it")


def denoise_loss(output: torch.Tensor, target: torch.Tensor, l1: float = 1.0, mse: float = 0.0, *, details: bool = False):
    """The denoiser's training loss (models/trainer_denoising.py:66-76, 225-235: ``--loss_l1`` / ``--loss_mse`` weighted by ``--lambda_l1`` /
    ``--lambda_mse``) of a batch on the HIP library: ``mse * mean((output - target)^2) + l1 * mean|output - target|``, differentiable in ``output`` only.
    Both tensors NCHW-contiguous fp32 on one GPU, 1 to 16 channels; a CPU tensor raises HipError.  ``details``: also a dict of non-differentiable device
    tensors -- ``l1``, ``mse`` (the unweighted terms) and ``sample_l1``, ``sample_mse`` (B,), whose bits do not depend on the batch."""
    _check_denoise_pair("denoise_loss", output, target)
    l1, mse = float(l1), float(mse)
    _check_lambdas("denoise_loss", l1, mse)
    loss, terms, sample = DenoiseLossFunction.apply(output, target.detach(), l1, mse)
    return (loss, _loss_details(terms, sample)) if details else loss
