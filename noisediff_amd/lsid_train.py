"""``TrainableLSID``: the reference's denoiser (models/archs/SID_arch.py:49-175) trained on MI355X -- the fourth workflow of the reference
(train_denoising.py, script.sh:17: LSID, L1 loss, Adam) without the reference tree.

    net = noisediff_amd.TrainableLSID().cuda().hip()
    opt = noisediff_amd.train.Adam(net.parameters(), lr=1e-4)
    loss = net.loss(noisy, clean); loss.backward(); opt.step()        # (l1=, mse=: the trainer's --lambda_l1 / --lambda_mse)
    noisediff_amd.LSID(None).load_state_dict(net.state_dict())        # the HIP inference path takes the trained weights as they are

``net.loss`` is the network and the trainer's loss (mse * lambda_mse + l1 * lambda_l1, trainer_denoising.py:225-235) as ONE Function,
``_LsidLossFunction``: the forward stops at the 1x1 head's NHWC output, the loss kernel (denoise_loss.hip) reads it there and its backward writes the
head's gradient in that layout.  ``net(noisy)`` followed by any PyTorch loss keeps working: it pays the two layout passes and ATen's loss kernels.

Parameters are registered under the reference's names and shapes (spec.lsid_param_spec) with its init, so ``state_dict()`` loads strictly into
``noisediff_amd.LSID`` and into the reference class.  Without ``.hip()`` the forward is plain differentiable PyTorch (CPU or GPU): the restatement
tests/test_lsid_train.py pins against the reference's loss and gradients.  With ``.hip()`` the whole network is ONE torch.autograd.Function
(``_LsidFunction``) over the HIP library, forward and backward:

  forward   lsid.lsid_forward_hip, the launches the inference LSID records: every convolution stores its RAW pre-activation, the consumers
            apply LeakyReLU(0.2) in their prologue (ND_PRO_LEAKY / ND_PRO_LEAKY_SECOND), the ceil-mode max-pools run on raw values (max commutes
            with the activation), each ConvTranspose2d(2, s=2) is one pointwise GEMM with a pixel-shuffle store that also crops.  Saved: the raw
            tensors below, nothing activated.
  backward  in reverse: conv10's weight gradient (nd_linear_wgrad_leaky_f32) and data gradient (pointwise GEMM); per LeakyReLU the gradient join
            nd_leaky_grad_join_f32 (direct gradient + max-pool scatter, times the slope); per 3x3 convolution the weight gradient with the activation
            applied on load (nd_conv3x3_wgrad_leaky / _cat_leaky_second) and the data gradient as the forward kernels on dgrad-packed weights; per
            ConvTranspose the weight gradient nd_convt2x2_wgrad_leaky_f32 and the data gradient as a pointwise GEMM reading d_up through a cropped
            pixel unshuffle (nd_pointwise_gemm_unshuffle_crop_nhwc_f32).  The input gradient is not built (out of scope: nothing trains the image).

Every launch goes on torch's CURRENT stream, every buffer (packed weights, saved tensors, workspaces) comes from torch's caching allocator on that
stream and is owned by the autograd context: nothing is freed while a queued launch may still read it, and a whole step (forward, loss, backward,
train.Adam) captures into one torch.cuda.graph without parallel branches.  The weights are packed per forward (and per backward for the data
gradients) from the parameters as they are: no cache that an optimizer step could leave stale.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import synth, train
from .lsid import _Launcher, _sizes, head_to_nchw, lsid_forward_hip
from .spec import LSID_STAGES, lsid_param_spec

SLOPE = 0.2
# F(4x4,3x3) Winograd kernels where they take the layer (train.conv3x3_kind), for the forward / the data-gradient convolutions; False: F(2x2,3x3) there.
# Measured at B = 4, 256 x 256 against float64 (max |g - g64| / max |g64| over the parameters): F(4x4) forward 1.8e-4, F(2x2) forward 5.2e-5 --
# PyTorch's own fp32 path 6.3e-5; the data-gradient form changes none of these figures.  The forward is what the saved activations carry into
# every weight gradient, so training keeps it on F(2x2).
WINO4_FORWARD, WINO4_DGRAD = False, True
PARAM_NAMES: Tuple[str, ...] = tuple(p.name for p in lsid_param_spec())


# --------------------------------------------------------------------------------------------------------- the PyTorch restatement
def lsid_forward_torch(p: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """LSID.forward (SID_arch.py:105-175) as functional PyTorch over the parameter table."""
    act = lambda t: F.leaky_relu(t, SLOPE)
    conv = lambda n, t, pad=1: F.conv2d(t, p[n + ".weight"], p[n + ".bias"], padding=pad)
    skips = []
    for i in range(1, 6):
        x = act(conv(f"conv{i}_2", act(conv(f"conv{i}_1", x))))
        if i < 5:
            skips.append(x)
            x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    for i in range(6, 10):
        skip = skips.pop()
        x = F.conv_transpose2d(x, p[f"up{i}.weight"], stride=2)
        x = torch.cat((x[:, :, :skip.shape[2], :skip.shape[3]], skip), 1)
        x = act(conv(f"conv{i}_2", act(conv(f"conv{i}_1", x))))
    return conv("conv10", x, 0)


# --------------------------------------------------------------------------------------------------------- HIP launches
def convt2x2_dgrad(run: _Launcher, w: torch.Tensor, d_up: torch.Tensor, ld_up: int, B: int, h: int, w_: int, up_h: int, up_w: int) -> torch.Tensor:
    """The data gradient (B, h, w_, cin) of ConvTranspose2d(cin, c, 2, s=2) + crop to (up_h, up_w), weight ``w`` (cin, c, 2, 2): a pointwise GEMM
    over the zero-filled pixel unshuffle of ``d_up`` -- its first c channels, pixel stride ``ld_up``."""
    cin, c = w.shape[0], w.shape[1]
    t = run.empty(B, h, w_, cin)
    src = L.src(d_up, c=4 * c, ld=ld_up, unshuffle=1)
    run.pointwise(src, run.pack_pw(w.reshape(cin, 4 * c).contiguous(), 4 * c, cin, unshuffle_c=c), None, t, B, h * w_, w_, 4 * c, cin, cin,
                  crop_src=(up_h, up_w))
    return t


def _lsid_hip_backward(P: Dict[str, torch.Tensor], saved: Dict[str, torch.Tensor], grad_out: torch.Tensor, run: _Launcher) -> Dict[str, torch.Tensor]:
    """Weight and bias gradients of every parameter from the gradient of the (B, 4, H, W) output: one layout pass, then the backward from the head."""
    B, H, W, _ = saved["x8"].shape
    g = grad_out.detach().to(torch.float32).contiguous()
    run.keep.append(g)
    dy = run.empty(B, H, W, 4)
    L.call("nd_nchw_to_nhwc_f32", g.data_ptr(), dy.data_ptr(), B, 4, H, W, run.st)
    return _lsid_hip_backward_from_head(P, saved, dy, run)


def _lsid_hip_backward_from_head(P: Dict[str, torch.Tensor], saved: Dict[str, torch.Tensor], dy: torch.Tensor, run: _Launcher) -> Dict[str, torch.Tensor]:
    """Weight and bias gradients of every parameter from the raw tensors of the forward and ``dy`` (B, H, W, 4), the gradient of the 1x1 head's own
    output, in reverse launch order."""
    lib = run.lib
    x8 = saved["x8"]
    B, H, W, _ = x8.shape
    sizes = _sizes(H, W)
    G: Dict[str, torch.Tensor] = {}

    def ws(n: int) -> torch.Tensor:
        return run.empty(int(n))

    def wgrad3(name: str, x: torch.Tensor, dz: torch.Tensor, cin: int, ldx: int, leaky: bool) -> None:
        h, w, cout = dz.shape[1], dz.shape[2], dz.shape[3]
        gw, gb = run.empty(cout, cin, 3, 3), run.empty(cout)
        L.call("nd_conv3x3_wgrad_leaky_nhwc_f32" if leaky else "nd_conv3x3_wgrad_nhwc_f32", x.data_ptr(), ldx, dz.data_ptr(), cout, gw.data_ptr(),
               gb.data_ptr(), ws(lib.nd_conv3x3_wgrad_workspace_floats(B, h, w, cin, cout)).data_ptr(), B, h, w, cin, cout, run.st)
        G[name + ".weight"], G[name + ".bias"] = gw, gb

    # ---- conv10 (1x1 on leaky(z9)): weight / bias gradient, then the gradient of leaky(z9)
    c = LSID_STAGES[0]
    N = B * H * W
    gw, gb = run.empty(4, c), run.empty(4)
    L.call("nd_linear_wgrad_leaky_f32", saved["z9"].data_ptr(), c, dy.data_ptr(), 4, gw.data_ptr(), gb.data_ptr(),
           ws(lib.nd_linear_wgrad_workspace_floats(N, c, 4)).data_ptr(), N, c, 4, run.st)
    G["conv10.weight"], G["conv10.bias"] = gw.reshape(4, c, 1, 1), gb
    t = run.empty(B, H, W, c)
    run.pointwise(L.src(dy), run.pack_pw_t(P["conv10.weight"].reshape(4, c).contiguous(), 4, c), None, t, B, H * W, W, 4, c, c)
    dz = run.join(saved["z9"], t, t, c, None)
    # ---- up path, last stage first
    dcat: Dict[int, torch.Tensor] = {}
    for j in range(9, 5, -1):
        i = 10 - j
        c = LSID_STAGES[i - 1]
        cin = LSID_STAGES[i]
        h, w = sizes[i - 1]
        hp, wp_ = sizes[i]
        a = saved[f"a{j}"]
        wgrad3(f"conv{j}_2", a, dz, c, c, True)
        t = run.conv3x3(P[f"conv{j}_2.weight"], None, L.src(dz), B, h, w, c, c, dgrad=True)
        da = run.join(a, t, t, c, None)
        gw, gb = run.empty(c, 2 * c, 3, 3), run.empty(c)
        L.call("nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32", saved[f"u{j}"].data_ptr(), c, c, saved[f"z{i}"].data_ptr(), c, c, da.data_ptr(), c,
               gw.data_ptr(), gb.data_ptr(), ws(lib.nd_conv3x3_wgrad_cat_workspace_floats(B, h, w, c, c, c)).data_ptr(), B, h, w, c, run.st)
        G[f"conv{j}_1.weight"], G[f"conv{j}_1.bias"] = gw, gb
        dc = run.conv3x3(P[f"conv{j}_1.weight"], None, L.src(da), B, h, w, c, 2 * c, dgrad=True)     # [d up | d leaky(skip)]
        dcat[i] = dc
        # ConvTranspose2d(cin -> c) on leaky(z_prev) + crop: weight gradient, then the gradient of leaky(z_prev)
        zp = saved[f"z{j - 1}"] if j > 6 else saved["z5"]
        gw = run.empty(cin, c, 2, 2)
        L.call("nd_convt2x2_wgrad_leaky_f32", zp.data_ptr(), cin, dc.data_ptr(), 2 * c, gw.data_ptr(),
               ws(lib.nd_convt2x2_wgrad_workspace_floats(B, hp, wp_, cin, c)).data_ptr(), B, hp, wp_, cin, c, h, w, run.st)
        G[f"up{j}.weight"] = gw
        t = convt2x2_dgrad(run, P[f"up{j}.weight"], dc, 2 * c, B, hp, wp_, h, w)
        dz = run.join(zp, t, t, cin, None)
    # ---- down path, deepest stage first; dz is the gradient of z5
    d_pool: Optional[torch.Tensor] = None
    for i in range(5, 0, -1):
        c = LSID_STAGES[i - 1]
        h, w = sizes[i - 1]
        if i < 5:                                            # skip half of the concat convolution's data gradient + the pooled gradient
            dz = run.join(saved[f"z{i}"], run.empty(B, h, w, c), dcat[i], 2 * c, d_pool, direct_offset=c)
        a = saved[f"a{i}"]
        wgrad3(f"conv{i}_2", a, dz, c, c, True)
        t = run.conv3x3(P[f"conv{i}_2.weight"], None, L.src(dz), B, h, w, c, c, dgrad=True)
        da = run.join(a, t, t, c, None)
        if i > 1:
            cprev = LSID_STAGES[i - 2]
            wgrad3(f"conv{i}_1", saved[f"p{i - 1}"], da, cprev, cprev, True)
            d_pool = run.conv3x3(P[f"conv{i}_1.weight"], None, L.src(da), B, h, w, c, cprev, dgrad=True)
        else:
            wgrad3("conv1_1", x8, da, 4, 8, False)          # the image itself: no activation, 4 of the 8 staged channels
    return G


class _LsidFunction(torch.autograd.Function):
    """The whole LSID forward and backward on libnoisediff_hip; inputs (x, *parameters in PARAM_NAMES order)."""

    @staticmethod
    def forward(ctx, x, *params):
        P = dict(zip(PARAM_NAMES, (p.detach() for p in params)))
        run = _Launcher(x.device, WINO4_FORWARD)
        saved: Dict[str, torch.Tensor] = {}
        with torch.cuda.device(x.device):
            out = lsid_forward_hip(P, x, saved, run)
        ctx.saved = saved                                    # raw tensors only; the packed weights and staging buffers are dropped with ``run``
        ctx.save_for_backward(*params)                       # (version-checked: an optimizer step between forward and backward raises)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        params = ctx.saved_tensors
        P = dict(zip(PARAM_NAMES, (p.detach() for p in params)))
        run = _Launcher(grad_out.device, WINO4_DGRAD)
        with torch.cuda.device(grad_out.device):
            G = _lsid_hip_backward(P, ctx.saved, grad_out, run)
        ctx.saved = None
        return (None,) + tuple(G[n] if need else None for n, need in zip(PARAM_NAMES, ctx.needs_input_grad[1:]))


class _LsidLossFunction(torch.autograd.Function):
    """The network and the trainer's loss as one Function: the forward stops at the 1x1 head's NHWC output, nd_denoise_loss_f32 reads it against the NCHW
    ``clean``, and the backward has nd_denoise_loss_backward_f32 write the head's gradient where _lsid_hip_backward_from_head reads it -- no layout pass
    in either direction.  Inputs (x, clean, l1, mse, want_output, *parameters in PARAM_NAMES order); outputs (loss, terms [3], sample terms [B, 2],
    the (B, 4, H, W) output or None), only the loss differentiable."""

    @staticmethod
    def forward(ctx, x, clean, l1, mse, want_output, *params):
        P = dict(zip(PARAM_NAMES, (p.detach() for p in params)))
        run = _Launcher(x.device, WINO4_FORWARD)
        saved: Dict[str, torch.Tensor] = {}
        with torch.cuda.device(x.device):
            y = lsid_forward_hip(P, x, saved, run, head_nhwc=True)
            terms, sample, ws = train._denoise_loss_launch(y, L.LAYOUT_NHWC, clean, l1, mse)
            out = head_to_nchw(run, y) if want_output else None
        ctx.saved, ctx.head, ctx.lambdas = saved, (y, clean, ws), (l1, mse)      # (ws: the launch's workspace lives as long as the step's graph node)
        ctx.save_for_backward(*params)
        ctx.mark_non_differentiable(*(t for t in (terms, sample, out) if t is not None))
        ctx.set_materialize_grads(False)                     # (no zero tensors -- fill launches -- for the outputs nobody differentiates)
        return terms[0], terms, sample, out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, *unused):
        if grad_loss is None:
            return (None,) * (5 + len(PARAM_NAMES))
        params = ctx.saved_tensors
        P = dict(zip(PARAM_NAMES, (p.detach() for p in params)))
        y, clean, _ws = ctx.head
        run = _Launcher(y.device, WINO4_DGRAD)
        with torch.cuda.device(y.device):
            dy = train._denoise_loss_grad(y, L.LAYOUT_NHWC, clean, grad_loss, *ctx.lambdas)
            G = _lsid_hip_backward_from_head(P, ctx.saved, dy, run)
        ctx.saved = ctx.head = None
        return (None,) * 5 + tuple(G[n] if need else None for n, need in zip(PARAM_NAMES, ctx.needs_input_grad[5:]))


def denoise_lr(epoch: int, max_iter: int, base_lr: float) -> float:
    """The trainer's step schedule (models/trainer_denoising.py:185-188) for epoch ``epoch`` of ``max_iter``: the base rate, half of it after
    ``max_iter // 2``, 1e-5 after ``int(0.8 * max_iter)``.  Feed it to ``train.Adam.set_lr``: with a tensor lr a captured step follows it."""
    if epoch > int(max_iter * 0.8):
        return 1e-5
    if epoch > max_iter // 2:
        return base_lr / 2.
    return base_lr


# --------------------------------------------------------------------------------------------------------- the module
class TrainableLSID(nn.Module):
    """``TrainableLSID(args=None)``: the reference's ``LSID(args)`` for training (4 input channels; ``args`` is accepted and unused, as there).
    ``.hip()`` moves forward and backward onto the HIP library (CUDA tensors; raises without the library)."""

    def __init__(self, args=None, seed: int = 0):
        super().__init__()
        self.block_size = 2
        self._hip = False
        for name, value in synth.make_state_dict(lsid_param_spec(), seed).items():     # N(0, sqrt(2 / (k*k*out))) weights, zero biases (SID_arch.py:96-103)
            mod, leaf = name.rsplit(".", 1)
            if mod not in self._modules:
                self.add_module(mod, nn.Module())
            self._modules[mod].register_parameter(leaf, nn.Parameter(value))

    def hip(self, on: bool = True) -> "TrainableLSID":
        if on:
            L.load()
        self._hip = bool(on)
        return self

    def _table(self) -> Dict[str, torch.Tensor]:
        return {n: getattr(self._modules[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1]) for n in PARAM_NAMES}

    def _check_hip_input(self, P: Dict[str, torch.Tensor], x: torch.Tensor) -> bool:
        """What the HIP path takes; True when the pass is differentiated (grad mode on and a parameter requires grad)."""
        if x.device.type != "cuda" or any(p.device != x.device for p in P.values()):
            raise L.HipError(f"TrainableLSID.hip() runs on the HIP library only: the input and every parameter must be on one GPU (input on {x.device})")
        if x.dim() != 4 or x.shape[1] != 4:
            raise ValueError(f"TrainableLSID takes (B, 4, H, W) images, got {tuple(x.shape)}")
        if x.requires_grad:
            raise ValueError("TrainableLSID.hip() does not compute the gradient of its input (conv1_1's data gradient is out of scope): "
                             "pass an input that does not require grad, or use TrainableLSID without .hip()")
        if any(p.dtype != torch.float32 for p in P.values()):
            raise ValueError("TrainableLSID.hip() trains fp32 parameters")
        return torch.is_grad_enabled() and any(p.requires_grad for p in P.values())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        P = self._table()
        if not self._hip:
            return lsid_forward_torch(P, x)
        if not self._check_hip_input(P, x):
            with torch.no_grad():
                return _LsidFunction.forward(_NoCtx(), x, *[P[n] for n in PARAM_NAMES])
        return _LsidFunction.apply(x, *[P[n] for n in PARAM_NAMES])

    def loss(self, noisy: torch.Tensor, clean: torch.Tensor, l1: float = 1.0, mse: float = 0.0, *, details: bool = False, return_output: bool = False):
        """The trainer's loss of a batch (models/trainer_denoising.py:220-235): ``mse * F.mse_loss(net(noisy), clean) + l1 * F.l1_loss(net(noisy), clean)``.
        With ``.hip()`` the network and the loss are ONE autograd Function (``_LsidLossFunction``): the loss kernel reads the head's NHWC output and its
        backward writes the head's gradient, in fp64 sums of a fixed order (train.denoise_loss's contract).  ``clean``: (B, 4, H, W) fp32, contiguous, on
        the input's device, no gradient.  Returns the loss; with ``details`` then a dict of detached tensors for the log line (``l1``, ``mse``: the
        unweighted terms; ``sample_l1``, ``sample_mse``: (B,)); with ``return_output`` then the detached (B, 4, H, W) output."""
        l1, mse = float(l1), float(mse)
        train._check_lambdas("TrainableLSID.loss", l1, mse)
        P = self._table()
        if not self._hip:
            out = lsid_forward_torch(P, noisy)
            loss = mse * F.mse_loss(out, clean) + l1 * F.l1_loss(out, clean)
            info = None
            if details:
                d = (out - clean).detach().flatten(1)
                info = {"l1": d.abs().mean(), "mse": (d * d).mean(), "sample_l1": d.abs().mean(1), "sample_mse": (d * d).mean(1)}
            out = out.detach()
        else:
            differentiated = self._check_hip_input(P, noisy)
            train._need_gpu(clean)
            if tuple(clean.shape) != tuple(noisy.shape) or clean.device != noisy.device or clean.dtype != torch.float32 or not clean.is_contiguous():
                raise ValueError(f"TrainableLSID.loss: clean {tuple(clean.shape)} {clean.dtype} must be a contiguous fp32 tensor of the input's shape "
                                 f"{tuple(noisy.shape)} on its device")
            if clean.requires_grad:
                raise ValueError("TrainableLSID.loss: no gradient is produced for clean; detach it")
            args = (noisy, clean, l1, mse, bool(return_output), *[P[n] for n in PARAM_NAMES])
            if differentiated:
                loss, terms, sample, out = _LsidLossFunction.apply(*args)
            else:
                with torch.no_grad():
                    loss, terms, sample, out = _LsidLossFunction.forward(_NoCtx(), *args)
            info = train._loss_details(terms, sample) if details else None
        res = (loss,) + ((info,) if details else ()) + ((out,) if return_output else ())
        return res[0] if len(res) == 1 else res


class _NoCtx:
    """Stands in for the autograd context of a forward nobody differentiates (under torch.no_grad / inference)."""

    def save_for_backward(self, *a):
        pass

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, value):
        pass
