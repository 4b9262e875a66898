"""NoiseDiffNet training kernels at the training step's own shapes: one ``TrainableNoiseDiffNet(...).hip()`` step of the README's B = 4, 256 x 256 at
d = 64 and at d = 48 (the reference's shipped width), against float64 on the CPU.

``TRAIN_SHAPES`` lists every (operation, shape) pair such a step runs through ``noisediff_amd.train``; a recorded step pins it to the product.  The tests
then run the norm_train.hip kernels (GroupNorm, GroupNorm + SiLU, the token sum, per-pixel modulation) at those shapes -- 256 pixel slots from
HW = 16384 on, group widths that do not divide 256 (d = 48) -- and the conv3x3 forward / data / weight gradients and the convolution-statistics
GroupNorm path, the 7x7 stem's weight gradient.  The bounds are those of the small-shape tests (tests/test_train_gpu.py): none grows with the shape."""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from noisediff_amd import GaussianDiffusion, TrainableNoiseDiffNet, _lib as L, synth, train, trainable
from util import rel_err

DEV = torch.device("cuda", 0)
B, S = 4, 256                                     # the README's training step

# (operation, shape) -> the widths d whose step runs it.  Shapes: conv3x3* (B, H, W, cin[, cin of the second source], cout); group_norm (B, H, W, C, groups);
# gn_silu (..., what rides along: the time embedding's modulation, the block's shortcut, the producing convolution's statistics); modulate_silu (B, H, W, C);
# layer_norm (tokens, C); linear (tokens, cin, cout, residual in the epilogue or not); conv1x1* (B, H, W, cin[, c1], cout[, residual]); stem (B, H, W, cout);
# token_sum (B, tokens, C): broadcast_add, whose gradient is nd_token_sum_f32.
TRAIN_SHAPES = {
    ('conv1x1', 4, 256, 256, 16, 8, 'plain'): (64, 48),
    ('conv1x1', 4, 256, 256, 24, 16, 'plain'): (64, 48),
    ('conv1x1', 4, 256, 256, 4, 8, 'plain'): (64, 48),
    ('conv1x1', 4, 256, 256, 48, 4, 'plain'): (48,),
    ('conv1x1', 4, 256, 256, 48, 48, 'plain'): (48,),
    ('conv1x1', 4, 256, 256, 48, 48, 'res'): (48,),
    ('conv1x1', 4, 256, 256, 64, 4, 'plain'): (64,),
    ('conv1x1', 4, 256, 256, 64, 64, 'plain'): (64,),
    ('conv1x1', 4, 256, 256, 64, 64, 'res'): (64,),
    ('conv1x1', 4, 256, 256, 8, 128, 'plain'): (64,),
    ('conv1x1', 4, 256, 256, 8, 48, 'plain'): (48,),
    ('conv1x1', 4, 256, 256, 8, 64, 'plain'): (64,),
    ('conv1x1', 4, 256, 256, 8, 96, 'plain'): (48,),
    ('conv1x1', 4, 128, 128, 128, 128, 'res'): (64,),
    ('conv1x1', 4, 128, 128, 192, 48, 'plain'): (48,),
    ('conv1x1', 4, 128, 128, 256, 64, 'plain'): (64,),
    ('conv1x1', 4, 128, 128, 48, 48, 'res'): (48,),
    ('conv1x1', 4, 128, 128, 64, 64, 'res'): (64,),
    ('conv1x1', 4, 128, 128, 96, 96, 'res'): (48,),
    ('conv1x1', 4, 64, 64, 128, 128, 'res'): (64,),
    ('conv1x1', 4, 64, 64, 192, 192, 'res'): (48,),
    ('conv1x1', 4, 64, 64, 192, 96, 'plain'): (48,),
    ('conv1x1', 4, 64, 64, 256, 128, 'plain'): (64,),
    ('conv1x1', 4, 64, 64, 256, 256, 'res'): (64,),
    ('conv1x1', 4, 64, 64, 96, 96, 'res'): (48,),
    ('conv1x1', 4, 32, 32, 192, 192, 'res'): (48,),
    ('conv1x1', 4, 32, 32, 256, 256, 'res'): (64,),
    ('conv1x1', 4, 32, 32, 384, 192, 'plain'): (48,),
    ('conv1x1', 4, 32, 32, 384, 384, 'res'): (48,),
    ('conv1x1', 4, 32, 32, 512, 256, 'plain'): (64,),
    ('conv1x1', 4, 32, 32, 512, 512, 'res'): (64,),
    ('conv1x1_shortcut_cat', 4, 256, 256, 48, 48, 48): (48,),
    ('conv1x1_shortcut_cat', 4, 256, 256, 64, 64, 64): (64,),
    ('conv1x1_shortcut_cat', 4, 128, 128, 128, 64, 128): (64,),
    ('conv1x1_shortcut_cat', 4, 128, 128, 96, 48, 96): (48,),
    ('conv1x1_shortcut_cat', 4, 64, 64, 192, 96, 192): (48,),
    ('conv1x1_shortcut_cat', 4, 64, 64, 256, 128, 256): (64,),
    ('conv1x1_shortcut_cat', 4, 32, 32, 384, 192, 384): (48,),
    ('conv1x1_shortcut_cat', 4, 32, 32, 512, 256, 512): (64,),
    ('conv3x3', 4, 256, 256, 128, 64): (64,),
    ('conv3x3', 4, 256, 256, 48, 48): (48,),
    ('conv3x3', 4, 256, 256, 64, 64): (64,),
    ('conv3x3', 4, 256, 256, 96, 48): (48,),
    ('conv3x3', 4, 128, 128, 192, 96): (48,),
    ('conv3x3', 4, 128, 128, 256, 128): (64,),
    ('conv3x3', 4, 64, 64, 384, 192): (48,),
    ('conv3x3', 4, 64, 64, 512, 256): (64,),
    ('conv3x3', 4, 32, 32, 192, 384): (48,),
    ('conv3x3', 4, 32, 32, 256, 512): (64,),
    ('conv3x3_cat_stats', 4, 256, 256, 48, 48, 48): (48,),
    ('conv3x3_cat_stats', 4, 256, 256, 64, 64, 64): (64,),
    ('conv3x3_cat_stats', 4, 128, 128, 128, 64, 128): (64,),
    ('conv3x3_cat_stats', 4, 128, 128, 96, 48, 96): (48,),
    ('conv3x3_cat_stats', 4, 64, 64, 192, 96, 192): (48,),
    ('conv3x3_cat_stats', 4, 64, 64, 256, 128, 256): (64,),
    ('conv3x3_cat_stats', 4, 32, 32, 384, 192, 384): (48,),
    ('conv3x3_cat_stats', 4, 32, 32, 512, 256, 512): (64,),
    ('conv3x3_stats', 4, 256, 256, 48, 48): (48,),
    ('conv3x3_stats', 4, 256, 256, 64, 64): (64,),
    ('conv3x3_stats', 4, 128, 128, 128, 128): (64,),
    ('conv3x3_stats', 4, 128, 128, 48, 48): (48,),
    ('conv3x3_stats', 4, 128, 128, 64, 64): (64,),
    ('conv3x3_stats', 4, 128, 128, 96, 96): (48,),
    ('conv3x3_stats', 4, 64, 64, 128, 128): (64,),
    ('conv3x3_stats', 4, 64, 64, 192, 192): (48,),
    ('conv3x3_stats', 4, 64, 64, 256, 256): (64,),
    ('conv3x3_stats', 4, 64, 64, 96, 96): (48,),
    ('conv3x3_stats', 4, 32, 32, 192, 192): (48,),
    ('conv3x3_stats', 4, 32, 32, 256, 256): (64,),
    ('conv3x3_stats', 4, 32, 32, 384, 384): (48,),
    ('conv3x3_stats', 4, 32, 32, 512, 512): (64,),
    ('gn_silu', 4, 256, 256, 48, 2, 'mod+stats'): (48,),
    ('gn_silu', 4, 256, 256, 48, 2, 'res+stats'): (48,),
    ('gn_silu', 4, 256, 256, 48, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 256, 256, 48, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 256, 256, 64, 2, 'mod+stats'): (64,),
    ('gn_silu', 4, 256, 256, 64, 2, 'res+stats'): (64,),
    ('gn_silu', 4, 256, 256, 64, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 256, 256, 64, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 128, 128, 128, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 128, 128, 128, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 128, 128, 48, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 128, 128, 48, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 128, 128, 64, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 128, 128, 64, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 128, 128, 96, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 128, 128, 96, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 64, 64, 128, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 64, 64, 128, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 64, 64, 192, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 64, 64, 192, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 64, 64, 256, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 64, 64, 256, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 64, 64, 96, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 64, 64, 96, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 32, 32, 192, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 32, 32, 192, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 32, 32, 256, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 32, 32, 256, 8, 'res+stats'): (64,),
    ('gn_silu', 4, 32, 32, 384, 8, 'mod+stats'): (48,),
    ('gn_silu', 4, 32, 32, 384, 8, 'res+stats'): (48,),
    ('gn_silu', 4, 32, 32, 512, 8, 'mod+stats'): (64,),
    ('gn_silu', 4, 32, 32, 512, 8, 'res+stats'): (64,),
    ('group_norm', 4, 256, 256, 48, 2): (48,),
    ('group_norm', 4, 256, 256, 64, 2): (64,),
    ('layer_norm', 262144, 64): (64,),
    ('layer_norm', 262144, 48): (48,),
    ('layer_norm', 65536, 128): (64,),
    ('layer_norm', 65536, 96): (48,),
    ('layer_norm', 65536, 64): (64,),
    ('layer_norm', 65536, 48): (48,),
    ('layer_norm', 16384, 256): (64,),
    ('layer_norm', 16384, 192): (48,),
    ('layer_norm', 16384, 128): (64,),
    ('layer_norm', 16384, 96): (48,),
    ('layer_norm', 4096, 512): (64,),
    ('layer_norm', 4096, 384): (48,),
    ('layer_norm', 4096, 256): (64,),
    ('layer_norm', 4096, 192): (48,),
    ('linear', 262144, 128, 64, 'res'): (64,),
    ('linear', 262144, 96, 48, 'res'): (48,),
    ('linear', 262144, 64, 128, 'plain'): (64,),
    ('linear', 262144, 48, 96, 'plain'): (48,),
    ('linear', 65536, 256, 128, 'res'): (64,),
    ('linear', 65536, 192, 96, 'res'): (48,),
    ('linear', 65536, 128, 256, 'plain'): (64,),
    ('linear', 65536, 128, 64, 'res'): (64,),
    ('linear', 65536, 96, 192, 'plain'): (48,),
    ('linear', 65536, 96, 48, 'res'): (48,),
    ('linear', 65536, 64, 128, 'plain'): (64,),
    ('linear', 65536, 48, 96, 'plain'): (48,),
    ('linear', 16384, 512, 256, 'res'): (64,),
    ('linear', 16384, 384, 192, 'res'): (48,),
    ('linear', 16384, 256, 512, 'plain'): (64,),
    ('linear', 16384, 256, 128, 'res'): (64,),
    ('linear', 16384, 192, 384, 'plain'): (48,),
    ('linear', 16384, 192, 96, 'res'): (48,),
    ('linear', 16384, 128, 256, 'plain'): (64,),
    ('linear', 16384, 96, 192, 'plain'): (48,),
    ('linear', 4096, 1024, 512, 'res'): (64,),
    ('linear', 4096, 768, 384, 'res'): (48,),
    ('linear', 4096, 512, 1024, 'plain'): (64,),
    ('linear', 4096, 512, 256, 'res'): (64,),
    ('linear', 4096, 384, 768, 'plain'): (48,),
    ('linear', 4096, 384, 192, 'res'): (48,),
    ('linear', 4096, 256, 512, 'plain'): (64,),
    ('linear', 4096, 192, 384, 'plain'): (48,),
    ('linear', 4, 256, 8192, 'plain'): (64,),
    ('linear', 4, 256, 256, 'plain'): (64,),
    ('linear', 4, 192, 6144, 'plain'): (48,),
    ('linear', 4, 192, 192, 'plain'): (48,),
    ('linear', 4, 128, 512, 'plain'): (64,),
    ('linear', 4, 128, 384, 'plain'): (48,),
    ('linear', 4, 128, 256, 'plain'): (64,),
    ('linear', 4, 128, 192, 'plain'): (48,),
    ('linear', 4, 128, 128, 'plain'): (64,),
    ('linear', 4, 128, 96, 'plain'): (48,),
    ('linear', 4, 128, 64, 'plain'): (64,),
    ('linear', 4, 128, 48, 'plain'): (48,),
    ('linear', 4, 64, 256, 'plain'): (64,),
    ('linear', 4, 48, 192, 'plain'): (48,),
    ('linear', 4, 16, 128, 'plain'): (64, 48),
    ('modulate_silu', 4, 256, 256, 48): (48,),
    ('modulate_silu', 4, 256, 256, 64): (64,),
    ('stem', 4, 256, 256, 48): (48,),
    ('stem', 4, 256, 256, 64): (64,),
    ('token_sum', 4, 65536, 64): (64,),
    ('token_sum', 4, 65536, 48): (48,),
    ('token_sum', 4, 16384, 128): (64,),
    ('token_sum', 4, 16384, 96): (48,),
    ('token_sum', 4, 16384, 64): (64,),
    ('token_sum', 4, 16384, 48): (48,),
    ('token_sum', 4, 4096, 256): (64,),
    ('token_sum', 4, 4096, 192): (48,),
    ('token_sum', 4, 4096, 128): (64,),
    ('token_sum', 4, 4096, 96): (48,),
    ('token_sum', 4, 1024, 512): (64,),
    ('token_sum', 4, 1024, 384): (48,),
    ('token_sum', 4, 1024, 256): (64,),
    ('token_sum', 4, 1024, 192): (48,),
}
def _key(op, a):
    """The (operation, shape) pair of one call of ``train.<op>`` whose arguments, bound by name, are ``a``."""
    if op in ("conv3x3", "conv3x3_with_stats"):
        Bn, cin, H, W = a["x"].shape
        return ("conv3x3" if op == "conv3x3" else "conv3x3_stats", Bn, H, W, cin, a["weight"].shape[0])
    if op == "conv3x3_cat":
        Bn, c0, H, W = a["x0"].shape
        return ("conv3x3_cat_stats" if a["with_stats"] else "conv3x3_cat", Bn, H, W, c0, a["x1"].shape[1], a["weight"].shape[0])
    if op == "group_norm":
        Bn, C_, H, W = a["x"].shape
        return ("group_norm", Bn, H, W, C_, a["groups"])
    if op == "group_norm_silu":
        Bn, C_, H, W = a["x"].shape
        parts = [n for n, v in (("mod", a["scale_shift"]), ("res", a["res"]), ("stats", a["conv_stats"])) if v is not None]
        return ("gn_silu", Bn, H, W, C_, a["groups"], "+".join(parts) or "plain")
    if op == "modulate_silu":
        Bn, C_, H, W = a["n"].shape
        return ("modulate_silu", Bn, H, W, C_)
    if op == "layer_norm":
        return ("layer_norm", a["x"].numel() // a["x"].shape[-1], a["x"].shape[-1])
    if op == "linear":
        cout, cin = a["weight"].shape
        return ("linear", a["x"].numel() // cin, cin, cout, "res" if a["res"] is not None else "plain")
    if op == "conv1x1":
        Bn, cin, H, W = a["x"].shape
        return ("conv1x1", Bn, H, W, cin, a["weight"].shape[0], "res" if a["res"] is not None else "plain")
    if op in ("conv1x1_cat", "conv1x1_shortcut_cat"):
        Bn, c0, H, W = a["x0"].shape
        return (op, Bn, H, W, c0, a["x1"].shape[1], a["weight"].shape[0])
    if op == "conv7x7_c4":
        Bn, _, H, W = a["x"].shape
        return ("stem", Bn, H, W, a["weight"].shape[0])
    if op == "broadcast_add":
        Bn, N, C_ = a["tokens"].shape
        return ("token_sum", Bn, N, C_)
    raise KeyError(op)


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(23, name, shape, lo, hi)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _of(*ops):
    return sorted(k for k in TRAIN_SHAPES if k[0] in ops)


# ====================================================================================================== 1. the table is the step's
def test_the_shape_table_is_what_a_training_step_runs(monkeypatch):
    """One GaussianDiffusion.p_losses step (forward and backward) of TrainableNoiseDiffNet(dim).hip() at B = 4, 256 x 256 for d = 64 and d = 48, with every
    autograd entry point of ``train`` wrapped to record its (operation, shape): the records of each width are exactly that width's entries of
    TRAIN_SHAPES (a call made inside another entry point, conv1x1's linear, counts as the outer one), and no layer left the library."""
    ops = ["conv3x3", "conv3x3_with_stats", "conv3x3_cat", "group_norm", "group_norm_silu", "modulate_silu", "layer_norm", "linear", "conv1x1",
           "conv1x1_cat", "conv1x1_shortcut_cat", "conv7x7_c4", "broadcast_add"]
    for dim in (64, 48):
        seen, depth = set(), [0]
        with monkeypatch.context() as mp:
            for op in ops:
                real = getattr(train, op)

                def wrapper(*a, _real=real, _sig=inspect.signature(real), _op=op, **k):
                    if depth[0] == 0:
                        bound = _sig.bind(*a, **k)
                        bound.apply_defaults()
                        seen.add(_key(_op, bound.arguments))
                    depth[0] += 1
                    try:
                        return _real(*a, **k)
                    finally:
                        depth[0] -= 1
                mp.setattr(train, op, wrapper)
            trainable.FALLBACKS.clear()
            net = TrainableNoiseDiffNet(SimpleNamespace(dim=dim)).to(DEV).hip()
            gd = GaussianDiffusion(net, image_size=S, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(DEV)
            x0, noise = U("step.x0", (B, 4, S, S)).to(DEV), synth.make_noise(5, "step.noise", B, 4, S).to(DEV)
            cond = {k: v.to(DEV) for k, v in synth.make_condition(B, S, seed=1).items()}
            loss = gd.p_losses(x0, torch.tensor([3, 250, 500, 777], device=DEV), cond, noise=noise)
            loss.backward()
            assert bool(torch.isfinite(loss)) and trainable.FALLBACKS == {}, trainable.FALLBACKS
        want = {k for k, dims in TRAIN_SHAPES.items() if dim in dims}
        assert not seen - want, f"d = {dim}: layers of the step missing from TRAIN_SHAPES: {sorted(seen - want, key=str)}"
        assert not want - seen, f"d = {dim}: TRAIN_SHAPES entries the step does not run: {sorted(want - seen, key=str)}"
        del net, gd, loss
    torch.cuda.empty_cache()


# ====================================================================================================== 2. the GroupNorm family
# (B, H, W, C, groups) of every GroupNorm of the step, then the edges next to them: around the switch to 256 pixel slots (HW = 16383 / 16384 / 16385), a
# ragged HW >= 16384 (257 x 255 = 65535, not a multiple of 256), the widest group the kernels take (cpg = 512)
GN_SHAPES = sorted({k[1:6] for k in _of("group_norm", "gn_silu")}) + [(2, 127, 129, 48, 8), (2, 64, 256, 96, 8), (2, 113, 145, 64, 2), (2, 257, 255, 48, 2),
                                                                   (1, 129, 130, 1024, 2), (1, 16, 24, 1024, 2)]
GN_IDS = ["x".join(map(str, s)) for s in GN_SHAPES]


def _gn_inputs(tag, shape):
    """x with a large per-channel mean (the kernels' pivot keeps the sum of squares well conditioned), gamma, beta, dy: as GN_CASES."""
    Bn, H, W, C_, G = shape
    x = (U(tag + ".x", (Bn, C_, H, W), -1.5, 1.5) + 3.0 * U(tag + ".m", (Bn, C_, 1, 1))).to(DEV)
    return x, U(tag + ".g", (C_,), 0.5, 1.5).to(DEV), U(tag + ".b", (C_,)).to(DEV), U(tag + ".gy", (Bn, C_, H, W)).to(DEV)


def _runs(fn, leaves, fmts=(torch.channels_last, torch.channels_last, torch.contiguous_format)):
    """leaves = (*inputs, gy): y = fn(*fresh copies of the inputs, the first one in memory format ``fmt``; None stays None), y.backward(gy), once per
    entry of ``fmts``; returns [[y, the inputs' gradients...] per run] on the CPU."""
    *ts, gy = leaves
    outs = []
    for fmt in fmts:
        a = [t.clone().contiguous(memory_format=fmt).requires_grad_() if i == 0 else (None if t is None else t.clone().requires_grad_()) for i, t in enumerate(ts)]
        y = fn(*a)
        y.backward(gy)
        outs.append([y.detach().float().cpu().contiguous()] + [t.grad.float().cpu().contiguous() for t in a if t is not None])
    return outs


def _same_bits(outs, what):
    for i, run in enumerate(outs[1:], 1):
        for j, (p, q) in enumerate(zip(outs[0], run)):
            assert torch.equal(p, q), (what, "run", i, "output", j)


@pytest.mark.parametrize("shape", GN_SHAPES, ids=GN_IDS)
def test_group_norm_at_the_step_shapes_matches_float64(shape):
    """train.group_norm (nd_groupnorm_train_forward / _backward): y, dx, dgamma, dbeta against float64 at 2e-5, on channels_last (twice: the same bits) and
    NCHW input (the same bits again)."""
    Bn, H, W, C_, G = shape
    x, gamma, beta, gy = _gn_inputs(f"gn.{shape}", shape)
    outs = _runs(lambda a, w, b: train.group_norm(a, G, w, b, 1e-5), (x, gamma, beta, gy))
    _same_bits(outs, "group_norm")
    xd, wd, bd = (t.double().cpu().requires_grad_() for t in (x, gamma, beta))
    y = F.group_norm(xd, G, wd, bd, 1e-5)
    y.backward(gy.double().cpu())
    for got, ref, name in zip(outs[0], (y, xd.grad, wd.grad, bd.grad), ("y", "dx", "dgamma", "dbeta")):
        assert got.shape == ref.shape
        assert rel_err(got.numpy(), ref.detach().numpy()) < 2e-5, (shape, name)


@pytest.mark.parametrize("tail", ["plain", "mod", "res"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=GN_IDS)
def test_group_norm_silu_at_the_step_shapes_matches_float64(shape, tail):
    """train.group_norm_silu (nd_groupnorm_silu_train_forward / _backward, the norm's own statistics pass): silu(group_norm(x) (* (scale + 1) + shift))
    (+ res) and its y, dx, dgamma, dbeta, d(scale | shift), dres against float64 at 3e-5; channels_last twice and NCHW: the same bits."""
    Bn, H, W, C_, G = shape
    x, gamma, beta, gy = _gn_inputs(f"gs.{shape}", shape)
    ss = U(f"gs.ss.{shape}", (Bn, 2 * C_), -0.5, 0.5).to(DEV) if tail == "mod" else None
    res = U(f"gs.r.{shape}", (Bn, C_, H, W)).to(DEV) if tail == "res" else None
    outs = _runs(lambda a, w, b, s, r: train.group_norm_silu(a, G, w, b, s, 1e-5, res=r), (x, gamma, beta, ss, res, gy))
    _same_bits(outs, "group_norm_silu")
    xd, wd, bd = (t.double().cpu().requires_grad_() for t in (x, gamma, beta))
    n = F.group_norm(xd, G, wd, bd, 1e-5)
    extra = []
    if ss is not None:
        sd = ss.double().cpu().requires_grad_()
        n = n * (sd[:, :C_, None, None] + 1) + sd[:, C_:, None, None]
        extra.append(sd)
    y = F.silu(n)
    if res is not None:
        rd = res.double().cpu().requires_grad_()
        y = y + rd
        extra.append(rd)
    y.backward(gy.double().cpu())
    for got, ref, name in zip(outs[0], [y, xd.grad, wd.grad, bd.grad] + [t.grad for t in extra], ("y", "dx", "dgamma", "dbeta", "dextra0", "dextra1")):
        assert got.shape == ref.shape, name
        assert rel_err(got.numpy(), ref.detach().numpy()) < 3e-5, (shape, tail, name)


@pytest.mark.parametrize("shape", [(4, 256, 256, 48, 2), (4, 256, 256, 48, 8), (2, 257, 255, 48, 2), (1, 129, 130, 1024, 2), (4, 128, 128, 96, 8)],
                         ids=lambda s: "x".join(map(str, s)))
def test_group_norm_c_abi_writes_every_output_and_saves_exact_statistics(shape):
    """The four GroupNorm entry points called directly on NaN-filled outputs and workspaces (an element a kernel never writes stays NaN): every output
    written, against float64 -- y / dx / dgamma / dbeta / d(scale | shift) at the bounds above, and the saved {mean, rstd} per (sample, group) at 1e-6
    (they are formed in float64 from the slot partials: what is left is the rounding of the partials and of the stored float)."""
    Bn, H, W, C_, G = shape
    HW = H * W
    x, gamma, beta, gy = _gn_inputs(f"abi.{shape}", shape)
    xn, gn = (t.permute(0, 2, 3, 1).contiguous() for t in (x, gy))                       # NHWC
    ss = U(f"abi.ss.{shape}", (Bn, 2 * C_), -0.5, 0.5).to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    st = _st()
    ws = nan(int(L.load().nd_groupnorm_silu_train_workspace_floats(Bn, HW, C_)))
    assert ws.numel() >= L.load().nd_groupnorm_train_workspace_floats(Bn, HW, C_)
    y, mr, dx, dg, db = nan(Bn, HW, C_), nan(Bn, G, 2), nan(Bn, HW, C_), nan(C_), nan(C_)
    L.call("nd_groupnorm_train_forward_f32", xn.data_ptr(), C_, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), C_, mr.data_ptr(), ws.data_ptr(),
           Bn, HW, C_, G, 1e-5, st)
    L.call("nd_groupnorm_train_backward_f32", gn.data_ptr(), C_, xn.data_ptr(), C_, gamma.data_ptr(), mr.data_ptr(), dx.data_ptr(), C_, dg.data_ptr(),
           db.data_ptr(), ws.data_ptr(), Bn, HW, C_, G, st)
    ys, mrs, mad, dxs, dgs, dbs, dss = nan(Bn, HW, C_), nan(Bn, G, 2), nan(Bn, 3, C_), nan(Bn, HW, C_), nan(C_), nan(C_), nan(Bn, 2 * C_)
    ws.fill_(float("nan"))
    L.call("nd_groupnorm_silu_train_forward_f32", xn.data_ptr(), C_, gamma.data_ptr(), beta.data_ptr(), ss.data_ptr(), None, 0, ys.data_ptr(), C_,
           mrs.data_ptr(), mad.data_ptr(), ws.data_ptr(), Bn, HW, C_, G, 1e-5, st)
    L.call("nd_groupnorm_silu_train_backward_f32", gn.data_ptr(), C_, xn.data_ptr(), C_, gamma.data_ptr(), beta.data_ptr(), ss.data_ptr(), mrs.data_ptr(),
           mad.data_ptr(), dxs.data_ptr(), C_, dgs.data_ptr(), dbs.data_ptr(), dss.data_ptr(), ws.data_ptr(), Bn, HW, C_, G, st)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in dict(y=y, mr=mr, dx=dx, dg=dg, db=db, ys=ys, mrs=mrs, dxs=dxs, dgs=dgs, dbs=dbs, dss=dss).items()}
    for k, v in got.items():
        assert not bool(v.isnan().any()), f"{k}: {int(v.isnan().sum())} elements not written"
    assert torch.equal(got["mr"], got["mrs"])                                              # one statistics pass for both operators
    x64 = x.double().cpu()
    grp = x64.reshape(Bn, G, -1)
    mean, var = grp.mean(dim=2), grp.var(dim=2, unbiased=False)
    assert rel_err(got["mr"][..., 0].numpy(), mean.numpy()) < 1e-6
    assert rel_err(got["mr"][..., 1].numpy(), (1.0 / torch.sqrt(var + 1e-5)).numpy()) < 1e-6
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(Bn, HW, C_)
    xd, wd, bd, sd = (t.double().cpu().requires_grad_() for t in (x, gamma, beta, ss))
    for silu in (False, True):
        n = F.group_norm(xd, G, wd, bd, 1e-5)
        yr = F.silu(n * (sd[:, :C_, None, None] + 1) + sd[:, C_:, None, None]) if silu else n
        grads = torch.autograd.grad(yr, (xd, wd, bd, sd) if silu else (xd, wd, bd), gy.double().cpu())
        names = ("ys", "dxs", "dgs", "dbs", "dss") if silu else ("y", "dx", "dg", "db")
        refs = (nhwc(yr.detach()), nhwc(grads[0])) + tuple(grads[1:])
        for name, ref in zip(names, refs):
            assert rel_err(got[name].numpy(), ref.numpy()) < (3e-5 if silu else 2e-5), (shape, name)


@pytest.mark.parametrize("case", [k[1:] for k in _of("token_sum") if k[2] >= 16384] + [(2, 65535, 48), (1, 16385, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_token_sum_at_the_step_shapes_matches_float64(case):
    """nd_token_sum_f32 (broadcast_add's gradient: gn_partials_kernel's sums, 256 slots from 16384 tokens on) on a NaN-filled output and workspace:
    against float64 at 2e-6, the same bits twice."""
    Bn, N, C_ = case
    x = U(f"ts.{case}", (Bn, N, C_)).to(DEV)
    ws = torch.full((int(L.load().nd_token_sum_workspace_floats(Bn, N, C_)),), float("nan"), device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((Bn, C_), float("nan"), device=DEV)
        L.call("nd_token_sum_f32", x.data_ptr(), C_, out.data_ptr(), ws.data_ptr(), Bn, N, C_, _st())
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and not bool(outs[0].isnan().any())
    assert rel_err(outs[0].numpy(), x.double().cpu().sum(dim=1).numpy()) < 2e-6


@pytest.mark.parametrize("case", [k[1:] for k in _of("modulate_silu")], ids=lambda s: "x".join(map(str, s)))
def test_modulate_silu_at_the_step_shapes_matches_float64(case):
    """train.modulate_silu (ResnetBlock2's per-pixel modulation + SiLU) at B = 4, 256 x 256: y, dn, d(scale | shift) against float64 at 2e-6; the same bits twice."""
    Bn, H, W, C_ = case
    n = U(f"ms.n.{case}", (Bn, C_, H, W), -2.0, 2.0).to(DEV).contiguous(memory_format=torch.channels_last)
    ss = U(f"ms.ss.{case}", (Bn, 2 * C_, H, W)).to(DEV).contiguous(memory_format=torch.channels_last)
    gy = U(f"ms.g.{case}", (Bn, C_, H, W)).to(DEV)
    outs = _runs(lambda a, s: train.modulate_silu(a, s), (n, ss, gy), fmts=(torch.channels_last, torch.channels_last))
    _same_bits(outs, "modulate_silu")
    nd, sd = n.double().cpu().requires_grad_(), ss.double().cpu().requires_grad_()
    y = F.silu(nd * (sd[:, :C_] + 1) + sd[:, C_:])
    y.backward(gy.double().cpu())
    for got, ref, name in zip(outs[0], (y, nd.grad, sd.grad), ("y", "dn", "dss")):
        assert rel_err(got.numpy(), ref.detach().numpy()) < 2e-6, (case, name)


@pytest.mark.parametrize("case", [k[1:] for k in _of("stem")], ids=lambda s: "x".join(map(str, s)))
def test_stem_weight_gradient_at_the_step_shapes_matches_float64(case):
    """train.conv7x7_c4 (init_conv) at B = 4, 256 x 256, cout = 64 / 48: the output, and the weight and bias gradient (nd_conv7x7_c4_wgrad_f32: sums over
    the B H W = 262144 pixels), against float64 at 2e-5 -- without the sqrt(B H W / 4096) growth tests/test_train_gpu.py allows this kernel against fp32
    PyTorch; the same bits twice."""
    Bn, H, W, cout = case
    assert int(L.load().nd_conv7x7_c4_wgrad_workspace_floats(Bn, H, W, cout)) >= 0         # (the kernel takes the shape: no unfolded-image fallback)
    x = U(f"stem.x.{case}", (Bn, 4, H, W), -1.5, 1.5).to(DEV)
    w, b = U(f"stem.w.{case}", (cout, 4, 7, 7), -0.1, 0.1).to(DEV), U(f"stem.b.{case}", (cout,)).to(DEV)
    gy = U(f"stem.gy.{case}", (Bn, cout, H, W)).to(DEV)
    outs = []
    for _ in range(2):
        wa, ba = w.clone().requires_grad_(), b.clone().requires_grad_()
        y = train.conv7x7_c4(x, wa, ba)
        y.backward(gy)
        outs.append([y.detach().cpu().contiguous(), wa.grad.cpu(), ba.grad.cpu()])
    _same_bits(outs, "stem")
    x64, g64 = x.double().cpu(), gy.double().cpu()
    y64 = F.conv2d(x64, w.double().cpu(), b.double().cpu(), padding=3)
    dw64 = torch.nn.grad.conv2d_weight(x64, w.shape, g64, padding=3)
    assert rel_err(outs[0][0].numpy(), y64.numpy()) < 2e-5
    assert rel_err(outs[0][1].numpy(), dw64.numpy()) < 2e-5
    assert rel_err(outs[0][2].numpy(), g64.sum(dim=(0, 2, 3)).numpy()) < 2e-5


# ====================================================================================================== 3. conv3x3
def _kernel(Bn, H, W, cin, cout, c0, c1):
    """What train._conv3x3_nhwc launches for this convolution: the kind and the split-K count of conv3x3_wino4."""
    kind = train.conv3x3_kind(Bn, H, W, cin, cout, c0, c1, cin)
    return kind, int(L.load().nd_conv3x3_wino4_splitk_plan(Bn, H, W, cin, cout)) if kind == "wino4" else 1


def _batch(H, W, cin, cout, c0, c1):
    """The smallest batch whose forward AND data-gradient launches are the step's (B = 4): the float64 references of the full-resolution cases on the
    CPU would otherwise take minutes.  The kernel does not depend on B beyond that choice."""
    for Bn in (1, 2, B):
        if _kernel(Bn, H, W, cin, cout, c0, c1) == _kernel(B, H, W, cin, cout, c0, c1) and _kernel(Bn, H, W, cout, cin, cout, 0) == _kernel(B, H, W, cout, cin, cout, 0):
            return Bn
    raise AssertionError("unreachable")


def _conv_case(k):
    """(H, W, c0, c1, cout) of a conv3x3 table entry (c1 = 0: one source)."""
    if k[0] == "conv3x3_cat_stats":
        return k[2], k[3], k[4], k[5], k[6]
    return k[2], k[3], k[4], 0, k[5]


def _check_kernel(k, Bn):
    H, W, c0, c1, cout = _conv_case(k)
    cin = c0 + c1
    fwd, dgrad = _kernel(B, H, W, cin, cout, c0, c1), _kernel(B, H, W, cout, cin, cout, 0)
    assert fwd[0] == "wino4" and dgrad[0] == "wino4", (k, fwd, dgrad)                 # every 3x3 convolution of the step: F(4x4, 3x3)
    if H == S:
        assert fwd[1] == 1 and dgrad[1] == 1, (k, fwd, dgrad)                          # full resolution: the plain kernel
    if H == S // 8:
        assert fwd[1] > 1 and dgrad[1] > 1, (k, fwd, dgrad)                            # H / 8: split-K
    assert _kernel(Bn, H, W, cin, cout, c0, c1) == fwd and _kernel(Bn, H, W, cout, cin, cout, 0) == dgrad


@pytest.mark.parametrize("k", _of("conv3x3"), ids=lambda k: "x".join(map(str, k[1:])))
def test_conv3x3_at_the_step_shapes_matches_float64(k):
    """train.conv3x3 at the step's plain 3x3 convolutions (the kernel asserted: conv3x3_kind and the split-K plan, at the test's batch as at B = 4):
    the output and the data gradient (the forward kernels on the dgrad packing) against float64 at the forward kernel's 5e-5, the weight and bias
    gradient (nd_conv3x3_wgrad_nhwc_f32) at 2e-5."""
    H, W, cin, _, cout = _conv_case(k)
    Bn = _batch(H, W, cin, cout, cin, 0)
    _check_kernel(k, Bn)
    x = U(f"c3.x.{k}", (Bn, cin, H, W), -1.5, 1.5).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (U(f"c3.w.{k}", (cout, cin, 3, 3)) / (9 * cin) ** 0.5).to(DEV)
    b = U(f"c3.b.{k}", (cout,)).to(DEV)
    gy = U(f"c3.gy.{k}", (Bn, cout, H, W)).to(DEV)
    xa, wa, ba = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = train.conv3x3(xa, wa, ba)
    y.backward(gy)
    xd, wd, bd = (t.double().cpu().requires_grad_() for t in (x, w, b))
    yd = F.conv2d(xd, wd, bd, padding=1)
    yd.backward(gy.double().cpu())
    for got, ref, tol, name in ((y, yd, 5e-5, "y"), (xa.grad, xd.grad, 5e-5, "dx"), (wa.grad, wd.grad, 2e-5, "dw"), (ba.grad, bd.grad, 2e-5, "db")):
        assert rel_err(got.detach().cpu().numpy(), ref.detach().numpy()) < tol, (k, Bn, name)


@pytest.mark.parametrize("k", _of("conv3x3_stats", "conv3x3_cat_stats"), ids=lambda k: k[0][8:] + "x".join(map(str, k[1:])))
def test_block_with_the_convs_statistics_at_the_step_shapes_matches_float64(k):
    """Block as the step runs it: conv3x3_with_stats / conv3x3_cat(with_stats=True) -> group_norm_silu(conv_stats=) with the time embedding's modulation and
    the shortcut (nd_groupnorm_finalize_train_f32 on the convolution's slots, the fused backward), against float64: the convolution's own output at 5e-5,
    the block's output at 1e-4 and every gradient at 2e-4 -- the bounds of test_block_with_the_convs_statistics_epilogue_matches_torch.  The kernel
    asserted as for the plain convolutions."""
    H, W, c0, c1, cout = _conv_case(k)
    cin = c0 + c1
    Bn = _batch(H, W, cin, cout, c0, c1)
    _check_kernel(k, Bn)
    G = 8
    tag = f"cs.{k}"
    x = U(tag + ".x", (Bn, cin, H, W), -1.5, 1.5).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (U(tag + ".w", (cout, cin, 3, 3)) / (9 * cin) ** 0.5).to(DEV)
    b = U(tag + ".b", (cout,)).to(DEV)
    gam, bet = U(tag + ".g", (cout,), 0.5, 1.5).to(DEV), U(tag + ".be", (cout,)).to(DEV)
    ss = U(tag + ".ss", (Bn, 2 * cout)).to(DEV)
    res = U(tag + ".r", (Bn, cout, H, W)).to(DEV)
    gy = U(tag + ".gy", (Bn, cout, H, W)).to(DEV)
    leaves = [x[:, :c0].contiguous(memory_format=torch.channels_last), x[:, c0:].contiguous(memory_format=torch.channels_last)] if c1 else [x]
    ts = [t.clone().requires_grad_() for t in leaves + [w, b, gam, bet, ss, res]]
    *xs, wa, ba, ga, bea, sa, ra = ts
    if c1:
        assert train.cat_sources_ok(xs[0], xs[1], cout)
        y, cs = train.conv3x3_cat(xs[0], xs[1], wa, ba, with_stats=True)
    else:
        y, cs = train.conv3x3_with_stats(xs[0], wa, ba)
    y.retain_grad()
    out = train.group_norm_silu(y, G, ga, bea, sa, 1e-5, res=ra, conv_stats=cs)
    out.backward(gy)
    td = [t.double().cpu().requires_grad_() for t in (x, w, b, gam, bet, ss, res)]
    yd = F.conv2d(td[0], td[1], td[2], padding=1)
    yd.retain_grad()
    ref = F.silu(F.group_norm(yd, G, td[3], td[4], 1e-5) * (td[5][:, :cout, None, None] + 1) + td[5][:, cout:, None, None]) + td[6]
    ref.backward(gy.double().cpu())
    assert rel_err(y.detach().cpu().numpy(), yd.detach().numpy()) < 5e-5, (k, "conv y")
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-4, (k, "y")
    dx = torch.cat([t.grad for t in xs], dim=1) if c1 else xs[0].grad
    for got, r, name in zip([dx, wa.grad, ba.grad, ga.grad, bea.grad, sa.grad, ra.grad, y.grad], [t.grad for t in td] + [yd.grad],
                            ("dx", "dw", "db", "dgamma", "dbeta", "dss", "dres", "dconv_out")):
        assert rel_err(got.cpu().numpy(), r.numpy()) < 2e-4, (k, name)


# ---------------------------------------------------------------------------------------------------------------- the questions and their entries

def test_the_norm_and_weight_gradient_questions_agree_with_their_entries():
    """nd_groupnorm_train_takes, nd_layernorm_train_takes, nd_rmsnorm_train_takes, nd_token_sum_takes and nd_conv3x3_wgrad_cat_takes against what their entries
    do, just inside and just outside each limit (one sample of 32 pixels; every pointer valid and aligned, so a refusal is a refusal of the shape).  An entry
    decides on the host before any launch: a shape its question refuses starts no kernel.  The answers are literals, not computed from the code."""
    lib, st = L.load(), _st()
    HW, CMAX = 32, 1028
    buf = lambda n: torch.zeros(n, device=DEV)
    x, y, g, dx = U("q.x", (HW * CMAX,)).to(DEV), buf(HW * CMAX), U("q.g", (HW * CMAX,)).to(DEV), buf(HW * CMAX)
    gamma, beta, dgam, dbet = U("q.gamma", (CMAX,)).to(DEV), U("q.beta", (CMAX,)).to(DEV), buf(CMAX), buf(CMAX)
    stats, mad = buf(2 * CMAX), buf(3 * CMAX)
    ws = buf(int(max(lib.nd_groupnorm_silu_train_workspace_floats(1, HW, CMAX), lib.nd_layernorm_train_workspace_floats(HW, CMAX),
                     lib.nd_rmsnorm_backward_workspace_floats(HW, CMAX), lib.nd_token_sum_workspace_floats(1, HW, CMAX))))
    p = lambda t: t.data_ptr()

    def agree(takes, want, entry, prefix, call):
        rc = call()
        msg = lib.nd_last_error().decode() if rc else ""
        assert rc <= 0, f"{entry}: HIP error {rc}: {msg}"
        assert bool(takes) == want == (rc == 0), f"{entry}: the question says {takes}, the entry returned {rc} '{msg}', expected {want}"
        assert rc == 0 or msg.startswith(prefix + ":"), msg

    for C_, G, want in ((64, 8, True), (1024, 2, True), (1024, 1, False), (1028, 4, False), (60, 8, False), (6, 2, False)):
        takes = lib.nd_groupnorm_train_takes(C_, G)
        agree(takes, want, "nd_groupnorm_train_forward_f32", "nd_groupnorm_train_forward",
              lambda: lib.nd_groupnorm_train_forward_f32(p(x), C_, p(gamma), p(beta), p(y), C_, p(stats), p(ws), 1, HW, C_, G, 1e-5, st))
        agree(takes, want, "nd_groupnorm_train_backward_f32", "nd_groupnorm_train_backward",
              lambda: lib.nd_groupnorm_train_backward_f32(p(g), C_, p(x), C_, p(gamma), p(stats), p(dx), C_, p(dgam), p(dbet), p(ws), 1, HW, C_, G, st))
        agree(takes, want, "nd_groupnorm_silu_train_forward_f32", "nd_groupnorm_silu_train_forward",
              lambda: lib.nd_groupnorm_silu_train_forward_f32(p(x), C_, p(gamma), p(beta), None, None, 0, p(y), C_, p(stats), p(mad), p(ws), 1, HW, C_, G, 1e-5, st))
        agree(takes, want, "nd_groupnorm_silu_train_backward_f32", "nd_groupnorm_silu_train_backward",
              lambda: lib.nd_groupnorm_silu_train_backward_f32(p(g), C_, p(x), C_, p(gamma), p(beta), None, p(stats), p(mad), p(dx), C_, p(dgam), p(dbet), None, p(ws),
                                                               1, HW, C_, G, st))
    for C_, want in ((16, True), (12, False), (1024, True), (1028, False), (18, False)):
        takes = lib.nd_layernorm_train_takes(C_)
        agree(takes, want, "nd_layernorm_train_forward_f32", "nd_layernorm_train_forward",
              lambda: lib.nd_layernorm_train_forward_f32(p(x), C_, p(gamma), p(beta), p(y), C_, p(stats), HW, C_, 1e-5, st))
        agree(takes, want, "nd_layernorm_train_backward_f32", "nd_layernorm_train_backward",
              lambda: lib.nd_layernorm_train_backward_f32(p(g), C_, p(x), C_, p(gamma), p(stats), p(dx), C_, p(dgam), p(dbet), p(ws), HW, C_, st))
    for C_, want in ((4, True), (1024, True), (1028, False), (6, False), (0, False)):
        agree(lib.nd_rmsnorm_train_takes(C_), want, "nd_rmsnorm_backward_f32", "nd_rmsnorm_backward",
              lambda: lib.nd_rmsnorm_backward_f32(p(g), C_, p(x), C_, p(gamma), p(dx), C_, p(dgam), p(ws), 1, HW, C_, st))
        agree(lib.nd_token_sum_takes(C_), want, "nd_token_sum_f32", "nd_token_sum", lambda: lib.nd_token_sum_f32(p(x), C_, p(y), p(ws), 1, HW, C_, st))
    # the two-source weight gradient: 4 x 16 pixels is one tile group of the Winograd-domain form, 9 x 11 and 6 x 16 are none; sources of whole 32-channel blocks
    dw, wsw = buf(64 * 64 * 9), buf(int(max(lib.nd_conv3x3_wgrad_workspace_floats(1, 9, 11, 64, 64), lib.nd_conv3x3_wgrad_workspace_floats(1, 4, 16, 64, 64),
                                         lib.nd_conv3x3_wgrad_workspace_floats(1, 4, 16, 64, 16))))
    for H, W, c0, c1, cout, want in ((4, 16, 32, 32, 16, True), (4, 16, 32, 32, 64, True), (4, 16, 16, 48, 16, False), (4, 16, 32, 16, 16, False), (9, 11, 32, 32, 16, False),
                                     (6, 16, 32, 32, 16, False), (4, 16, 32, 32, 8, False)):
        agree(lib.nd_conv3x3_wgrad_cat_takes(1, H, W, c0, c1, cout, c0, c1, cout), want, "nd_conv3x3_wgrad_cat_nhwc_f32", "nd_conv3x3_wgrad_cat_nhwc_f32",
              lambda: lib.nd_conv3x3_wgrad_cat_nhwc_f32(p(x), c0, c0, p(g), c1, c1, p(y), cout, p(dw), p(dbet), p(wsw), 1, H, W, cout, st))
    torch.cuda.synchronize()
