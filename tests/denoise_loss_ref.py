"""numpy restatement of the denoiser's training loss (noisediff_amd/csrc/denoise_loss.hip): d as a float32 subtraction, everything after it in float64,
rounded to float32 once -- and the trainer's learning-rate loop replayed literally (models/trainer_denoising.py:184-188)."""
import numpy as np


def diff(out, target) -> np.ndarray:
    """d = fl32(out - target), widened to float64."""
    d = np.asarray(out, dtype=np.float32) - np.asarray(target, dtype=np.float32)
    assert d.dtype == np.float32
    return d.astype(np.float64)


def loss(out, target, l1: float, mse: float):
    """(terms [3] = {loss, mean |d|, mean d^2}, sample terms [B, 2]) as float32, from sums in float64."""
    d = diff(out, target)
    B = d.shape[0]
    n = d.size // B
    s1, s2 = np.abs(d).reshape(B, -1).sum(1), (d * d).reshape(B, -1).sum(1)
    m1, m2 = s1.sum() / d.size, s2.sum() / d.size
    terms = np.array([mse * m2 + l1 * m1, m1, m2], dtype=np.float64)
    return terms.astype(np.float32), np.stack([s1 / n, s2 / n], 1).astype(np.float32)


def grad(out, target, l1: float, mse: float, g: float = 1.0) -> np.ndarray:
    """d loss / d out times the upstream gradient g (a float32 value), formed in float64 and rounded to float32 once; sign(0) = 0."""
    d = diff(out, target)
    g = float(np.float32(g))
    return (g * l1 / d.size * np.sign(d) + g * 2.0 * mse / d.size * d).astype(np.float32)


def l1_grad_exact(out, target, g: float = 1.0) -> np.ndarray:
    """The pure L1 gradient: float32(g / N) * sign(d), what ATen's l1_loss gives."""
    d = diff(out, target)
    return np.float32(float(np.float32(g)) / d.size) * np.sign(d).astype(np.float32)


def within_one_ulp(got, ref) -> bool:
    """|got - ref| <= 2^-23 |ref| for every element (both float32): they are equal or neighbours."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref)))


def trainer_lrs(max_iter: int, base_lr: float) -> list:
    """The learning rate of every epoch as the trainer's loop leaves it in param_groups[0]['lr']."""
    lr, out = base_lr, []
    for i in range(0, max_iter):
        if i > max_iter // 2:
            lr = base_lr / 2.
        if i > int(max_iter * 0.8):
            lr = 1e-5
        out.append(lr)
    return out
