"""numpy restatement of the training step's two ends (noisediff_amd/csrc/diffusion_train.hip): the Philox counters of the timestep, offset and element
noise draws, the noising arithmetic one rounded fp32 operation at a time, and the weighted loss with its gradient in float64."""
import numpy as np

from oracle import noisediff_oracle as O

BLOCK_NOISE, BLOCK_OFFSET, BLOCK_T = 1, 2, 3


def philox(seed: int, index, sample, draw: int, block: int) -> np.ndarray:
    """The four words of counter {index, sample, draw, block} under key = the 64-bit seed, for arrays of index / sample (broadcast)."""
    index, sample = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    ctr = np.stack([index & 0xFFFFFFFF, sample & 0xFFFFFFFF, np.full(index.shape, draw & 0xFFFFFFFF, np.uint64), np.full(index.shape, block, np.uint64)],
                   -1).astype(np.uint32)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), index.shape + (2,))
    return O.philox4x32_10(ctr, key)


def draw_t_words(seed: int, samples, draw: int) -> np.ndarray:
    return philox(seed, np.zeros(len(samples), np.uint64), samples, draw, BLOCK_T)[..., 0]


def draw_t(seed: int, samples, draw: int, T: int) -> np.ndarray:
    """t = (w * T) >> 32 for word 0 of block 3."""
    return ((draw_t_words(seed, samples, draw).astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def draw_offset(seed: int, sample: int, draw: int, C: int) -> np.ndarray:
    """(C,) float64: channel c is component c & 3 of the block with index c >> 2."""
    return O.philox_normal4(philox(seed, np.arange(C // 4), np.full(C // 4, sample), draw, BLOCK_OFFSET)).reshape(C)


def draw_noise(seed: int, sample: int, draw: int, C: int, H: int, W: int) -> np.ndarray:
    """(C, H, W) float64: quad q of the sample's NHWC elements takes the four normals of the block with index q."""
    nq = H * W * C // 4
    return O.philox_normal4(philox(seed, np.arange(nq), np.full(nq, sample), draw, BLOCK_NOISE)).reshape(H, W, C).transpose(2, 0, 1)


def noising(x0, noise, offset, t, sqrt_ac, sqrt_1m_ac, objective: str, auto_normalize: bool = False, strength: float = 0.0):
    """(x_t, target) in fp32, every operation rounded on its own, in the reference's order."""
    f = np.float32
    x = np.asarray(x0, dtype=f)
    n = np.asarray(noise, dtype=f)
    if auto_normalize:
        x = (x * f(2)) - f(1)
    if strength > 0:
        n = n + (f(strength) * np.asarray(offset, dtype=f))[:, :, None, None]
    a = np.asarray(sqrt_ac, dtype=f)[np.asarray(t)][:, None, None, None]
    b = np.asarray(sqrt_1m_ac, dtype=f)[np.asarray(t)][:, None, None, None]
    x_t = (a * x) + (b * n)
    target = {"pred_noise": n, "pred_x0": x, "pred_v": (a * n) - (b * x)}[objective]
    assert x_t.dtype == f and target.dtype == f
    return x_t, target


def loss64(out, target, t, loss_weight, x0_term: bool = False):
    """(loss, sample_loss [B]) in float64 from the fp32 inputs."""
    o, g = np.asarray(out, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w = np.asarray(loss_weight, dtype=np.float64)[np.asarray(t)]
    sample = ((o - g) ** 2).reshape(o.shape[0], -1).mean(1) * w
    loss = sample.mean()
    if x0_term:
        loss = loss + np.abs(o.mean((2, 3)) - g.mean((2, 3))).mean()
    return loss, sample


def grad64(out, target, t, loss_weight, x0_term: bool = False, g: float = 1.0) -> np.ndarray:
    """d loss / d out times the upstream gradient g, float64."""
    o, tg = np.asarray(out, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B, C, H, W = o.shape
    n = B * C * H * W
    w = np.asarray(loss_weight, dtype=np.float64)[np.asarray(t)][:, None, None, None]
    grad = 2.0 * w / n * (o - tg)
    if x0_term:
        grad = grad + np.sign(o.mean((2, 3)) - tg.mean((2, 3)))[:, :, None, None] / n
    return g * grad
