"""The scoring contract of noisediff_amd.metrics restated in float64 numpy ("Scoring the denoiser").

skimage is not a dependency: this is what ``peak_signal_noise_ratio`` and ``structural_similarity(channel_axis=2, data_range=R)`` compute
with their defaults (7 x 7 uniform window, cov_norm 49/48, K1 0.01, K2 0.03, the pad-3 border cropped), and what
``IlluminanceCorrect`` (test_denoising.py:232-263) computes, with every sum in float64."""
import numpy as np

K1, K2, WIN = 0.01, 0.03, 7


def clip(a, R=1.0):
    """tensor2im's clip, on fp32 values; np.clip keeps NaN."""
    return np.clip(np.asarray(a, dtype=np.float32), np.float32(0), np.float32(R))


def _box_means(a):
    """7 x 7 window means of an (H, W) float64 image at the interior centres: shape (H - 6, W - 6)."""
    H, W = a.shape
    h = a[:, 0:W - 6].copy()
    for i in range(1, WIN):
        h += a[:, i:W - 6 + i]
    v = h[0:H - 6].copy()
    for i in range(1, WIN):
        v += h[i:H - 6 + i]
    return v / 49.0


def ssim_map(x, y, R=1.0):
    """S at the interior pixels of one (H, W) channel pair (already clipped)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    cov_norm = 49.0 / 48.0
    ux, uy = _box_means(x), _box_means(y)
    uxx, uyy, uxy = _box_means(x * x), _box_means(y * y), _box_means(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim(x, y, R=1.0):
    """Mean over channels of the mean interior S; x, y: (C, H, W), clipped to [0, R] here."""
    x, y = clip(x, R), clip(y, R)
    if x.shape[-1] < WIN or x.shape[-2] < WIN:
        raise ValueError("H and W must be at least 7")
    return float(np.mean([ssim_map(x[c], y[c], R).mean() for c in range(x.shape[0])]))


def mse(x, y, R=1.0):
    x, y = clip(x, R), clip(y, R)
    d = x - y                                   # fp32
    return float(np.mean((d * d).astype(np.float64)))


def psnr(x, y, R=1.0):
    m = mse(x, y, R)
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(np.float64(R) ** 2 / np.float64(m)))


def illum_scale(pred, source):
    """num / den of one image in float64: p = clamp(pred, 0, 1), over the elements with source != 1."""
    p = clip(pred, 1.0).astype(np.float64).ravel()
    s = np.asarray(source, dtype=np.float32).astype(np.float64).ravel()
    m = s != 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(p[m] * s[m]) / np.sum(p[m] * p[m]))
