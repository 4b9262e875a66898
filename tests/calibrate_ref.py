"""numpy restatement of noisediff_amd.calibrate (csrc/calibrate.hip), importing nothing of the package: the yardstick of tests/test_calibrate.py.

Integer quantities are Python integers (exact); the long floating-point sums are ``math.fsum`` (exact, rounded once), so where the two sides
differ this is the more accurate one.  Frames are uint16 ``(N, H2, W2)``; a packed frame is ``h x w = H2 / 2 x W2 / 2``; a frame's ``n = 4 h w``
values are ordered (channel, packed row, packed column) with the channels of ``raw``'s Bayer cell: (2Y, 2X), (2Y, 2X + 1), (2Y + 1, 2X + 1),
(2Y + 1, 2X).
"""
import math

import numpy as np

SITES = ((0, 0), (0, 1), (1, 1), (1, 0))                  # (row, column) of channel c inside the 2 x 2 cell


def pack(a):
    """(N, H2, W2) -> (N, 4, h, w), any dtype."""
    a = np.asarray(a)
    return np.stack([a[:, r::2, c::2] for r, c in SITES], axis=1)


def stack_sums(frames):
    """DarkStack.sums: int64 here, exact."""
    return np.asarray(frames).astype(np.int64).sum(axis=0)


def stack_mean(sums, count):
    return sums.astype(np.float64) / float(count)


def pixel_values(frames, black=512, subtract="black"):
    """t = D code - P as int64 (N, 4, h, w), and D."""
    f = np.asarray(frames).astype(np.int64)
    if subtract == "black":
        return pack(f - int(black)), 1
    N = f.shape[0]
    return pack(N * f - stack_sums(frames)[None]), N


def row_sums(frames, black=512, subtract="black"):
    """R[n, c, Y] = sum_X t, exact (int64 holds it: |t| < 2^31, w <= 2^15)."""
    t, _ = pixel_values(frames, black, subtract)
    return t.sum(axis=3)


def residuals(frames, black=512, subtract="black"):
    """x = (double)(t w - R) / (double)(w D): numerator and denominator exact, one IEEE division.  (N, n) float64."""
    t, D = pixel_values(frames, black, subtract)
    w = t.shape[3]
    num = t * w - t.sum(axis=3, keepdims=True)
    assert np.abs(num).max() < 2 ** 53
    return (num.astype(np.float64) / float(w * D)).reshape(t.shape[0], -1)


def row_stats(frames, black=512, subtract="black"):
    """Per frame: sigR_pmn, sigR, bias (4,), V_x, as the kernel defines them, from Python integers and fsum."""
    t, D = pixel_values(frames, black, subtract)
    N, _, h, w = t.shape
    R = t.sum(axis=3)
    x = residuals(frames, black, subtract)
    out = []
    for n in range(N):
        total, bias = 0, []
        for c in range(4):
            r = [int(v) for v in R[n, c]]
            S, Q = sum(r), sum(v * v for v in r)
            total += h * Q - S * S
            bias.append(float(S) / float(h * w * D))
        v = float(total) / float(4 * h * h) / float(w * D) / float(w * D)
        mean = math.fsum(x[n]) / x.shape[1]
        vx = math.fsum((x[n] - mean) ** 2) / x.shape[1]
        out.append({"sigR_pmn": math.sqrt(v), "sigR": math.sqrt(max(v - vx / (w - 1), 0.0)), "bias": np.array(bias), "V_x": vx})
    return out


def medians(n):
    """scipy.stats._morestats._calc_uniform_order_statistic_medians, statement by statement."""
    v = np.empty(n, dtype=np.float64)
    v[-1] = 0.5 ** (1.0 / n)
    v[0] = 1 - v[-1]
    i = np.arange(2, n)
    v[1:-1] = (i - 0.3175) / (n + 0.365)
    return v


def tukey_quantile(u, lam):
    """(expm1(lam log u) - expm1(lam log1p(-u))) / lam, and log u - log1p(-u) at lam == 0."""
    u, lam = np.asarray(u, np.float64), float(lam)
    a, b = np.log(u), np.log1p(-u)
    if lam == 0.0:
        return a - b
    return (np.expm1(lam * a) - np.expm1(lam * b)) / lam


def quantile_tolerance(u, lam):
    """The per-element bound on the Tukey-lambda quantile (test_physics_noise._quantile_tolerance, restated): log, log1p and expm1 are good to
    about an ulp and four more roundings follow; the difference of the two expm1 is taken between numbers no larger than max(1, e^(-lam log)),
    and the division by lam turns an error relative to lam log back into one relative to log: 64 ulp of
    max(1, |log u|, |log(1-u)|) e^max(0, -lam log)."""
    a = np.maximum(np.abs(np.log(u)), np.abs(np.log1p(-u)))
    return 64 * 2.0 ** -53 * np.maximum(1.0, a) * np.exp(np.maximum(0.0, -lam) * a)


def fit(xs, q):
    """(slope, intercept, r) of sorted xs on the quantiles q: scipy.stats.probplot's linregress and ppcc's pearsonr, every sum an fsum."""
    xs, q = np.asarray(xs, np.float64), np.asarray(q, np.float64)
    n = len(xs)
    xm, qm = math.fsum(xs) / n, math.fsum(q) / n
    dx, dq = xs - xm, q - qm
    cxx, cqq, cxq = math.fsum(dx * dx), math.fsum(dq * dq), math.fsum(dx * dq)
    slope = cxq / cqq
    with np.errstate(invalid="ignore", divide="ignore"):
        r = float(np.float64(cxq) / (np.sqrt(np.float64(cxx)) * np.sqrt(np.float64(cqq))))
    return slope, xm - slope * qm, max(min(r, 1.0), -1.0) if r == r else r


def probplot(xs, lam=None, normal_quantile=None):
    """One probability plot of sorted xs: Tukey-lambda of shape lam, or normal with ``normal_quantile`` (scipy.special.ndtri)."""
    m = medians(len(xs))
    return fit(xs, tukey_quantile(m, lam) if lam is not None else normal_quantile(m))


def objective(xs, lam):
    """1 - r(lam): what ppcc_max minimises."""
    return 1.0 - probplot(xs, lam)[2]
