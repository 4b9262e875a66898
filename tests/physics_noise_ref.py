"""Numpy restatement of noisediff_amd.physics_noise (csrc/physics_noise.hip): the contract of DESIGN.md section 22, one IEEE operation per line
in the order given there.  Philox, the uniforms, the float64 normal and the Poisson draw are raw_ref's and denoise_data_ref's.

Nothing here imports the package: it can be wrong only in its own way."""
import math

import numpy as np

import raw_ref as R
from denoise_data_ref import philox4x32_10

BLACK, WHITE = 512, 16383
READ_BLOCK, ROW_BLOCK = 32, 33
f32 = np.float32


def tukey_quantile(u, lam):
    """Q(u) of the unit Tukey-lambda variate, float64: a = log u; b = log1p(-u); lam != 0: (expm1(lam a) - expm1(lam b)) / lam; lam == 0: a - b."""
    u = np.asarray(u, np.float64)
    lam = np.float64(lam)
    a = np.log(u)
    b = np.log1p(-u)
    if lam == 0.0:
        return a - b
    p = lam * a
    q = lam * b
    ep = np.expm1(p)
    eq = np.expm1(q)
    d = ep - eq
    return d / lam


def tukey_variance(lam):
    """Variance of the unit Tukey-lambda variate: (2 / lam^2) (1 / (1 + 2 lam) - Gamma(lam + 1)^2 / Gamma(2 lam + 2)), lam > -1/2, lam != 0."""
    return 2.0 / lam ** 2 * (1.0 / (1.0 + 2.0 * lam) - math.gamma(lam + 1.0) ** 2 / math.gamma(2.0 * lam + 2.0))


def read64(kind, lam, seed, sample, draw, n):
    """The unit read variates of elements 0 .. n-1 in float64: kind 0 is raw_ref.normal64 (words 0 and 1 of block 32), kind 1 the quantile of word 2."""
    if kind == 0:
        return R.normal64(seed, sample, draw, n)
    return tukey_quantile(R.uniforms(seed, sample, draw, n, READ_BLOCK)[:, 2], lam)


def quant(seed, sample, draw, n):
    """uq = (float)(u3 - 0.5), word 3 of block 32."""
    return (R.uniforms(seed, sample, draw, n, READ_BLOCK)[:, 3] - 0.5).astype(f32)


def row64(seed, row_stream, draw, Y, C=4):
    """The unit row variates of absolute rows ``Y`` in float64, (C, len(Y)): Box-Muller on words 0 and 1 of counter {4 Y + c, row_stream, draw, 33}."""
    Y = np.asarray(Y, np.int64).reshape(-1)
    idx = (4 * Y[None, :] + np.arange(C)[:, None]).reshape(-1)
    c = np.stack([idx.astype(np.uint32), np.full(idx.size, row_stream & 0xFFFFFFFF, np.uint32), np.full(idx.size, draw, np.uint32),
                  np.full(idx.size, ROW_BLOCK, np.uint32)], -1)
    k = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), (idx.size, 2))
    u = (philox4x32_10(c, k).astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos((2.0 * np.pi) * u[:, 1])
    return z.reshape(C, Y.size)


def source_rows(y0, h, flip):
    """Absolute packed row of output rows 0 .. h-1."""
    y = np.arange(h)
    return y0 + (h - 1 - y if flip else y)


def rate(x, ratio, K, black=BLACK):
    """(c0, lamP): c0 = max(x - black, 0) in fp32, lamP = (double)(c0 / (float)ratio) / K."""
    return R.pg_rate(x, ratio, K, black)


def clean(x, black=BLACK, white=WHITE):
    return R.pg_clean(x, black, white)


def signal(counts, reads, rows, quants, p):
    """t before the sensor clip, float64: t = K n; t += s_read r; t += s_row g; t += qstep uq; t += bias.  counts, reads, quants (4, h, w), rows (4, h);
    the variates are widened from whatever type they come in."""
    w = lambda a: np.asarray(a).astype(np.float64)          # noqa: E731
    t = np.float64(p["K"]) * w(counts)
    pr = np.float64(p["s_read"]) * w(reads)
    t = t + pr
    pg = np.float64(p["s_row"]) * w(rows)[..., None]
    t = t + pg
    pq = np.float64(p["qstep"]) * w(quants)
    t = t + pq
    return t + np.float64(p["bias"])


def noisy(counts, reads, rows, quants, p, ratio, clip01=True, black=BLACK, white=WHITE):
    """noisy (fp32) from the four variate arrays; p: K, s_read, s_row, qstep, bias.  Float64 throughout."""
    wb = np.float64(f32(white) - f32(black))
    lo = -np.float64(f32(black))
    t = np.clip(signal(counts, reads, rows, quants, p), lo, wb)
    v = t * np.float64(ratio)
    v = v / wb
    if clip01:
        v = np.clip(v, 0.0, 1.0)
    return v.astype(f32)


def noise(noisy_, clean_):
    return np.asarray(noisy_, f32) - np.asarray(clean_, f32)
