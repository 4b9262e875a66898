"""The numpy / torch restatement the noise-statistics kernels are tested against (utils/util.py:185-255, utils/raw_util.py:161-189).

Bins by ``np.searchsorted`` on the float64 edges, float64 for everything else.  The KL functions are the reference's expressions, so they equal
the goldens bit for bit; ``kl_terms`` also hands out the summed terms, from which the tests take their a-priori bound."""
import numpy as np
import torch
import torch.nn.functional as F


def kld_edges():
    bw = 0.2 / 64
    return np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, bw), [1000.0]), axis=0)


def default_edges(left_edge=0.0, right_edge=1.0, n_bins=1000):
    bin_width = (right_edge - left_edge) / n_bins
    return np.arange(left_edge, right_edge + bin_width, bin_width)


def counts(data, edges):
    """np.histogram(data, edges)[0] spelled out: v is in bin i when edges[i] <= v < edges[i + 1] in float64, the last bin also takes the last
    edge; NaN and everything outside the edges is dropped."""
    v = np.asarray(data).reshape(-1).astype(np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n_bins = edges.size - 1
    v = v[(v >= edges[0]) & (v <= edges[-1])]                   # NaN fails both
    idx = np.searchsorted(edges, v, side="right") - 1
    idx[idx == n_bins] = n_bins - 1                             # v == edges[-1]
    return np.bincount(idx, minlength=n_bins).astype(np.int64)


def get_histogram(data, bin_edges=None, left_edge=0.0, right_edge=1.0, n_bins=1000):
    bin_width = (right_edge - left_edge) / n_bins
    if bin_edges is None:
        bin_edges = default_edges(left_edge, right_edge, n_bins)
    return counts(data, bin_edges) / np.prod(np.asarray(data).shape), bin_edges[:-1] + (bin_width / 2.0)


def _overlap(p, q):
    idx = ~(np.isnan(p) | np.isinf(p) | np.isnan(q) | np.isinf(q))
    p, q = p[idx], q[idx]
    idx = (p > 0) & (q > 0)
    return p[idx], q[idx]


def kl_div_forward(p, q):
    p, q = _overlap(p, q)
    return np.sum(p * np.log(p / q))


def kl_div_inverse(p, q):
    p, q = _overlap(p, q)
    return np.sum(q * np.log(q / p))


def kl_div_3(p, q):
    kl_fwd, kl_inv = kl_div_forward(p, q), kl_div_inverse(p, q)
    return kl_fwd, kl_inv, (kl_inv + kl_fwd) / 2.0


def kl_terms(p, q):
    """(forward terms, inverse terms): what kl_div_forward and kl_div_inverse sum."""
    p, q = _overlap(p, q)
    return p * np.log(p / q), q * np.log(q / p)


def kl_bound(p, q):
    """|got - ref| <= (n_bins + 8) 2^-53 sum |t_i| for the forward and the inverse value and (their mean) for the symmetric one: n_bins terms
    that each carry a few ulp of log and division error, summed in any order."""
    tf, ti = kl_terms(p, q)
    k = (len(p) + 8) * 2.0 ** -53
    bf, bi = k * np.abs(tf).sum(), k * np.abs(ti).sum()
    return np.array([bf, bi, (bf + bi) / 2.0])               # the symmetric value's terms are both lists, halved


def patch_std_mean(x, dtype=torch.float64):
    """sliding_window + torch.std_mean(dim=2) in ``dtype`` on the CPU: (std, mean), each (B, C, H, W)."""
    x = torch.as_tensor(x).to(dtype)
    B, C, H, W = x.shape
    patch = F.unfold(x, kernel_size=(3, 3), padding=1, stride=1, dilation=1).view(B, C, 9, -1)
    std, mean = torch.std_mean(patch, dim=2)
    return std.view(B, C, H, W), mean.view(B, C, H, W)


def line_fit(mean, std):
    """Least-squares slope and intercept of std on mean per (sample, channel) in float64, closed form: (B, C) each."""
    m = np.asarray(mean, dtype=np.float64).reshape(mean.shape[0], mean.shape[1], -1)
    s = np.asarray(std, dtype=np.float64).reshape(m.shape)
    N = m.shape[-1]
    sm, ss, smm, sms = m.sum(-1), s.sum(-1), (m * m).sum(-1), (m * s).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = N * smm - sm * sm
        slope = np.where(den == 0, np.nan, (N * sms - sm * ss) / den)
        return slope, (ss - slope * sm) / N


def ramp_image(seed, shape):
    """The fit's test input: a column ramp 0.02 .. 0.9 plus Gaussian noise of variance 0.01 ramp + 1e-4, so the window means spread."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.02, 0.9, W).view(1, 1, 1, W).expand(B, C, H, W)
    return (ramp + torch.randn(shape, generator=g) * (0.01 * ramp + 1e-4).sqrt()).to(torch.float32).contiguous()
