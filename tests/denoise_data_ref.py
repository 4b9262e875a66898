"""Numpy restatement of noisediff_amd.denoise_data (csrc/denoise_batch.hip): the stages of the training batch, one IEEE operation per line in
the order DESIGN.md section 11 gives, in a dtype of the caller's choice, and the Philox-Poisson draw in float64.

Run in float32 the stages repeat the reference's own numpy / torch operations and must equal its goldens bit for bit; run in float64 they are
the yardstick of the device kernel.  Nothing here imports the package: it can be wrong only in its own way."""
import math

import numpy as np

from oracle.noisediff_oracle import philox4x32_10

try:
    from scipy.special import gammaln
except ImportError:      # pragma: no cover
    gammaln = np.vectorize(math.lgamma, otypes=[np.float64])

WB = 15871               # white point 16383 - black level 512
INV_MAX = 200            # steps of the inversion search
MAX_ATTEMPTS = 64        # rejection attempts


def clip(a, lo, hi):
    """np.clip: NaN passes through."""
    return np.clip(a, lo, hi)


def compose(noise, clean, dtype):
    """(v, g) = (clip(clip(noise, -1, 1) + clean, 0, 1), clip(clean, 0, 1))."""
    noise, clean = np.asarray(noise, dtype), np.asarray(clean, dtype)
    return clip(clip(noise, -1, 1) + clean, 0, 1), clip(clean, 0, 1)


def pack_planes(bayer):
    """(2H, 2W) Bayer map -> (4, H, W) planes: channel c of packed pixel (Y, X) is Bayer (2Y + (c >= 2), 2X + (c == 1 or c == 2))."""
    return np.stack([bayer[0::2, 0::2], bayer[0::2, 1::2], bayer[1::2, 1::2], bayer[1::2, 0::2]])


def remove_dark_shading(v, ratio, iso, dk, db, blc, dtype):
    """v: (4, h, w) composed patch; dk, db: the (4, h, w) windows of the shading planes under it; one operation per line."""
    t = dtype
    v, dk, db = np.asarray(v, t), np.asarray(dk, t), np.asarray(db, t)
    ratio, iso, blc = t(ratio), t(iso), t(blc)
    im = v / ratio
    im = im * t(WB)
    im = im + t(512)
    im = clip(im, 0, 16383)
    dark = dk * iso
    dark = dark + db
    dark = dark + blc
    im = im - dark
    im = im - t(512)
    im = np.maximum(im, 0)
    im = im / t(WB)
    im = im * ratio
    return clip(im, 0, 1)


def sna_rate(g32, ratio, wb_c, K):
    """lam in float64 from the fp32 inputs: ((g * 15871 / ratio) * wb) / K, left to right."""
    g = np.asarray(g32, np.float32).astype(np.float64)
    return g * 15871.0 / np.float64(np.float32(ratio)) * np.asarray(wb_c, np.float32).astype(np.float64) / np.float64(np.float32(K))


def sna_terms(g, counts, ratio, wb_c, K, dtype):
    """(dn, dy) of the shot-noise augmentation; wb_c broadcasts against g ((4, 1, 1) for a (4, h, w) sample)."""
    t = dtype
    g, counts = np.asarray(g, t), np.asarray(counts, t)
    ratio, K, wb_c = t(np.float32(ratio)), t(np.float32(K)), np.asarray(np.asarray(wb_c, np.float32), t)
    gt = g * t(WB)
    gt = gt / ratio
    dy = gt * wb_c
    dn = counts * K
    dy = dy * ratio
    dy = dy / t(WB)
    dn = dn / t(WB)
    dn = dn * ratio
    return dn, dy


def window(a, cx, cy, h, w, flip):
    """The crop at even offset (cx, cy), rows reversed when flip: out[:, y, x] = a[:, cy + (h-1-y if flip else y), cx + x]."""
    out = a[..., cy:cy + h, cx:cx + w]
    return out[..., ::-1, :] if flip else out


def build_sample(noise, clean, x0, y0, cx, cy, flip, iso, ratio, h, w, planes=None, blc_mean=None, wb=None, K=None, counts=None, dtype=np.float64):
    """One sample of the batch: (noisy, clean_out), each (4, h, w) in ``dtype``.  planes: {"k_high", "b_high", "k_low", "b_low"} -> (4, H, W)
    or None; wb: 4 gains or None (an all-zero row: no augmentation); counts: (4, h, w) Poisson counts (needed when the augmentation is on)."""
    P = noise.shape[-1]
    v, g = compose(window(noise, cx, cy, h, w, flip), window(clean, cx, cy, h, w, flip), dtype)
    if planes is not None:
        pair = "high" if iso > 1600 else "low"
        dk = window(planes["k_" + pair][:, y0:y0 + P, x0:x0 + P], cx, cy, h, w, flip)
        db = window(planes["b_" + pair][:, y0:y0 + P, x0:x0 + P], cx, cy, h, w, flip)
        v = remove_dark_shading(v, ratio, iso, dk, db, blc_mean[iso], dtype)
    if wb is not None and np.abs(np.asarray(wb)).max() != 0:
        dn, dy = sna_terms(g, counts, ratio, np.asarray(wb, np.float32).reshape(4, 1, 1), K, dtype)
        v, g = v + dn, g + dy
    return v, g


def sample_rates(clean, cx, cy, flip, ratio, h, w, wb, K):
    """The float64 Poisson rates of one sample, (4, h, w), or None when its gains are all zero."""
    if wb is None or np.abs(np.asarray(wb)).max() == 0:
        return None
    g = clip(window(np.asarray(clean, np.float32), cx, cy, h, w, flip), 0, 1)
    return sna_rate(g, ratio, np.asarray(wb, np.float32).reshape(4, 1, 1), K)


# ----------------------------------------------------------------------------- the Philox-Poisson draw

def _uniforms(seed, sample, draw, elem, block):
    c = np.stack([elem.astype(np.uint32), np.full(elem.shape, sample & 0xFFFFFFFF, np.uint32), np.full(elem.shape, draw, np.uint32),
                  block.astype(np.uint32)], -1)
    k = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), c.shape[:-1] + (2,))
    return (philox4x32_10(c, k).astype(np.float64) + 0.5) * 2.0 ** -32


def poisson(lam, seed, sample, draw, eps=0.0, return_tries=False):
    """Poisson(lam[i]) for element index i of sample ``sample``: float64 counts, the device's decisions restated.

    lam == 0: 0; 0 < lam < 10: inversion on word 0 of block 0; lam >= 10: Hoermann's PTRS, attempt t on words 2 (t % 2), 2 (t % 2) + 1 of block
    t // 2; negative, NaN or infinite: NaN.  eps perturbs exp and lgamma relatively: how many decisions hang on the last bits of libm."""
    lam = np.asarray(lam, np.float64).reshape(-1)
    n = lam.size
    elem = np.arange(n, dtype=np.uint32)
    out = np.full(n, np.nan)
    tries = np.zeros(n)
    out[lam == 0] = 0.0
    with np.errstate(all="ignore"):
        idx = np.nonzero((lam > 0) & (lam < 10))[0]
        if idx.size:
            l = lam[idx]
            u = _uniforms(seed, sample, draw, elem[idx], np.zeros(idx.size, np.uint32))[:, 0]
            p = np.exp(-l) * (1 + eps)
            s = p.copy()
            k = np.zeros(idx.size)
            act = (u > s) & (k < INV_MAX)
            while act.any():
                k[act] += 1
                p[act] *= l[act] / k[act]
                s[act] += p[act]
                act = act & (u > s) & (k < INV_MAX)
            out[idx] = k
        idx = np.nonzero((lam >= 10) & np.isfinite(lam))[0]
        l = lam[idx]
        sl, ll = np.sqrt(l), np.log(l)
        b = 0.931 + 2.53 * sl
        a = -0.059 + 0.02483 * b
        lia = np.log(1.1239 + 1.1328 / (b - 3.4))
        vr = 0.9277 - 3.6224 / (b - 2.0)
        res = np.full(idx.size, np.nan)
        pend = np.arange(idx.size)
        for t in range(MAX_ATTEMPTS):
            if not pend.size:
                break
            U4 = _uniforms(seed, sample, draw, elem[idx[pend]], np.full(pend.size, t // 2, np.uint32))
            U = U4[:, 2 * (t % 2)] - 0.5
            V = U4[:, 2 * (t % 2) + 1]
            us = 0.5 - np.abs(U)
            k = np.floor((2.0 * a[pend] / us + b[pend]) * U + l[pend] + 0.43)
            fast = (us >= 0.07) & (V <= vr[pend])
            rej = (k < 0) | ((us < 0.013) & (V > us))
            lhs = np.log(V) + lia[pend] - np.log(a[pend] / (us * us) + b[pend])
            rhs = -l[pend] + k * ll[pend] - gammaln(k + 1.0) * (1 + eps)
            acc = fast | (~rej & (lhs <= rhs))
            res[pend[acc]] = k[acc]
            tries[idx[pend]] += 1
            pend = pend[~acc]
        out[idx] = res
    return (out, tries) if return_tries else out


def poisson_stats(x, lam):
    """z-scores of a sample of Poisson(lam) draws: (mean, variance, chi-square against the pmf over bins of expected count >= 32, dof)."""
    x = np.asarray(x, np.float64)
    N = x.size
    zm = (x.mean() - lam) / math.sqrt(lam / N)
    zv = (x.var() - lam) / math.sqrt((lam + 2 * lam * lam) / N)          # variance of the sample variance: (mu4 - sigma^4) / N
    ks = np.arange(0, int(lam + 12 * math.sqrt(lam) + 30))
    pmf = np.exp(-lam + ks * math.log(lam) - gammaln(ks + 1.0))
    cnt = np.bincount(np.minimum(x.astype(np.int64), ks[-1]), minlength=ks.size).astype(np.float64)
    exp = pmf * N
    exp[-1] += N - exp.sum()
    E, Cn, ce, cc = [], [], 0.0, 0.0
    for e, c_ in zip(exp, cnt):
        ce += e
        cc += c_
        if ce >= 32:
            E.append(ce)
            Cn.append(cc)
            ce = cc = 0.0
    if ce > 0:
        E[-1] += ce
        Cn[-1] += cc
    E, Cn = np.array(E), np.array(Cn)
    dof = E.size - 1
    chi = ((Cn - E) ** 2 / E).sum()
    zc = (chi - dof) / math.sqrt(2 * dof) if dof > 0 else 0.0
    return zm, zv, zc, dof
