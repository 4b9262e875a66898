"""Numpy restatement of noisediff_amd.render (csrc/develop.hip): LibRaw's develop steps as DESIGN.md section 20 lists them -- integers, except the
scaling multiply and the colour matrix, which are float32 with one rounding per operation in the written order, and the tone curve, which is
float64.  It is the yardstick of the device kernel (bitwise); it was NOT compared with LibRaw, which is not a dependency of this project.
Nothing here imports the package: it can be wrong only in its own way."""
import numpy as np

from raw_ref import to_bayer

f32 = np.float32


def gamma_params(power, slope):
    """(g2, g3, g4) of dcraw's gamma_curve: g2 by 48 bisection steps on bnd, g3 = g2 / slope, g4 = g2 (1 / power - 1)."""
    g0, g1 = np.float64(power), np.float64(slope)
    g2 = g3 = g4 = np.float64(0)
    bnd = [np.float64(0), np.float64(0)]
    bnd[int(g1 >= 1)] = np.float64(1)
    if g1 != 0 and (g1 - 1) * (g0 - 1) <= 0:
        for _ in range(48):
            g2 = (bnd[0] + bnd[1]) / 2
            bnd[int(((g2 / g1) ** -g0 - 1) / g0 - 1 / g2 > -1)] = g2
        g3 = g2 / g1
        g4 = g2 * (1 / g0 - 1)
    return float(g2), float(g3), float(g4)


def gamma_curve(power=0.45, slope=4.5, imax=65536):
    """uint16[65536]: 65535 where r = i / imax >= 1, else trunc(65536 (r < g3 ? r slope : r^power (1 + g4) - g4))."""
    _, g3, g4 = gamma_params(power, slope)
    r = np.arange(65536, dtype=np.float64) / np.float64(imax)
    toe = r * np.float64(slope)
    knee = np.power(r, np.float64(power)) * (1 + g4) - g4
    v = np.float64(65536) * np.where(r < g3, toe, knee)
    out = np.full(65536, 65535, np.int64)
    out[r < 1] = v[r < 1].astype(np.int64)
    assert out.min() >= 0 and out.max() <= 65535
    return out.astype(np.uint16)


def scale_mul(cam_mul, maximum):
    """pre = cam_mul as fp32, pre[3] = pre[1] when cam_mul[3] == 0, pre = fl32(pre / min(pre)); fl32((double)pre * 65535.0 / maximum)."""
    pre = np.array(cam_mul, dtype=f32)
    if cam_mul[3] == 0:
        pre[3] = pre[1]
    pre = (pre / pre.min()).astype(f32)
    return (pre.astype(np.float64) * np.float64(65535.0) / np.float64(maximum)).astype(f32)


def channel_of_site(H2, W2):
    """(2H, 2W) int: the package's channel at each mosaic site: 0 = R (2Y, 2X), 1 = G1 (2Y, 2X+1), 2 = B (2Y+1, 2X+1), 3 = G2 (2Y+1, 2X)."""
    c = np.zeros((H2, W2), np.int64)
    c[0::2, 1::2], c[1::2, 1::2], c[1::2, 0::2] = 1, 2, 3
    return c


def scaled(mosaic, black, mul):
    """(2H, 2W) uint16 codes -> s per site (int64): v = max(x - black[c], 0); s = min(trunc(fl32(v) * scale_mul[c]), 65535)."""
    mosaic = np.asarray(mosaic)
    assert mosaic.dtype == np.uint16
    c = channel_of_site(*mosaic.shape)
    v = np.maximum(mosaic.astype(np.int64) - np.asarray(black, np.int64)[c], 0)
    p = v.astype(f32) * np.asarray(mul, f32)[c]
    assert p.dtype == f32
    return np.minimum(p.astype(np.int64), 65535)


def half(s):
    """(2H, 2W) -> (H, W, 3): R = s0, G = (s1 + s3) >> 1, B = s2."""
    return np.stack([s[0::2, 0::2], (s[0::2, 1::2] + s[1::2, 0::2]) >> 1, s[1::2, 1::2]], -1)


COLOUR = np.array([0, 1, 2, 1])       # channel -> R, G, B: both greens count as G


def _window_sum(a):
    """Sum over the 3 x 3 window around every site; sites outside the frame add nothing."""
    p = np.pad(a, 1)
    H2, W2 = a.shape
    return sum(p[dy:dy + H2, dx:dx + W2] for dy in range(3) for dx in range(3))


def full(s):
    """(2H, 2W) -> (2H, 2W, 3), the general rule: a site keeps its own colour; each other colour is floor(sum / count) over the sites of that
    colour inside the 3 x 3 window around it that lie inside the frame."""
    colour = COLOUR[channel_of_site(*s.shape)]
    out = np.zeros(s.shape + (3,), np.int64)
    for k in range(3):
        has = (colour == k).astype(np.int64)
        total, count = _window_sum(s * has), _window_sum(has)
        assert (count[colour != k] >= 1).all()
        out[..., k] = np.where(colour == k, s, total // np.maximum(count, 1))
    return out


def full_interior(s):
    """The closed forms of the interior, sites (1 .. 2H-2, 1 .. 2W-2): (a + b) >> 1 at green sites, (a + b + c + d) >> 2 at red and blue sites."""
    c = channel_of_site(*s.shape)[1:-1, 1:-1]
    m = s[1:-1, 1:-1]
    up, dn, lf, rt = s[:-2, 1:-1], s[2:, 1:-1], s[1:-1, :-2], s[1:-1, 2:]
    cross = (up + dn + lf + rt) >> 2
    diag = (s[:-2, :-2] + s[:-2, 2:] + s[2:, :-2] + s[2:, 2:]) >> 2
    rows, cols = (up + dn) >> 1, (lf + rt) >> 1
    R = np.select([c == 0, c == 1, c == 2, c == 3], [m, cols, diag, rows])
    G = np.select([c == 0, c == 2], [cross, cross], m)
    B = np.select([c == 0, c == 1, c == 2, c == 3], [diag, rows, m, cols])
    return np.stack([R, G, B], -1)


def mix(rgb, m):
    """(..., 3) integers -> (..., 3) float32 sums: o = 0 + R m[k][0]; o = o + G m[k][1]; o = o + B m[k][2], each product rounded, then added."""
    m = np.asarray(m, f32).reshape(3, 3)
    R, G, B = (rgb[..., i].astype(f32) for i in range(3))
    out = []
    for k in range(3):
        o = f32(0) + R * m[k, 0]
        o = o + G * m[k, 1]
        o = o + B * m[k, 2]
        assert o.dtype == f32
        out.append(o)
    return np.stack(out, -1)


def tone(o, curve, bps):
    """u = clip((int)o, 0, 65535), the cast truncating toward zero; curve[u] >> 8 as uint8, or curve[u] as uint16."""
    u = np.clip(np.trunc(o.astype(np.float64)).astype(np.int64), 0, 65535)
    t = np.asarray(curve, np.uint16)[u]
    return (t >> 8).astype(np.uint8) if bps == 8 else t


def mosaic_of(src, black, white):
    """A (4, H, W) fp32 image as its codes (raw.to_bayer's rule), a (2H, 2W) uint16 mosaic as it is."""
    src = np.asarray(src)
    return to_bayer(src, black, white) if src.dtype == f32 else src


def develop(src, black, white, mul, rgb_cam, curve, bps=8, full_res=False, window=None, sums=None):
    """One image.  window = (x0, y0, h, w) in packed pixels: the crop of the WHOLE frame's picture.  sums: a list that receives the float32 sums."""
    s = scaled(mosaic_of(src, black, white), black, mul)
    o = mix(full(s) if full_res else half(s), rgb_cam)
    if sums is not None:
        sums.append(o)
    out = tone(o, curve, bps)
    if window is not None:
        k = 2 if full_res else 1
        x0, y0, h, w = window
        out = out[k * y0:k * (y0 + h), k * x0:k * (x0 + w)]
    return out
