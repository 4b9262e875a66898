"""Numpy restatement of noisediff_amd.frame (csrc/frame.hip): the layout of a frame's patches and the three outputs of nd_frame_assemble, one IEEE
operation per line in the order of DESIGN.md section 21 -- float32 through np.float32 values for noise and noisy, float64 for the short exposure.

Nothing here imports the package: it can be wrong only in its own way."""
import numpy as np

from raw_ref import codes

BLACK, WHITE = 512, 16383
f32 = np.float32


def patch_grid(crop, w, h):
    """dataloader/dataset.py:203-219: stride crop - crop // 4, a last patch flush with the border (it can repeat the one before)."""
    step = crop - crop // 4
    ys = list(range(0, h - crop + 1, step))
    if h - (ys[-1] + crop) < crop:
        ys.append(h - crop)
    xs = list(range(0, w - crop + 1, step))
    if w - (xs[-1] + crop) < crop:
        xs.append(w - crop)
    return [(x, y) for y in ys for x in xs]


def seams(origins, crop, length):
    s = [0]
    for a, b in zip(origins[:-1], origins[1:]):
        s.append((a + crop + b) // 2)              # the middle of the overlap [b, a + crop)
    return s + [length]


def layout(crop, H, W):
    """(xs, ys, sx, sy, patches, rects): unique sorted origins, seams, (x, y) origins row-major with ys outer, and (ax0, ay0, ax1, ay1) per patch."""
    grid = patch_grid(crop, W, H)
    xs, ys = sorted(set(x for x, _ in grid)), sorted(set(y for _, y in grid))
    sx, sy = seams(xs, crop, W), seams(ys, crop, H)
    patches = [(x, y) for y in ys for x in xs]
    rects = [(sx[i], sy[j], sx[i + 1], sy[j + 1]) for j in range(len(ys)) for i in range(len(xs))]
    return xs, ys, sx, sy, patches, rects


def clip(v, lo, hi):
    """By comparisons, as the kernel: a NaN passes through, a zero keeps its sign."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def clean(long_frame, black=BLACK, white=WHITE):
    """(2H, 2W) uint16 -> (4, H, W): max(x' - black, 0) / (white - black), not clipped."""
    g = codes(long_frame) - f32(black)
    g = np.where(g < f32(0), f32(0), g)
    return g / (f32(white) - f32(black))


def noisy(n, cl):
    """io.compose_noisy: clip(clip(n, -1, 1) + clean, 0, 1) in fp32."""
    n, cl = np.asarray(n, f32), np.asarray(cl, f32)
    nc = clip(n, f32(-1), f32(1))
    s = nc + cl
    assert s.dtype == f32
    return clip(s, f32(0), f32(1))


def short_codes(ny, ratio, black=BLACK, white=WHITE):
    """(4, H, W) fp32 noisy -> (4, H, W) int64 codes: min(trunc(p wb / ratio + black + 0.5), white) in fp64, NaN -> p = 0."""
    ny = np.asarray(ny, f32)
    p = np.where(np.isnan(ny), f32(0), ny).astype(np.float64)
    t = p * np.float64(f32(white) - f32(black))
    t = t / np.float64(f32(ratio))
    t = t + np.float64(f32(black))
    t = t + 0.5
    return np.minimum(np.trunc(t), np.float64(f32(white))).astype(np.int64)


def mosaic(planes):
    """(4, H, W) -> (2H, 2W) uint16 at pack_raw's Bayer sites."""
    _, h, w = planes.shape
    out = np.zeros((2 * h, 2 * w), np.uint16)
    out[0::2, 0::2], out[0::2, 1::2], out[1::2, 1::2], out[1::2, 0::2] = planes[0], planes[1], planes[2], planes[3]
    return out


def short(ny, ratio, black=BLACK, white=WHITE):
    return mosaic(short_codes(ny, ratio, black, white))


def stitch(patches, origins, rects, H, W):
    """The scatter: (P, 4, c, c) patches -> (4, H, W), each pixel from its owner."""
    out = np.zeros((4, H, W), f32)
    for p, (x0, y0), (ax0, ay0, ax1, ay1) in zip(patches, origins, rects):
        out[:, ay0:ay1, ax0:ax1] = p[:, ay0 - y0:ay1 - y0, ax0 - x0:ax1 - x0]
    return out


def frame(patches, crop, long_frame, ratio, hw=None, black=BLACK, white=WHITE):
    """One whole frame from its patches in layout order: {"noise", "noisy", "short"}.  long_frame None: a dark frame of packed size hw."""
    H, W = hw if long_frame is None else (long_frame.shape[0] // 2, long_frame.shape[1] // 2)
    _, _, _, _, origins, rects = layout(crop, H, W)
    noise = stitch(np.asarray(patches, f32), origins, rects, H, W)
    cl = np.zeros((4, H, W), f32) if long_frame is None else clean(long_frame, black, white)
    ny = noisy(noise, cl)
    return {"noise": noise, "noisy": ny, "short": short(ny, ratio, black, white)}
