"""Numpy restatement of nd_raw_diffusion_batch_f32 (csrc/raw.hip): one IEEE float32 operation per line, in the order the
header lists them.

Run on the capture's inputs the restatement must equal the reference's own dataset code (tests/golden/diffusion_data.npz) bit for bit; it is the
yardstick of the device kernel.  Nothing here imports the package: it can be wrong only in its own way."""
import numpy as np

from raw_ref import codes, window

BLACK, WHITE = 512, 16383
f32 = np.float32


def noisy(x, ratio, black=BLACK, white=WHITE):
    """x: the short exposure's codes as float32 -> clip(max(x - black, 0) / wb * ratio, 0, 1)."""
    wb = f32(white) - f32(black)
    sv = x - f32(black)
    sv = np.maximum(sv, f32(0))
    sv = sv / wb
    sv = sv * f32(ratio)
    return np.clip(sv, f32(0), f32(1))


def clean(x, black=BLACK, white=WHITE):
    """x: the long exposure's codes as float32 -> max(x - black, 0) / wb, NOT clipped."""
    wb = f32(white) - f32(black)
    g = x - f32(black)
    g = np.maximum(g, f32(0))
    return g / wb


def coord(H, W, x0, y0, h, w):
    """(2, h, w): the window of make_coord(H, W, rescale=True), channels first -- row / (H - 1), then column / (W - 1), of the WHOLE frame."""
    rows = np.arange(y0, y0 + h).astype(f32) / f32(H - 1)
    cols = np.arange(x0, x0 + w).astype(f32) / f32(W - 1)
    return np.stack([np.broadcast_to(rows[:, None], (h, w)), np.broadcast_to(cols[None, :], (h, w))]).astype(f32)


def sample(short, long, x0, y0, h, w, ratio, black=BLACK, white=WHITE):
    """One sample's {noise, noisy_img, clean_img, coord} from two (2H, 2W) uint16 frames; either frame may be None, and what needs it is left out."""
    out = {}
    ref = short if short is not None else long
    if short is not None:
        out["noisy_img"] = noisy(window(codes(short), x0, y0, h, w, 0), ratio, black, white)
    if long is not None:
        out["clean_img"] = clean(window(codes(long), x0, y0, h, w, 0), black, white)
    if short is not None and long is not None:
        out["noise"] = out["noisy_img"] - out["clean_img"]
    out["coord"] = coord(ref.shape[0] // 2, ref.shape[1] // 2, x0, y0, h, w)
    return out
