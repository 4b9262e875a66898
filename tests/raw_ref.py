"""Numpy restatement of noisediff_amd.raw (csrc/raw.hip): the four contracts of DESIGN.md section 12, one IEEE operation per line in the order
given there -- float32 for the pack modes, the reference's mix of float32 and float64 for the Poisson-Gaussian set, float64 for the Bayer write.

Run on the capture's inputs the restatement must equal the reference's own functions (tests/golden/raw.npz) bit for bit; it is the yardstick
of the device kernels.  Nothing here imports the package: it can be wrong only in its own way."""
import numpy as np

from denoise_data_ref import philox4x32_10, poisson  # noqa: F401  (poisson: the draw the device repeats; re-exported for the tests)

BLACK, WHITE = 512, 16383
NORMAL_BLOCK = 32         # the Philox block of the normal draw: the Poisson draw stops at block 31
f32 = np.float32


def pack_planes(a):
    """(..., 2H, 2W) -> (..., 4, H, W) in pack_raw's channel order."""
    return np.stack([a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 1::2], a[..., 1::2, 0::2]], axis=-3)


def window(a, x0, y0, h, w, flip):
    """out[..., y, x] = a[..., y0 + (h-1-y if flip else y), x0 + x]."""
    out = a[..., y0:y0 + h, x0:x0 + w]
    return out[..., ::-1, :] if flip else out


def codes(frame):
    """(2H, 2W) uint16 -> x = (float)code as packed planes (4, H, W)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint16
    return pack_planes(frame).astype(f32)


def dark(dk, db, iso, blc):
    """d = (ds_k * iso + ds_b) + blc in fp32 from plane windows."""
    d = np.asarray(dk, f32) * f32(iso)
    d = d + np.asarray(db, f32)
    return d + f32(blc)


def pack(x, rescale=True, ratio=None, black=BLACK, white=WHITE):
    """ND_RAW_PACK: max(x - black, 0) [/ wb] [clip(v ratio, 0, 1)]."""
    wb = f32(white) - f32(black)
    v = np.maximum(x - f32(black), f32(0))
    if rescale:
        v = v / wb
    if ratio is not None:
        v = np.clip(v * f32(ratio), f32(0), f32(1))
    return v


def pack_shaded(x, d, ratio, black=BLACK, white=WHITE):
    """ND_RAW_PACK_SHADED: clip(pack_raw_withdarkshading(raw, iso, ratio) * ratio, 0, 1), nine steps."""
    black, white, ratio = f32(black), f32(white), f32(ratio)
    wb = white - black
    v = (x - black) / wb
    v = np.clip(v * ratio, f32(0), f32(1))
    v = v / ratio
    v = v * wb
    v = v + black
    v = np.clip(v, f32(0), white)
    v = v - d
    v = np.maximum(v - black, f32(0))
    v = v / wb
    return np.clip(v * ratio, f32(0), f32(1))


def train_real(x, d, ratio, black=BLACK, white=WHITE):
    """ND_RAW_TRAIN_REAL's noisy tensor; d None: no --sub_darkshading."""
    black, white, ratio = f32(black), f32(white), f32(ratio)
    wb = white - black
    v = np.maximum(x - black, f32(0))
    if d is not None:
        v = v - d
    v = v * ratio
    v = np.clip(v, f32(0), wb)
    return v / wb


def uniforms(seed, sample, draw, n, block):
    """(n, 4) float64 uniforms (word + 0.5) 2^-32 of Philox block ``block`` for element indices 0 .. n-1."""
    c = np.stack([np.arange(n, dtype=np.uint32), np.full(n, sample & 0xFFFFFFFF, np.uint32), np.full(n, draw, np.uint32),
                  np.full(n, block, np.uint32)], -1)
    k = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), (n, 2))
    return (philox4x32_10(c, k).astype(np.float64) + 0.5) * 2.0 ** -32


def normal64(seed, sample, draw, n):
    """Box-Muller in float64 on words 0 and 1 of block 32: z = sqrt(-2 log(u0)) cos((2 pi) u1)."""
    u = uniforms(seed, sample, draw, n, NORMAL_BLOCK)
    return np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos((2.0 * np.pi) * u[:, 1])


def normal(seed, sample, draw, n):
    """The normal the device uses and returns: normal64 rounded to float32."""
    return normal64(seed, sample, draw, n).astype(f32)


def pg_rate(x, ratio, k, black=BLACK):
    """(c, lam): c = max(x - black, 0) in fp32, lam = (double)(c / (float)ratio) / k."""
    c = np.maximum(x - f32(black), f32(0))
    latent = c / f32(ratio)
    return c, latent.astype(np.float64) / np.float64(k)


def pg_noisy(counts, normals, k, sd, ratio, black=BLACK, white=WHITE):
    """noisy = fl32(clip((k n + sd z) ratio, 0, wb) / wb), float64 throughout.  counts and normals are widened from whatever type they come in:
    the reference's own int64 counts and float64 normals, or the fp32 values the device uses and returns."""
    wb = np.float64(f32(white) - f32(black))
    p = np.float64(k) * np.asarray(counts).astype(np.float64)
    g = np.float64(sd) * np.asarray(normals).astype(np.float64)
    t = p + g
    t = t * np.float64(ratio)
    t = np.clip(t, 0.0, wb)
    t = t / wb
    return t.astype(f32)


def pg_clean(x, black=BLACK, white=WHITE):
    return np.maximum(x - f32(black), f32(0)) / (f32(white) - f32(black))


def to_bayer(img, bl, white=WHITE):
    """(4, h, w) fp32 -> (2h, 2w) uint16: trunc((double)clip(x, 0, 1) * (white - bl[c]) + bl[c]); NaN -> 0."""
    img = np.asarray(img, f32)
    nan = np.isnan(img)
    p = np.clip(np.where(nan, f32(0), img), f32(0), f32(1)).astype(np.float64)
    bl = np.asarray(bl, np.int64).reshape(4, 1, 1)
    t = p * (np.int64(white) - bl).astype(np.float64)
    t = t + bl.astype(np.float64)
    code = np.where(nan, 0, t.astype(np.int64)).astype(np.uint16)
    _, h, w = img.shape
    out = np.zeros((2 * h, 2 * w), np.uint16)
    out[0::2, 0::2], out[0::2, 1::2], out[1::2, 1::2], out[1::2, 0::2] = code[0], code[1], code[2], code[3]
    return out
