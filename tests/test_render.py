"""noisediff_amd.render / csrc/develop.hip: a packed RAW frame developed to an sRGB picture, half size and bilinear.

CPU part: the surface, the tone curve and the scale multipliers against the restatement (tests/render_ref.py) and its pins, the restatement's
general bilinear rule against its closed interior forms, and every refusal.  GPU part (-m gpu): every output byte equals the restatement; the
outputs are pre-filled with 0xAB and one image longer than written, and the tail must stay untouched."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import render_ref as RR
from noisediff_amd import synth

DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CAM = (2.3, 1, 1.6, 0)
NEGATIVE = [[1.9, -0.7, -0.2], [-0.25, 1.6, -0.35], [0.03, -0.55, 1.52]]
BRIGHT = [[0.9, 0.3, 0.2], [0.2, 1.0, 0.2], [0.1, 0.3, 1.0]]                  # every row sums to 1.4
MATRICES = {"identity": np.eye(3).tolist(), "negative": NEGATIVE, "bright": BRIGHT}


# --------------------------------------------------------------------------- CPU

def test_the_develop_entry_point_is_built_declared_bound_and_exported():
    import noisediff_amd
    from noisediff_amd import _lib as L, build
    assert "develop" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "develop.hip"))
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    assert "int nd_raw_develop(" in header and "nd_develop_params" in header and "nd_raw_develop" in L.SIGNATURES
    assert hasattr(L.load(), "nd_raw_develop")
    assert C.sizeof(L.DevelopParams) == 4 * 4 + 4 + 4 * 4 + 9 * 4 + 4 * 4                       # nd_develop_params
    for name in ("Develop", "gamma_curve", "postprocess_bayer"):
        assert name in noisediff_amd.__all__ and callable(getattr(noisediff_amd, name))


@pytest.mark.parametrize("power,slope,imax", [(0.45, 4.5, 65536), (1 / 2.4, 12.92, 65536), (1, 1, 65536), (0.45, 4.5, 32768)])
def test_gamma_curve_equals_the_restatement_and_its_pins(power, slope, imax):
    from noisediff_amd import render
    curve = render.gamma_curve(power, slope, imax)
    assert curve.dtype == np.uint16 and curve.shape == (65536,) and np.array_equal(curve, RR.gamma_curve(power, slope, imax))
    assert (np.diff(curve.astype(np.int64)) >= 0).all() and np.array_equal(np.unique(curve >> 8), np.arange(256))
    _, g3, g4 = RR.gamma_params(power, slope)
    if (power, slope, imax) == (0.45, 4.5, 65536):
        assert (g3, g4) == (0.018053968510807452, 0.09929682680944099)
        assert curve[[0, 1, 2, 255, 1183, 4096, 32768, 65535]].tolist() == [0, 4, 9, 1147, 5323, 14181, 46231, 65535]
    if (power, slope) == (1, 1):
        assert np.array_equal(curve, np.arange(65536))
    if slope == 12.92:
        assert g3 == 0.003041282560127564
    if imax == 32768:
        assert (curve[32768:] == 65535).all() and np.array_equal(curve[:32768], RR.gamma_curve(power, slope, 65536)[::2])        # bright = 2: r doubles


@pytest.mark.parametrize("cam", [(2.3, 1, 1.6, 0), (2, 1.1, 1.5, 1.05)])
def test_scale_multipliers_equal_the_restatement_bit_for_bit(cam):
    from noisediff_amd import render
    for black, maximum in (((512,) * 4, None), ((512, 510, 515, 512), 12000.0)):
        d = render.Develop(black, cam_mul=cam, maximum=maximum)
        want = RR.scale_mul(cam, 16383 - min(black) if maximum is None else maximum)
        assert d.scale_mul.dtype == np.float32 and d.scale_mul.tobytes() == want.tobytes()
    assert (cam[3] != 0 or d.scale_mul[3] == d.scale_mul[1]) and d.scale_mul.min() == np.float32(65535.0 / 12000.0)       # the smallest multiplier becomes 1


def test_the_restated_bilinear_rule_equals_its_closed_interior_forms():
    s = np.floor(synth.uniform(4, "render.t.rule", (38, 54), 0.0, 65536.0).numpy()).astype(np.int64)
    got = RR.full(s)
    assert np.array_equal(got[1:-1, 1:-1], RR.full_interior(s))
    c = RR.channel_of_site(38, 54)
    for k, own in enumerate((c == 0, (c == 1) | (c == 3), c == 2)):
        assert np.array_equal(got[..., k][own], s[own])                                      # a site keeps its own colour
    assert got[0, 0].tolist() == [s[0, 0], (s[0, 1] + s[1, 0]) // 2, s[1, 1]]                # a corner: two greens, one blue
    assert got[0, 1].tolist() == [(s[0, 0] + s[0, 2]) // 2, s[0, 1], s[1, 1]]                # the top edge: no blue above
    assert got[-1, -1].tolist() == [(s[-2, -2]), (s[-1, -2] + s[-2, -1]) // 2, s[-1, -1]]
    assert got[-1, 2].tolist() == [s[-2, 2], s[-1, 2], (s[-1, 1] + s[-1, 3]) // 2]
    assert got[3, 0, 0] == (s[2, 0] + s[4, 0]) // 2 and got[2, 0, 2] == (s[1, 1] + s[3, 1]) // 2 and got[2, 0, 1] == (s[1, 0] + s[3, 0] + s[2, 1]) // 3


def test_develop_refuses_bad_arguments_without_a_gpu():
    from noisediff_amd import _lib as L, render
    D = render.Develop
    for kw in (dict(white=0), dict(white=65536), dict(black_level_per_channel=(512, 512, 512)), dict(black_level_per_channel=(512, -1, 512, 512)),
               dict(black_level_per_channel=(512, 512, 512, 16384)), dict(cam_mul=(0, 1, 1, 0)), dict(cam_mul=(1, -1, 1, 0)), dict(cam_mul=(1, 1, NAN, 0)),
               dict(cam_mul=(1, float("inf"), 1, 0)), dict(cam_mul=(1, 1, 1)), dict(maximum=0), dict(maximum=-5.0), dict(output_bps=12), dict(bright=0),
               dict(bright=-1.0), dict(rgb_cam=np.eye(4)), dict(rgb_cam=[[1, 0, 0], [0, NAN, 0], [0, 0, 1]]), dict(gamma=(0, 4.5))):
        with pytest.raises(ValueError):
            D(**kw)
    d, d16, dfull = D(), D(output_bps=16), D(half_size=False)
    x = torch.zeros(2, 4, 8, 12)
    for bad in (torch.zeros(2, 3, 8, 12), torch.zeros(8, 12), torch.zeros(2, 4, 0, 12), torch.zeros(3, 8, 12), torch.zeros(1, 2, 4, 8, 12),
                torch.zeros(2, 7, 12, dtype=torch.int16), torch.zeros(8, 11, dtype=torch.int16), np.zeros((2, 7, 12), np.uint16)):
        with pytest.raises(ValueError):
            d(bad)
    for bad in (torch.zeros(2, 4, 8, 12, dtype=torch.float64), torch.zeros(2, 16, 24, dtype=torch.int32), np.zeros((16, 24), np.int16), [[1, 2], [3, 4]]):
        with pytest.raises(TypeError):
            d(bad)
    for window in ((0, 0, 9, 12), (0, 0, 8, 13), (-1, 0, 4, 4), (0, -1, 4, 4), (9, 0, 4, 4), (0, 5, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        with pytest.raises(ValueError, match="leaves the packed frame"):
            d(x, window=window)
    for dev, out in ((d, torch.zeros(2, 8, 12, 3, dtype=torch.int16)), (d, torch.zeros(2, 8, 12, 4, dtype=torch.uint8)), (d, torch.zeros(1, 8, 12, 3, dtype=torch.uint8)),
                     (d, torch.zeros(2, 8, 12, 3, dtype=torch.uint8, device="meta")), (d, torch.zeros(2, 8, 24, 3, dtype=torch.uint8)[:, :, ::2]),
                     (d16, torch.zeros(2, 8, 12, 3, dtype=torch.uint8)), (dfull, torch.zeros(2, 8, 12, 3, dtype=torch.uint8)), (d, np.zeros((2, 8, 12, 3), np.uint8))):
        with pytest.raises(ValueError, match="out must be"):
            dev(x, out=out)
    with pytest.raises(ValueError, match="out must be"):
        d(x, window=(2, 1, 4, 8), out=torch.zeros(2, 8, 12, 3, dtype=torch.uint8))
    # CPU tensors reach the library's door and no further
    with pytest.raises(L.HipError, match="no CPU path"):
        d(x)
    with pytest.raises(L.HipError, match="no CPU path"):
        dfull(torch.zeros(16, 24, dtype=torch.int16), out=torch.zeros(1, 16, 24, 3, dtype=torch.uint8))
    with pytest.raises(L.HipError, match="no CPU path"):
        render.postprocess_bayer(x, d)


def test_the_entry_point_checks_its_arguments_before_any_launch():
    from noisediff_amd import _lib as L
    lib = L.load()
    f, odd, a4 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)             # never dereferenced: every call below fails its checks first

    def call(f32=f, u16=None, B=2, H=32, W=48, curve=f, out=f, h=32, w=48, params=True, **kw):
        p = L.DevelopParams((C.c_int32 * 4)(*kw.pop("black", (512,) * 4)), kw.pop("white", 16383), (C.c_float * 4)(*kw.pop("scale", (4.0,) * 4)),
                            (C.c_float * 9)(*kw.pop("m", np.eye(3).reshape(-1).tolist())), kw.pop("x0", 0), kw.pop("y0", 0), kw.pop("bps", 8), kw.pop("full", 0))
        assert not kw
        return lib.nd_raw_develop(f32, u16, B, H, W, C.byref(p) if params else None, curve, out, h, w, None)

    assert call(params=False) == -1 and call(curve=None) == -1 and call(out=None) == -1 and call(f32=None) == -1 and call(u16=f) == -1
    assert b"one of them" in lib.nd_last_error()
    assert call(B=0) == -1 and call(B=65536) == -1 and call(H=0) == -1 and call(w=0) == -1 and call(bps=12) == -1 and call(full=2) == -1
    assert call(white=0) == -1 and call(white=65536) == -1 and call(black=(512, -1, 512, 512)) == -1 and call(black=(512, 512, 512, 16384)) == -1
    assert call(scale=(1.0, NAN, 1.0, 1.0)) == -1 and call(scale=(1.0, 1.0, -1.0, 1.0)) == -1 and call(m=[float("inf")] + [0.0] * 8) == -1
    for full in (0, 1):
        assert call(h=33, full=full) == -2 and call(w=49, full=full) == -2 and call(x0=1, full=full) == -2 and call(y0=-1, h=8, full=full) == -2
        assert call(x0=8, y0=4, h=28, w=41, full=full) == -2 and call(x0=-2, w=8, full=full) == -2
    assert b"leaves the packed frame" in lib.nd_last_error()
    assert call(H=(1 << 24) + 1) == -2
    assert call(f32=odd) == -3 and call(f32=None, u16=odd) == -3 and call(out=odd) == -3 and call(curve=a4) == -3


# --------------------------------------------------------------------------- GPU

def _mosaic(tag, B, H2, W2, lo=0.0, hi=65536.0):
    return np.floor(synth.uniform(6, f"render.t.{tag}", (B, H2, W2), lo, hi).numpy()).astype(np.uint16)


def _on_device(src):
    """numpy uint16 frames as the device holds them (int16 storage), numpy fp32 as it is."""
    return torch.from_numpy(src.view(np.int16) if src.dtype == np.uint16 else src).to(DEV)


def _run(dev, src, window=None):
    """``dev`` on the device tensor ``src`` into an output filled with 0xAB and one image longer than written; the written part as numpy."""
    B = src.shape[0]
    H, W = (src.shape[2], src.shape[3]) if src.dtype == torch.float32 else (src.shape[1] // 2, src.shape[2] // 2)
    _, _, h, w = (0, 0, H, W) if window is None else window
    k = 1 if dev.half_size else 2
    if dev.output_bps == 8:
        buf = torch.full((B + 1, k * h, k * w, 3), 0xAB, dtype=torch.uint8, device=DEV)
    else:
        buf = torch.full((B + 1, k * h, k * w, 3), 0xABAB - 65536, dtype=torch.int16, device=DEV)
    got = dev(src, window=window, out=buf[:B])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    a = buf.cpu().numpy()
    a = a if dev.output_bps == 8 else a.view(np.uint16)
    assert (a[B] == (0xAB if dev.output_bps == 8 else 0xABAB)).all(), "the kernel wrote past its output"
    return a[:B]


def _ref(dev, src, window=None, sums=None):
    """The restatement with ``dev``'s parameters, image by image."""
    return np.stack([RR.develop(img, dev.black, dev.white, dev.scale_mul, dev.rgb_cam, RR.gamma_curve(), dev.output_bps, not dev.half_size, window, sums)
                     for img in src])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} values differ"


@pytest.mark.gpu
@pytest.mark.parametrize("bps", [8, 16])
def test_every_uint16_code_half_size(bps):
    from noisediff_amd import render
    perm = np.argsort(synth.uniform01(5, "render.t.codes", 65536), kind="stable").astype(np.uint16)
    assert np.array_equal(np.sort(perm), np.arange(65536, dtype=np.uint16))
    frame = perm.reshape(1, 256, 256)
    dev = render.Develop(cam_mul=CAM, output_bps=bps)
    s = RR.scaled(frame[0], dev.black, dev.scale_mul)
    inside = s[(frame[0] > 512) & (frame[0] < 4000)]
    assert (s[frame[0] <= 512] == 0).all() and (s[frame[0] > 16383] == 65535).all() and inside.min() > 0 and inside.max() < 65535
    _same(_run(dev, _on_device(frame)), _ref(dev, frame), f"every code, {bps} bit")


@pytest.mark.gpu
def test_packed_fp32_source_equals_the_restatement_and_the_mosaic_of_to_bayer():
    from noisediff_amd import raw, render
    j = np.arange(15872, dtype=np.float64)
    edge = (j / 15871).astype(np.float32)
    vals = np.concatenate([edge, np.nextafter(edge, np.float32(-1)), np.nextafter(edge, np.float32(2)), np.array([NAN, -0.25, 1.5], np.float32)])
    h, w = 72, 96
    n = 2 * 4 * h * w
    assert vals.size <= n
    flat = np.tile(vals, -(-n // vals.size))[:n]
    img = flat[np.argsort(synth.uniform01(3, "render.t.fp32", n), kind="stable")].reshape(2, 4, h, w)
    assert np.isnan(img).any() and (img == 1.5).any() and (img == -0.25).any()
    black = (512, 510, 515, 512)
    x = torch.from_numpy(img).to(DEV)
    mosaic = raw.to_bayer(x, black)
    for half_size in (True, False):
        dev = render.Develop(black, cam_mul=CAM, rgb_cam=NEGATIVE, half_size=half_size)
        got = _run(dev, x)
        _same(got, _ref(dev, img), f"fp32 source, half_size={half_size}")
        _same(_run(dev, mosaic if mosaic.dtype == torch.int16 else mosaic.view(torch.int16)), got, "the mosaic of to_bayer, developed")


@pytest.mark.gpu
@pytest.mark.parametrize("half_size", [True, False])
def test_colour_matrix_truncates_toward_zero_and_clips(half_size):
    from noisediff_amd import render
    frame = np.concatenate([_mosaic("matrix.wide", 1, 64, 96), _mosaic("matrix.low", 1, 64, 96, 0.0, 9.0)], axis=1)            # (1, 128, 96): s = code below
    frame[0, 0:2, 0:2] = [[1, 3], [3, 0]]                                                    # R = 1, G = 3, B = 0: 1.9 - 2.1 lies in (-1, 0)
    seen = {}
    for name, m in MATRICES.items():
        dev = render.Develop((0,) * 4, white=65535, rgb_cam=m, half_size=half_size)
        assert dev.scale_mul.tolist() == [1.0] * 4
        sums = []
        want = _ref(dev, frame, sums=sums)
        o = sums[0]
        seen[name] = (bool((o <= -1).any()), bool(((o > -1) & (o < 0)).any()), bool((o > 65535).any()))
        _same(_run(dev, _on_device(frame)), want, f"matrix {name}")
    assert seen["negative"] == (True, True, True) and seen["bright"][2] and seen["identity"] == (False, False, False)


FRAMES = {"33x47": (33, 47), "64x130": (64, 130), "96x512": (96, 512)}                      # packed; the last: 12 half-size workgroups of 1024 threads, 3 x 8 tiles of 32 x 64


def _windows(H, W):
    far_h, far_w = H // 2 + 1, W // 4 * 2
    return [(8, 4, H - 6, W - 12), (3, 2, H // 2, W // 2), (0, 0, 16, 32), (W - far_w, H - far_h, far_h, far_w)]


@functools.lru_cache(maxsize=None)
def _addressing_case(frame, half_size, packed):
    """(Develop, source as numpy, the restatement's whole-frame pictures), computed once per case and left unchanged."""
    from noisediff_amd import render
    H, W = FRAMES[frame]
    dev = render.Develop((512, 510, 515, 512), cam_mul=CAM, rgb_cam=NEGATIVE, half_size=half_size)
    src = synth.uniform(8, f"render.t.addr.{frame}", (3, 4, H, W), -0.05, 1.05).numpy() if packed else _mosaic(f"addr.{frame}", 3, 2 * H, 2 * W, 400.0, 17000.0)
    whole = _ref(dev, src)
    whole.setflags(write=False)
    return dev, src, whole


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["fp32", "u16"])
@pytest.mark.parametrize("half_size", [True, False], ids=["half", "full"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_addressing(frame, half_size, packed):
    dev, src, whole = _addressing_case(frame, half_size, packed)
    H, W = FRAMES[frame]
    k = 1 if half_size else 2
    x = _on_device(src)
    got = _run(dev, x)
    _same(got, whole, f"{frame} whole frame")
    _same(_run(dev, x), got, "a repeated call")
    for b in range(3):
        _same(_run(dev, x[b:b + 1]), got[b:b + 1], f"image {b} alone")
    for x0, y0, h, w in _windows(H, W):
        assert x0 + w <= W and y0 + h <= H
        _same(_run(dev, x, (x0, y0, h, w)), whole[:, k * y0:k * (y0 + h), k * x0:k * (x0 + w)], f"{frame} window {h} x {w} at ({x0}, {y0})")
    assert _windows(H, W)[-1][0] + _windows(H, W)[-1][3] == W and _windows(H, W)[-1][1] + _windows(H, W)[-1][2] == H           # it touches the far corner


@pytest.mark.gpu
@pytest.mark.parametrize("bps", [8, 16])
def test_full_resolution_borders(bps):
    from noisediff_amd import render
    dev = render.Develop(cam_mul=CAM, rgb_cam=BRIGHT, half_size=False, output_bps=bps)
    frame = _mosaic("border", 2, 74, 142, 300.0, 9000.0)                                      # packed 37 x 71: two 32 x 64 tiles on each axis, odd sides
    whole = _ref(dev, frame)
    x = _on_device(frame)
    got = _run(dev, x)
    ring = np.ones(whole.shape[1:3], bool)
    ring[1:-1, 1:-1] = False
    _same(got[:, ring], whole[:, ring], "the frame's outermost ring")
    _same(got, whole, "the whole frame")
    s = RR.scaled(frame[0], dev.black, dev.scale_mul)
    interior = RR.tone(RR.mix(RR.full_interior(s), dev.rgb_cam), RR.gamma_curve(), bps)
    assert not np.array_equal(np.pad(interior, ((1, 1), (1, 1), (0, 0)), mode="edge"), whole[0])          # clamping the border would show
    for x0, y0, h, w in ((5, 3, 9, 14), (0, 0, 37, 1), (70, 0, 37, 1), (0, 36, 1, 71), (1, 1, 35, 69), (40, 20, 17, 31)):
        _same(_run(dev, x, (x0, y0, h, w)), whole[:, 2 * y0:2 * (y0 + h), 2 * x0:2 * (x0 + w)], f"window {h} x {w} at ({x0}, {y0}): neighbours from outside it")
    one = _mosaic("one", 1, 2, 2, 300.0, 9000.0)                                              # a 1 x 1 packed frame: every neighbour count is 1 or 2
    _same(_run(dev, _on_device(one)), _ref(dev, one), "a 1 x 1 packed frame")


@pytest.mark.gpu
@pytest.mark.parametrize("half_size", [True, False], ids=["half", "full"])
def test_a_frame_larger_than_one_sweep_of_the_resident_workgroups(half_size):
    """One workgroup per CU walks the launch: 1024 x 1040 packed pixels are 520 full-resolution tiles and 260 K half-size thread items, more than 256
    workgroups of 1024 threads take in one sweep, so the second sweep, and the tile buffer's reuse, show here and at no smaller size."""
    from noisediff_amd import render
    dev = render.Develop(cam_mul=CAM, rgb_cam=NEGATIVE, half_size=half_size)
    frame = _mosaic("sweep", 1, 2048, 2080, 400.0, 17000.0)
    _same(_run(dev, _on_device(frame)), _ref(dev, frame), "1024 x 1040")


@pytest.mark.gpu
def test_postprocess_bayer_twin_and_a_captured_launch():
    from noisediff_amd import render
    dev = render.Develop((512, 510, 515, 512), cam_mul=CAM, rgb_cam=NEGATIVE)
    img = synth.uniform(8, "render.t.twin", (2, 4, 40, 52), 0.0, 1.0).numpy()
    x = torch.from_numpy(img).to(DEV)
    pic = render.postprocess_bayer(x, dev)
    want = _ref(dev, img)
    assert isinstance(pic, np.ndarray) and pic.shape == (40, 52, 3)
    _same(pic, want[0], "postprocess_bayer")
    assert np.array_equal(dev(x).cpu().numpy(), want) and np.array_equal(dev(x[1]).cpu().numpy(), want[1:])          # the allocating call; (4, H, W)
    frames = _mosaic("twin.u16", 1, 80, 104, 400.0, 17000.0)
    assert np.array_equal(dev(frames).cpu().numpy(), _ref(dev, frames))                        # numpy uint16 through raw.frames_on_device
    for full in (dev, render.Develop((512, 510, 515, 512), cam_mul=CAM, rgb_cam=NEGATIVE, half_size=False)):
        k = 1 if full.half_size else 2
        eager = full(x).clone()
        out = torch.full((2, 40 * k, 52 * k, 3), 0xAB, dtype=torch.uint8, device=DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            full(x, out=out)                                                                   # the curve is on the device before the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            full(x, out=out)
        for _ in range(2):
            out.fill_(0xAB)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
