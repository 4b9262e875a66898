"""noisediff_amd.frame: whole synthetic noisy frames from sampled patches, one HIP launch per batch (nd_frame_assemble, csrc/frame.hip).

CPU: the layout is a partition of the frame (every packed pixel owned once, by a patch that contains it); the numpy restatement
(tests/frame_ref.py) equals io.compose_noisy and, at ratio 1, raw_ref's Bayer write up to its rounding; bad arguments are refused without a GPU.
GPU: the launch equals the restatement with zero difference for every subset of outputs, on every vector width and batch size; rows with an empty
or an invalid rectangle write nothing; a captured launch replays with a rewritten table; the uint16 frame packs back to the noisy image within
half a code; FrameSynthesizer's frames do not depend on the batch size and equal the restatement on patches sampled one at a time.
Outputs are pre-filled with a sentinel and longer than the kernel writes."""
import ctypes as C
import functools
import itertools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_ref as R
import raw_ref
from noisediff_amd import synth

DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
KEYS = ("noise", "noisy", "short")
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(KEYS, n)]
F32_SENTINEL, U16_SENTINEL = np.float32(12345.0), np.uint16(0xABCD)           # neither can be a result: patch values stay below 2, codes below white


def _same(a, b):
    """Zero difference: the same bits, or a NaN on both sides."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# --------------------------------------------------------------------------- CPU 1: the layout

def _axis_is_partitioned(origins, seams, crop, L):
    assert origins == sorted(set(origins)) and origins[0] == 0 and origins[-1] == L - crop
    assert len(seams) == len(origins) + 1 and seams[0] == 0 and seams[-1] == L
    owners = np.zeros(L, np.int64)
    for o, a, b in zip(origins, seams[:-1], seams[1:]):
        assert o <= a <= b <= o + crop, (crop, L, o, a, b)         # the owned interval lies inside its patch
        owners[a:b] += 1
    assert (owners == 1).all(), (crop, L)                          # every pixel is owned once


def test_layout_is_a_partition_of_the_frame():
    from noisediff_amd import io
    from noisediff_amd.frame import FrameLayout
    for crop in (1, 2, 3, 5, 8, 16, 32, 256, 512):
        for L in range(crop, crop + 70):
            lay = FrameLayout(crop, (crop, L))
            _axis_is_partitioned(lay.xs, lay.sx, crop, L)
            assert lay.ys == [0] and lay.sy == [0, crop]
            tall = FrameLayout(crop, (L, crop))
            assert (tall.ys, tall.sy, tall.xs, tall.sx) == (lay.xs, lay.sx, [0], [0, crop])
            assert (lay.xs, lay.ys, lay.sx, lay.sy, lay.patches, lay.rects) == R.layout(crop, crop, L)
            assert set(lay.patches) == set(io.patch_grid(crop, L, crop)) and len(set(lay.patches)) == len(lay.patches)
    for crop, n in ((256, 88), (512, 24)):
        lay = FrameLayout(crop)                                     # the SID geometry, 1424 x 2128
        assert (lay.H, lay.W) == (1424, 2128) and len(lay) == len(lay.patches) == len(lay.rects) == n
        _axis_is_partitioned(lay.xs, lay.sx, crop, 2128)
        _axis_is_partitioned(lay.ys, lay.sy, crop, 1424)
        assert lay.patches == [(x, y) for y in lay.ys for x in lay.xs] and len(set(lay.patches)) == n
        owners = np.zeros((1424, 2128), np.int64)
        for (x, y), (ax0, ay0, ax1, ay1) in zip(lay.patches, lay.rects):
            assert x <= ax0 < ax1 <= x + crop and y <= ay0 < ay1 <= y + crop
            owners[ay0:ay1, ax0:ax1] += 1
        assert (owners == 1).all()
    assert FrameLayout(256).sx == [0, 224, 416, 608, 800, 992, 1184, 1376, 1568, 1760, 1928, 2128]
    small = FrameLayout(8, (20, 28))                                # the GPU test's frame: widths 7, 6, 6, 4, 5 at 0, 7, 13, 19, 23
    assert small.xs == [0, 6, 12, 18, 20] and small.ys == [0, 6, 12] and small.sx == [0, 7, 13, 19, 23, 28] and len(small) == 15
    for bad in ((0, (8, 8)), (8, (7, 28)), (8, (20, 7))):
        with pytest.raises(ValueError):
            FrameLayout(*bad)


def test_a_seam_gives_each_pixel_to_the_patch_it_lies_deepest_in():
    """Between two neighbours the seam is the middle of their overlap: left of it the left patch's border is further away, from it on the right one's."""
    from noisediff_amd.frame import FrameLayout
    for crop, L in ((8, 28), (16, 36), (32, 104), (256, 2128), (512, 1424)):
        lay = FrameLayout(crop, (crop, L))
        for i, (a, b) in enumerate(zip(lay.xs[:-1], lay.xs[1:])):
            s = lay.sx[i + 1]
            for p in range(b, a + crop):                            # the overlap of patches i and i + 1
                left, right = a + crop - 1 - p, p - b               # the pixel's distance to the border it is nearest to, in each patch
                assert (left > right) if p < s else (right >= left), (crop, L, p)


def test_synthesizer_batches_pad_the_tail_with_empty_rectangles():
    from noisediff_amd.frame import FrameLayout, FrameSynthesizer
    lay = FrameLayout(8, (20, 28))
    got = list(FrameSynthesizer.batches(lay, 2, 7))
    assert [k0 for k0, *_ in got] == [0, 7, 14, 21, 28] and all(len(fo) == len(xy) == len(rect) == 7 for _, fo, xy, rect in got)
    fo, xy, rect = ([v for b in got for v in b[i]] for i in (1, 2, 3))
    assert fo[:30] == [0] * 15 + [1] * 15 and xy[:30] == lay.patches * 2 and rect[:30] == lay.rects * 2
    assert fo[30:] == [1] * 5 and xy[30:] == [lay.patches[-1]] * 5
    assert all(r[0] == r[2] and r[1] == r[3] and r[:2] == lay.rects[-1][:2] for r in rect[30:])       # empty, and inside the patch
    assert [len(b[1]) for b in FrameSynthesizer.batches(lay, 1, 15)] == [15]
    with pytest.raises(ValueError):
        next(FrameSynthesizer.batches(lay, 1, 0))
    with pytest.raises(ValueError):
        next(FrameSynthesizer.batches(lay, 0, 4))


# --------------------------------------------------------------------------- CPU 2: the restatement

def _values(name, shape, nan=True):
    """Patch values in (-1.6, 1.6) with +-0, values beyond +-1, +-inf and NaN planted every 37 elements."""
    v = synth.uniform(21, name, shape, -1.6, 1.6).numpy().copy()
    special = [0.0, -0.0, 1.5, -1.5, INF, -INF, 1.0, -1.0] + ([NAN] if nan else [])
    flat = v.reshape(-1)
    at = np.arange(0, flat.size, 37)
    flat[at] = np.array(special, np.float32)[np.arange(len(at)) % len(special)]
    return v


def _long_frames(name, n, H, W):
    """Long-exposure codes in 400 .. 17500: some below black, some above white."""
    return np.floor(synth.uniform(9, name, (n, 2 * H, 2 * W), 400.0, 17500.0).numpy()).astype(np.uint16)


def test_restatement_of_noisy_equals_compose_noisy():
    from noisediff_amd import io
    n = _values("frame.t.compose", (4, 33, 47))
    cl = R.clean(_long_frames("frame.t.compose.long", 1, 33, 47)[0])
    assert cl.dtype == np.float32 and float(cl.max()) > 1 and float(cl.min()) == 0
    for c in (cl, np.zeros_like(cl)):                               # against a long exposure, and a dark frame
        got = R.noisy(n, c)
        want = io.compose_noisy(torch.from_numpy(n), torch.from_numpy(c)).numpy()
        assert got.dtype == np.float32 and _same(got, want)
        assert np.isnan(got).sum() == np.isnan(n).sum() > 0 and set(np.unique(got[~np.isnan(got)])) >= {0.0, 1.0}
    dark = R.clip(R.clip(n, np.float32(-1), np.float32(1)), np.float32(0), np.float32(1))     # a dark frame: the sum with 0 only makes a -0 a +0
    assert np.array_equal(R.noisy(n, np.zeros_like(cl)), dark, equal_nan=True)


def test_restatement_of_short_rounds_where_to_bayer_truncates():
    """At ratio 1 the code is nd_raw_to_bayer_u16's with every channel's black level at 512, except that it is rounded to nearest (t + 0.5 truncated)
    where raw_ref truncates t: the same code where t's fraction is below a half, the next one (white at most) elsewhere."""
    ny = R.noisy(_values("frame.t.short", (4, 20, 28), nan=False), R.clean(_long_frames("frame.t.short.long", 1, 20, 28)[0]))
    p = np.clip(np.where(np.isnan(ny), np.float32(0), ny), np.float32(0), np.float32(1)).astype(np.float64)
    t = p * np.float64(R.WHITE - R.BLACK)
    t = t + np.float64(R.BLACK)                                    # raw_ref.to_bayer's t
    want = np.minimum(np.trunc(t + 0.5), R.WHITE).astype(np.int64)
    got = R.short_codes(ny, 1.0)
    assert np.array_equal(got, want) and got.min() == R.BLACK and got.max() == R.WHITE
    trunc = raw_ref.to_bayer(ny, [R.BLACK] * 4)
    up = (t - np.trunc(t)) >= 0.5
    assert up.any() and not up.all()
    assert np.array_equal(R.short(ny, 1.0), R.mosaic(raw_ref.pack_planes(trunc).astype(np.int64) + up))
    assert np.array_equal(raw_ref.pack_planes(R.short(ny, 1.0)), got)                         # the Bayer sites are pack_raw's
    assert R.short_codes(np.float32([NAN, 0.0]), 1.0).tolist() == [R.BLACK, R.BLACK]             # a NaN is a zero here; to_bayer writes code 0 for it
    low = R.short_codes(ny, 300.0)
    assert low.min() == R.BLACK and low.max() == R.BLACK + 53                                  # 15871 / 300 + 0.5 = 53.4


# --------------------------------------------------------------------------- CPU 3: refusals

def test_check_refuses_bad_parameters_on_the_host():
    from noisediff_amd import _lib as L, frame as FR
    for bad in (dict(crop=0), dict(crop=8, black=600, white=600), dict(crop=8, white=70000)):
        with pytest.raises(ValueError):
            FR.FrameAssembler(**bad)
    a = FR.FrameAssembler(8)
    shape = (2, 40, 56)                                             # packed 20 x 28
    ok = dict(n_out=2, frame_out=[0, 1, 1], long=[1, 0, 0], xy=[(0, 0), (6, 6), (12, 6)], rect=[(0, 0, 7, 7), (7, 7, 13, 12), (13, 7, 19, 12)],
              ratio=[100, 250, 300], want=KEYS)
    rows = a.check(3, shape, **ok).view(FR.ROW)
    assert rows["frame_out"].tolist() == [0, 1, 1] and rows["frame_clean"].tolist() == [1, 0, 0] and rows["x0"].tolist() == [0, 6, 12]
    assert rows["ax0"].tolist() == [0, 7, 13] and rows["ay1"].tolist() == [7, 12, 12] and rows["ratio"].tolist() == [100.0, 250.0, 300.0]
    a.check(3, shape, **{**ok, "rect": [(0, 0, 7, 7), (7, 7, 7, 7), (13, 7, 19, 7)]})               # empty rectangles are valid
    a.check(3, shape, **{**ok, "rect": [(0, 0, 7, 7), (7, 7, 14, 12), (13, 7, 19, 12)], "frame_out": [0, 1, 0]})        # overlap on different frames
    a.check(3, shape, **{**ok, "rect": [(0, 0, 7, 7), (7, 7, 13, 12), (12, 7, 12, 12)]})            # an empty one overlaps nothing
    a.check(3, shape, **{**ok, "ratio": None, "want": ("noise", "noisy")})                           # the ratio is the short exposure's alone
    a.check(3, shape, **{**ok, "ratio": [0, NAN, -1], "want": ("noisy",)})
    overlap = {"rect": [(0, 0, 7, 7), (7, 7, 14, 12), (13, 7, 19, 12)]}
    changes = [overlap, {"rect": [(0, 0, 7, 7), (7, 7, 13, 12), (12, 11, 19, 12)]},
               {"ratio": [100, 0, 300]}, {"ratio": [100, -1, 300]}, {"ratio": [100, NAN, 300]}, {"ratio": [INF, 250, 300]}, {"ratio": None},
               {"ratio": [100, 250, 1e-60]}, {"ratio": [100, 250, 1e60]},
               {"frame_out": [0, 2, 1]}, {"frame_out": [-1, 1, 1]}, {"long": [2, 0, 0]}, {"long": [1, -1, 0]}, {"n_out": 1}, {"n_out": 0},
               {"xy": [(0, 0), (21, 6), (12, 6)]}, {"xy": [(0, 0), (6, 13), (12, 6)]}, {"xy": [(-1, 0), (6, 6), (12, 6)]},
               {"rect": [(0, 0, 9, 7), (7, 7, 13, 12), (13, 7, 19, 12)]}, {"rect": [(0, 0, 7, 7), (5, 7, 13, 12), (13, 7, 19, 12)]},
               {"rect": [(0, 0, 7, 7), (7, 7, 13, 15), (13, 7, 19, 12)]}, {"rect": [(0, 0, 7, 7), (7, 5, 13, 12), (13, 7, 19, 12)]},
               {"rect": [(0, 0, 7, 7), (9, 7, 8, 12), (13, 7, 19, 12)]}, {"rect": [(0, 0, 7, 7), (7, 9, 13, 8), (13, 7, 19, 12)]},
               {"frame_out": [0, 1]}, {"long": [1, 0]}, {"xy": [(0, 0), (6, 6)]}, {"rect": [(0, 0, 7, 7)]},
               {"want": ()}, {"want": ("noisy", "clean")}]
    for change in changes:
        with pytest.raises(ValueError):
            a.check(3, shape, **{**ok, **change})
    with pytest.raises(ValueError, match="overlapping"):
        a.check(3, shape, **{**ok, **overlap})
    for bad_shape in ((2, 39, 56), (2, 40, 55), (2, 14, 56), (2, 40, 14), (40,)):
        with pytest.raises(ValueError):
            a.check(3, bad_shape, **ok)
    dk = FR.FrameAssembler(8, dark_frame=True)
    rows = dk.check(3, (20, 28), **{**ok, "long": None}).view(FR.ROW)
    assert rows["frame_clean"].tolist() == [0, 0, 0] and rows["x0"].tolist() == [0, 6, 12]
    for bad_shape in ((2, 40, 56), (7, 28)):
        with pytest.raises(ValueError):
            dk.check(3, bad_shape, **{**ok, "long": None})
    patches, frames = torch.zeros(3, 4, 8, 8), torch.zeros(shape, dtype=torch.int16)
    with pytest.raises(L.HipError):
        a(patches, frames, **ok)
    with pytest.raises(L.HipError):
        dk(patches, (20, 28), **{**ok, "long": None})
    with pytest.raises(L.HipError):
        a.capture_inputs(3, "cpu")
    with pytest.raises(L.HipError):
        FR.FrameSynthesizer(8)(SimpleNamespace(image_size=8, sample_offset=0), frames, [0], 3)


def test_entry_point_refuses_each_bad_argument_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    f, odd = C.c_void_p(4096), C.c_void_p(4098)                    # never dereferenced: every call below fails its checks first

    def call(patches=f, frames=f, N=2, H2=40, W2=56, table=f, black=512.0, white=16383.0, noise=f, noisy=f, short=f, B=3, c=8, F=2):
        return lib.nd_frame_assemble(patches, frames, N, H2, W2, table, black, white, noise, noisy, short, B, c, F, None)

    none = dict(noise=None, noisy=None, short=None)
    assert call(H2=39) == -1 and b"even" in lib.nd_last_error()
    assert call(W2=55) == -1 and call(H2=0) == -1 and call(W2=-2) == -1
    assert call(c=0) == -1 and call(B=0) == -1 and call(F=0) == -1 and call(c=-1) == -1 and call(B=65536) == -1 and call(F=-3) == -1
    assert call(c=21) == -1 and b"does not fit" in lib.nd_last_error() and call(c=29) == -1
    assert call(table=None) == -1 and b"null table or patches" in lib.nd_last_error()
    assert call(patches=None) == -1
    assert call(**none) == -1 and b"at least one" in lib.nd_last_error()
    for name in ("noisy", "short"):
        assert call(N=0, **{**none, name: f}) == -1 and b"N must be positive" in lib.nd_last_error()
        assert call(N=-1, **{**none, name: f}) == -1
    for name in ("patches", "frames", "table", "noise", "noisy", "short"):
        assert call(**{name: odd}) == -1 and b"aligned" in lib.nd_last_error(), name
    assert call(white=512.0) == -1 and call(black=-1.0) == -1 and call(white=70000.0) == -1


def test_header_signatures_and_row_agree():
    from noisediff_amd import _lib as L, frame as FR
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    assert "int nd_frame_assemble(" in header and "nd_frame_assemble" in L.SIGNATURES and hasattr(L.load(), "nd_frame_assemble")
    args = re.search(r"int nd_frame_assemble\(([^;]*)\);", header).group(1).split(",")
    assert len(args) == len(L.SIGNATURES["nd_frame_assemble"][1]) == 15
    body = re.search(r"typedef struct nd_frame_patch \{(.*?)\} nd_frame_patch;", header, re.S).group(1)
    fields = [n.strip() for decl in re.findall(r"^\s*(?:int32_t|float)\s+([^;]+);", body, re.M) for n in decl.split(",")]
    assert fields == ["frame_out", "frame_clean", "x0", "y0", "ax0", "ay0", "ax1", "ay1", "ratio", "reserved[3]"]
    assert [n for n, *_ in L.FramePatch._fields_] == list(FR.ROW.names) == [n.split("[")[0] for n in fields]
    assert C.sizeof(L.FramePatch) == FR.ROW.itemsize == 12 * 4 == FR.FrameInputs.PER_SAMPLE
    assert all(getattr(L.FramePatch, n).offset == FR.ROW.fields[n][1] for n in FR.ROW.names)
    import noisediff_amd
    from noisediff_amd import build
    assert "frame" in build.SOURCES and all(getattr(noisediff_amd, n) is getattr(FR, n) for n in ("FrameLayout", "FrameAssembler", "FrameSynthesizer"))


# --------------------------------------------------------------------------- GPU

def _dev_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).to(DEV)


GEOMETRY = {                                                        # packed (H, W), crop
    "seams_on_every_residue": ((20, 28), 8),                        # owned widths 7, 6, 6, 4, 5 at 0, 7, 13, 19, 23: heads and tails at every width
    "three_by_two": ((24, 36), 16),
    "frame_equal_to_the_crop": ((12, 12), 12),                      # one patch owns everything
}
RATIOS, LONG = (1.0, 100.0, 250.0, 300.0), (1, 0, 1, 1)             # per output frame: its ratio and its long exposure


@functools.lru_cache(maxsize=None)
def _case(name, dark=False):
    """Inputs and the restatement's frames of one geometry, computed once: four output frames from two long exposures."""
    (H, W), c = GEOMETRY[name]
    _, _, _, _, origins, rects = R.layout(c, H, W)
    P, F = len(origins), len(RATIOS)
    patches = _values(f"frame.t.{name}", (F * P, 4, c, c))
    longs = _long_frames(f"frame.t.{name}.long", 2, H, W)
    ref = [R.frame(patches[f * P:(f + 1) * P], c, None if dark else longs[LONG[f]], RATIOS[f], (H, W)) for f in range(F)]
    want = {k: np.stack([r[k] for r in ref]) for k in KEYS}
    rows = [(f, LONG[f], *origins[p], *rects[p], RATIOS[f]) for f in range(F) for p in range(P)]
    return SimpleNamespace(H=H, W=W, c=c, P=P, F=F, patches=patches, longs=longs, want=want, rows=rows)


def _table(rows):
    from noisediff_amd import frame as FR
    t = np.zeros(len(rows), FR.ROW)
    for r, (fo, fc, x0, y0, ax0, ay0, ax1, ay1, ratio) in zip(t, rows):
        r["frame_out"], r["frame_clean"], r["x0"], r["y0"], r["ax0"], r["ay0"], r["ax1"], r["ay1"], r["ratio"] = fo, fc, x0, y0, ax0, ay0, ax1, ay1, ratio
        r["reserved"] = -1
    return t


class _Buffers:
    """Sentinel-filled outputs, `pad` elements longer than the kernel writes at each end + `offset` 4-byte words into them."""

    def __init__(self, F, H, W, want, offset=0, pad=64):
        self.n = {"noise": F * 4 * H * W, "noisy": F * 4 * H * W, "short": F * 4 * H * W}
        self.F, self.H, self.W, self.lead = F, H, W, pad + offset
        self.buf = {}
        for k in want:
            if k == "short":                                        # uint16 pairs: 4-byte words of two codes
                host = np.full(2 * (self.lead + self.n[k] // 2 + pad), U16_SENTINEL, np.uint16)
                self.buf[k] = torch.from_numpy(host.view(np.int16)).to(DEV)
            else:
                self.buf[k] = torch.full((self.lead + self.n[k] + pad,), float(F32_SENTINEL), device=DEV)

    def ptr(self, k):
        return self.buf[k].data_ptr() + 4 * self.lead if k in self.buf else None

    def read(self, must_be_written=True):
        """{name: the frames} after checking that nothing around them changed and, with must_be_written, that no sentinel is left inside."""
        res = {}
        for k, t in self.buf.items():
            a = t.cpu().numpy()
            if k == "short":
                a, lead, n, sentinel = a.view(np.uint16), 2 * self.lead, self.n[k], U16_SENTINEL
                shape = (self.F, 2 * self.H, 2 * self.W)
            else:
                lead, n, sentinel, shape = self.lead, self.n[k], F32_SENTINEL, (self.F, 4, self.H, self.W)
            assert (a[:lead] == sentinel).all() and (a[lead + n:] == sentinel).all(), f"the kernel wrote outside {k}"
            inside = a[lead:lead + n]
            assert not must_be_written or not (inside == sentinel).any(), f"{k}: pixels were left unwritten"
            res[k] = inside.reshape(shape).copy()
        return res


def _launch(bufs, patches, rows, fd, N, case):
    """One nd_frame_assemble for the rows given, straight through the C entry point."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    table = torch.from_numpy(_table(rows).view(np.uint8)).to(DEV)
    pd = torch.from_numpy(np.ascontiguousarray(patches)).to(DEV)
    L.call("nd_frame_assemble", pd.data_ptr(), L.ptr(fd), N, 2 * case.H, 2 * case.W, table.data_ptr(), 512.0, 16383.0,
           *[bufs.ptr(k) for k in KEYS], len(rows), case.c, case.F, _stream(DEV))


def _empty(row):
    fo, fc, x0, y0, ax0, ay0, ax1, ay1, ratio = row
    return (fo, fc, x0, y0, ax0, ay0, ax0, ay0, ratio)


def _invalid(case, N, row):
    """Rows that name a rectangle or an index the launch must not touch: each would write if it were not refused."""
    fo, fc, x0, y0, ax0, ay0, ax1, ay1, ratio = row
    H, W, c = case.H, case.W, case.c
    bad = [(case.F, fc, x0, y0, ax0, ay0, ax1, ay1, ratio), (-1, fc, x0, y0, ax0, ay0, ax1, ay1, ratio),
           (fo, fc, W - c + 1, y0, W - c + 1, ay0, W - c + 2, ay1, ratio), (fo, fc, x0, H - c + 1, ax0, H - c + 1, ax1, H - c + 2, ratio),
           (fo, fc, -1, y0, 0, ay0, 1, ay1, ratio), (fo, fc, x0, -1, ax0, 0, ax1, 1, ratio),
           (fo, fc, x0, y0, x0 - 1, ay0, ax1, ay1, ratio), (fo, fc, x0, y0, ax0, ay0, x0 + c + 1, ay1, ratio),
           (fo, fc, x0, y0, ax0, y0 - 1, ax1, ay1, ratio), (fo, fc, x0, y0, ax0, ay0, ax1, y0 + c + 1, ratio),
           (fo, fc, x0, y0, ax1, ay0, ax0 - 1, ay1, ratio), (fo, fc, x0, y0, ax0, ay1, ax1, ay0 - 1, ratio)]
    if N:
        bad += [(fo, N, x0, y0, ax0, ay0, ax1, ay1, ratio), (fo, -1, x0, y0, ax0, ay0, ax1, ay1, ratio)]
    return bad


def _run(case, want, bs, offset, fd, N, spoil=False):
    """Every patch of the case in launches of exactly `bs` rows; the last is padded with an empty row and (spoil) invalid ones."""
    bufs = _Buffers(case.F, case.H, case.W, want, offset)
    total = len(case.rows)
    for k0 in range(0, total, bs):
        idx = [min(k, total - 1) for k in range(k0, k0 + bs)]
        rows = [case.rows[k] if k0 + i < total else _empty(case.rows[k]) for i, k in enumerate(idx)]
        if spoil:
            bad = _invalid(case, N, case.rows[-1])
            rows = [r if k0 + i < total or i % 2 else bad[i % len(bad)] for i, r in enumerate(rows)]
        _launch(bufs, case.patches[idx], rows, fd, N, case)
    torch.cuda.synchronize()
    return bufs.read()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_kernel_equals_the_restatement_on_every_path(name):
    case = _case(name)
    fd = _dev_frames(case.longs)
    assert np.isnan(case.want["noise"]).any() and np.isinf(case.want["noise"]).any() and (case.want["noisy"] == 1).any()
    assert (case.P * case.F) % 7 != 0                               # seven rows a launch leave a padded tail
    for want in SUBSETS:
        for offset in (0, 1, 2):                                    # outputs 16-, 4- and 8-byte aligned: four, one and two columns per thread
            got4 = _run(case, want, 4, offset, fd, 2)
            got7 = _run(case, want, 7, offset, fd, 2, spoil=True)
            assert set(got4) == set(got7) == set(want)
            for k in want:
                diff = int((got4[k] != case.want[k]).sum()) if k == "short" else -1
                assert _same(got4[k], case.want[k]), f"{name} {want} offset {offset}: {k} differs from the restatement ({diff} codes)"
                assert _same(got7[k], got4[k]), f"{name} {want} offset {offset}: {k} depends on the batch size"
    assert case.want["short"].max() <= 16383 and case.want["short"].min() == 512


@pytest.mark.gpu
def test_empty_and_invalid_rows_write_nothing():
    case = _case("seams_on_every_residue")
    fd = _dev_frames(case.longs)
    row = case.rows[7]                                              # an inner patch of frame 0: every neighbour is inside the frame
    for frames, N in ((fd, 2), (None, 0)):
        bad = [_empty(row)] + _invalid(case, N, row)
        bad += [row[:8] + (r,) for r in (0.0, -100.0, NAN, INF)]    # a ratio the short exposure cannot be formed with
        bufs = _Buffers(case.F, case.H, case.W, KEYS)
        _launch(bufs, case.patches[[7] * len(bad)], bad, frames, N, case)
        torch.cuda.synchronize()
        got = bufs.read(must_be_written=False)
        assert all((got[k] == (U16_SENTINEL if k == "short" else F32_SENTINEL)).all() for k in KEYS)
        bufs = _Buffers(case.F, case.H, case.W, ("noise", "noisy"))                           # without short the ratio is not read
        _launch(bufs, case.patches[[7] * 2], [row[:8] + (NAN,), _empty(row)], frames, N, case)
        torch.cuda.synchronize()
        got = bufs.read(must_be_written=False)
        fo, _, _, _, ax0, ay0, ax1, ay1, _ = row
        written = np.zeros((case.F, 4, case.H, case.W), bool)
        written[fo, :, ay0:ay1, ax0:ax1] = True
        assert all(((got[k] != F32_SENTINEL) == written).all() for k in got)
        assert _same(got["noise"][written], case.want["noise"][written])


@pytest.mark.gpu
def test_dark_frames_have_no_long_exposure():
    case = _case("seams_on_every_residue", dark=True)
    for want in (KEYS, ("noisy",), ("short",)):
        got = _run(case, want, 7, 0, None, 0)
        assert all(_same(got[k], case.want[k]) for k in want)
    n = case.want["noise"]
    one, zero = np.float32(1), np.float32(0)
    assert np.array_equal(got["short"], case.want["short"]) and len(np.unique(case.want["short"])) > 50
    assert np.array_equal(case.want["noisy"], R.clip(R.clip(n, -one, one), zero, one), equal_nan=True)
    noisy = _run(case, ("noisy",), 4, 0, None, 0)["noisy"]
    assert np.array_equal(noisy, np.clip(np.clip(n, -one, one), zero, one), equal_nan=True)
    from noisediff_amd.frame import FrameAssembler
    dk = FrameAssembler(case.c, dark_frame=True)
    rows = np.array(case.rows[:case.P])
    out = dk(torch.from_numpy(case.patches[:case.P]).to(DEV), (case.H, case.W), 1, rows[:, 0], None, rows[:, 2:4], rows[:, 4:8], RATIOS[0], want=KEYS)
    torch.cuda.synchronize()
    assert _same(out["noisy"][0].cpu().numpy(), case.want["noisy"][0]) and _same(out["noise"][0].cpu().numpy(), case.want["noise"][0])
    assert np.array_equal(out["short"][0].cpu().numpy().view(np.uint16), case.want["short"][0])


def _batch(case, k0, n):
    rows = np.array(case.rows[k0:k0 + n])
    return dict(frame_out=rows[:, 0], long=rows[:, 1], xy=rows[:, 2:4], rect=rows[:, 4:8], ratio=rows[:, 8])


def _prefilled(case):
    out = {k: torch.full((case.F, 4, case.H, case.W), float(F32_SENTINEL), device=DEV) for k in ("noise", "noisy")}
    out["short"] = torch.from_numpy(np.full((case.F, 2 * case.H, 2 * case.W), U16_SENTINEL, np.uint16).view(np.int16)).to(DEV)
    return out


@pytest.mark.gpu
def test_a_captured_launch_replays_with_a_rewritten_table():
    from noisediff_amd.frame import FrameAssembler
    case = _case("seams_on_every_residue")
    fd = _dev_frames(case.longs)
    shape, B = tuple(fd.shape), 5
    asm = FrameAssembler(case.c)
    first, second = _batch(case, 0, B), _batch(case, case.P + 3, B)                          # rows of frame 0, then of frame 1
    pd = torch.from_numpy(case.patches[:B].copy()).to(DEV)
    inputs = asm.capture_inputs(B, DEV)
    asm.update(inputs, shape, case.F, **first, want=KEYS)
    out = _prefilled(case)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        asm.launch(inputs, pd, fd, out=out, want=KEYS)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = asm.launch(inputs, pd, fd, out=out, want=KEYS)
    assert set(res) == set(KEYS) and all(res[k] is out[k] for k in KEYS)                    # the launch wrote into what it was given
    for params, k0 in ((first, 0), (second, case.P + 3), (first, 0)):
        asm.update(inputs, shape, case.F, **params, want=KEYS)
        pd.copy_(torch.from_numpy(case.patches[k0:k0 + B].copy()))
        fresh = _prefilled(case)
        for k in KEYS:
            out[k].copy_(fresh[k])
        g.replay()
        torch.cuda.synchronize()
        eager = asm(pd, fd, case.F, **params, want=KEYS, out=fresh)
        torch.cuda.synchronize()
        assert all(eager[k] is fresh[k] for k in KEYS)
        written = np.zeros((case.F, case.H, case.W), bool)
        for fo, (ax0, ay0, ax1, ay1) in zip(params["frame_out"], params["rect"]):
            written[int(fo), int(ay0):int(ay1), int(ax0):int(ax1)] = True
        every = np.broadcast_to(written[:, None], (case.F, 4, case.H, case.W))
        for k in ("noise", "noisy"):
            a, e = out[k].cpu().numpy(), fresh[k].cpu().numpy()
            assert _same(a, e) and _same(a[every], case.want[k][every]) and (a[~every] == F32_SENTINEL).all()
        a, e = (t.cpu().numpy().view(np.uint16) for t in (out["short"], fresh["short"]))
        site = np.repeat(np.repeat(written, 2, axis=1), 2, axis=2)
        assert np.array_equal(a, e) and np.array_equal(a[site], case.want["short"][site]) and (a[~site] == U16_SENTINEL).all()


@pytest.mark.gpu
def test_the_short_frame_packs_back_to_the_noisy_image():
    """raw.load_pair of the uint16 frame against noisy: |diff| <= (0.5 + 2^-7) ratio / (white - black), everywhere.  0.5 is the half code of
    rounding to nearest (the code itself is formed in double: its own error is far below).  The 2^-7 of a code is derived, not measured: on the way
    back load_pair rounds to fp32 three times on values <= 1 (the division by wb, the product with the ratio, and noisy is an fp32 value itself),
    2^-24 each at most, and 2^-24 of the packed range is wb / ratio * 2^-24 <= 15871 * 2^-24 < 2^-10 of a code: 3 * 2^-10 in all, under half of 2^-7.
    The final clip to [0, 1] only moves the value towards noisy, which lies in [0, 1].  Measured on this frame: 0.4995, 0.4986, 0.4994 and 0.4998 of a
    code at ratios 1, 100, 250 and 300."""
    from noisediff_amd import raw
    from noisediff_amd.frame import FrameAssembler, FrameLayout
    (H, W), c = GEOMETRY["three_by_two"]
    lay = FrameLayout(c, (H, W))
    P = len(lay)
    longs = _long_frames("frame.t.round.long", 2, H, W)
    patches = _values("frame.t.round", (4 * P, 4, c, c), nan=False)                          # a NaN has no code to come back from
    fd = _dev_frames(longs)
    asm = FrameAssembler(c)
    fo = [f for f in range(4) for _ in range(P)]
    out = asm(torch.from_numpy(patches).to(DEV), fd, 4, fo, [LONG[f] for f in fo], lay.patches * 4, lay.rects * 4, [RATIOS[f] for f in fo], want=("noisy", "short"))
    for f, ratio in enumerate(RATIOS):
        back = raw.load_pair(out["short"][f], longs[LONG[f]], 100, ratio)[0]
        diff = float((back[0] - out["noisy"][f]).abs().max())
        bound = (0.5 + 2.0 ** -7) * ratio / (16383 - 512)
        print(f"ratio {ratio}: max |load_pair(short) - noisy| = {diff:.6g}, bound {bound:.6g}")
        assert diff <= bound, (ratio, diff, bound)
        assert diff > 0.2 * ratio / (16383 - 512)                                           # the codes do round: the error is not zero either


@pytest.mark.gpu
def test_whole_frames_end_to_end_do_not_depend_on_the_batch_size():
    from noisediff_amd import Develop, FrameSynthesizer, GaussianDiffusion, GenerationBatchBuilder, NoiseDiffNet, noise_level, raw
    from util import state_dict
    dim, c, (H, W) = 16, 32, (40, 56)
    longs = _long_frames("frame.t.e2e.long", 3, H, W)
    fd = _dev_frames(longs)
    net = NoiseDiffNet(SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
    net.load_state_dict(state_dict(dim), strict=True)
    net = net.to(DEV).eval()
    gs = GaussianDiffusion(net, image_size=c, timesteps=1000, sampling_timesteps=3, beta_schedule="sigmoid2").to(DEV)
    long, idx, ratio, seed, first = [2, 0, 1], [7, 74, 31], [100.0, 250.0, 300.0], 11, 7
    synthesize = FrameSynthesizer(c)
    gs.sample_offset = 3
    a = synthesize(gs, fd, long, idx, ratio, batch_size=5, seed=seed, first_sample=first, want=KEYS)      # 12 patches: 5 + 5 + 2 and three padded rows
    assert gs.sample_offset == 3
    b = synthesize(gs, fd, long, idx, ratio, batch_size=3, seed=seed, first_sample=first, want=KEYS)
    torch.cuda.synchronize()
    assert set(a) == set(b) == set(KEYS) and a["noise"].shape == a["noisy"].shape == (3, 4, H, W) and a["short"].shape == (3, 2 * H, 2 * W)
    assert all(torch.equal(a[k], b[k]) for k in KEYS)
    assert torch.isfinite(a["noise"]).all() and float(a["noise"].std()) > 0

    _, _, _, _, origins, _ = R.layout(c, H, W)
    assert len(origins) == 4
    gb, singles = GenerationBatchBuilder(c), []
    try:
        for k in range(3 * len(origins)):                           # the same patches, sampled one at a time
            f, p = divmod(k, len(origins))
            gs.sample_offset = first + k
            singles.append(gs.sample(batch_size=1, condition=gb(fd, [long[f]], [origins[p]], idx[f]), seed=seed)[0].cpu().numpy())
    finally:
        gs.sample_offset = 3
    for f in range(3):
        want = R.frame(np.stack(singles[4 * f:4 * f + 4]), c, longs[long[f]], ratio[f])
        assert _same(a["noise"][f].cpu().numpy(), want["noise"]) and _same(a["noisy"][f].cpu().numpy(), want["noisy"])
        assert np.array_equal(a["short"][f].cpu().numpy().view(np.uint16), want["short"])

    other = synthesize(gs, fd, long, idx, ratio, batch_size=5, seed=seed, first_sample=first + 1, want=("noise",))
    assert set(other) == {"noise"} and not torch.equal(other["noise"], a["noise"]) and gs.sample_offset == 3
    into = {"noisy": torch.empty_like(a["noisy"])}
    again = synthesize(gs, fd, long, idx, batch_size=5, seed=seed, first_sample=first, out=into)                         # the default: noisy alone, no ratio
    assert set(again) == {"noisy"} and again["noisy"] is into["noisy"] and torch.equal(into["noisy"], a["noisy"])

    for f in range(3):                                              # the outputs are frames to the tools that take frames: finite results only
        pic = Develop()(a["short"][f])
        assert pic.shape[-1] == 3 and Develop()(a["noisy"][f]).shape == pic.shape
        noisy, clean = raw.load_pair(a["short"][f], longs[long[f]], 100, ratio[f])
        lam, sigma = noise_level.get_poisson_lambda(clean, noisy)
        assert math.isfinite(float(lam)) and math.isfinite(float(sigma))
