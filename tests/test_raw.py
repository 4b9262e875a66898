"""noisediff_amd.raw: uint16 Bayer frames to packed fp32 (pack_raw, load_image, the RealSony and Poisson-Gaussian training samples) and back
(postprocess_bayer's write), one HIP launch each.

CPU: the numpy restatement (tests/raw_ref.py) equals the reference's own functions (tests/golden/raw.npz, captured by tests/golden/capture_raw.py)
bit for bit; bad arguments are refused without a GPU; random_params consumes np.random as the reference does; the float64 Box-Muller draw passes
mean / variance / correlation checks.
GPU: every pack mode equals the restatement bit for bit on every uint16 code and on every addressing path; the Poisson-Gaussian launch equals
it bit for bit from explicit draws and within one fp32 rounding when it draws; the Bayer write is bitwise; the launches capture into graphs;
evaluate_raw scores a full-size frame as evaluate does; a training step runs on both kinds of batch.  Outputs are pre-filled with NaN."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raw_ref as R
from noisediff_amd import synth

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(100, 800), (250, 1600), (300, 25600)]          # ratio, iso
BLC = {800: 0.25, 1600: -0.5, 25600: 1.75}
NAN = float("nan")


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "raw.npz"))
    seed, (H2, W2) = int(z["meta.seed"]), z["meta.shape"]
    frames = {n: np.floor(synth.uniform(seed, f"raw.{n}", (H2, W2), lo, hi).numpy()).astype(np.uint16)
              for n, lo, hi in (("short", 480.0, 700.0), ("long", 400.0, 16384.0))}
    rng = {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}
    bayer = {k: synth.uniform(seed, f"raw.ds_{k}", (H2, W2), lo, hi).numpy() for k, (lo, hi) in rng.items()}
    assert [tuple(c) for c in z["meta.cases"]] == CASES and dict(zip(z["meta.blc_iso"].tolist(), z["meta.blc"].tolist())) == BLC
    return SimpleNamespace(z=z, frames=frames, bayer=bayer, planes={k: R.pack_planes(v) for k, v in bayer.items()}, crop=int(z["meta.crop"]))


def ref_dark(planes, iso, x0, y0, h, w, flip, blc=BLC):
    pair = "high" if iso > 1600 else "low"
    return R.dark(R.window(planes["k_" + pair], x0, y0, h, w, flip), R.window(planes["b_" + pair], x0, y0, h, w, flip), iso, blc[iso])


def ref_pack(mode, frame, x0, y0, h, w, flip, ratio, iso, planes=None, rescale=True, clip=True, blc=BLC):
    """One sample of nd_raw_pack_u16_f32 from the restatement: mode 'pack' | 'shaded' | 'real'."""
    x = R.window(R.codes(frame), x0, y0, h, w, flip)
    d = ref_dark(planes, iso, x0, y0, h, w, flip, blc) if planes is not None else None
    if mode == "pack":
        return R.pack(x, rescale, ratio if clip else None)
    return R.pack_shaded(x, d, ratio) if mode == "shaded" else R.train_real(x, d, ratio)


# --------------------------------------------------------------------------- CPU 1: the restatement against the reference

def test_restated_pack_raw_equals_the_reference(gold):
    z, f = gold.z, gold.frames
    assert np.array_equal(R.pack(R.codes(f["long"]), True), z["pack_raw.long.1"])
    got = R.pack(R.codes(f["short"]), False)
    assert got.dtype == np.float32 and np.array_equal(got, z["pack_raw.short.0"])
    assert float((z["pack_raw.short.0"] == 0).mean()) > 0.05 and float(z["pack_raw.long.1"].max()) > 0.99          # both ends of the range are there


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restated_load_image_equals_the_reference_with_and_without_shading(gold, i):
    z, f = gold.z, gold.frames
    ratio, iso = CASES[i]
    H, W = f["short"].shape[0] // 2, f["short"].shape[1] // 2
    shaded = ref_pack("shaded", f["short"], 0, 0, H, W, 0, ratio, iso, gold.planes)
    plain = ref_pack("pack", f["short"], 0, 0, H, W, 0, ratio, iso)
    assert shaded.dtype == np.float32 and np.array_equal(shaded, z[f"load_image.{i}.1.noisy"])
    assert np.array_equal(plain, z[f"load_image.{i}.0.noisy"])
    assert np.array_equal(ref_pack("pack", f["long"], 0, 0, H, W, 0, 1, 0), z["load_image.clean"])
    assert not np.array_equal(shaded, plain) and 0.05 < float((shaded > 0).mean()) and float((shaded < 1).mean()) > 0.05


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restated_real_sample_equals_the_reference_with_and_without_shading(gold, i):
    z, f, c = gold.z, gold.frames, gold.crop
    ratio, iso = CASES[i]
    for sub in (1, 0):
        x0, y0 = (int(v) for v in z[f"real.{i}.{sub}.xy"])
        noisy = ref_pack("real", f["short"], x0, y0, c, c, 0, ratio, iso, gold.planes if sub else None)
        clean = ref_pack("pack", f["long"], x0, y0, c, c, 0, 1, 0, clip=False)
        assert np.array_equal(noisy, z[f"real.{i}.{sub}.noisy"]) and np.array_equal(clean, z[f"real.{i}.{sub}.clean"])
        assert 0.05 < float((noisy > 0).mean())


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restated_apply_noise_equals_the_reference_from_its_recorded_draws(gold, i):
    z, f, c = gold.z, gold.frames, gold.crop
    ratio, _ = CASES[i]
    x0, y0 = (int(v) for v in z[f"pg.{i}.xy"])
    k, var = float(z[f"pg.{i}.k"]), float(z[f"pg.{i}.var"])
    K, VAR = z["meta.profile"][i]
    assert 0.7 * K <= k <= 1.3 * K and k != K and 0.7 * VAR <= var <= 1.3 * VAR
    x = R.window(R.codes(f["long"]), x0, y0, c, c, 0)
    counts, normals = z[f"pg.{i}.counts"], z[f"pg.{i}.normals"]
    assert np.array_equal(counts.astype(np.float32), counts)                      # counts are exact in fp32, as the builder's 2**24 check promises
    # the reference's normals are float64 and pg_noisy widens what it is given: from the recorded draws it must give the reference's bits
    assert normals.dtype == np.float64 and not np.array_equal(normals.astype(np.float32), normals)
    got = R.pg_noisy(counts, normals, k, math.sqrt(var), ratio)
    assert got.dtype == np.float32 and np.array_equal(got, z[f"pg.{i}.noisy"])
    assert 0.05 < float((got > 0).mean()) and float((got < 1).mean()) > 0.05
    assert np.array_equal(R.pg_clean(x), z[f"pg.{i}.clean"])
    # the rate the reference handed to np.random.poisson: fp32 division by ratio, widened, fp64 division by k
    c, lam = R.pg_rate(x, ratio, k)
    assert c.dtype == np.float32 and lam.dtype == np.float64 and np.array_equal(lam, z[f"pg.{i}.lam"])
    assert abs(counts.mean() / lam.mean() - 1) < 0.05                             # and the recorded counts were drawn at it


def test_restated_bayer_write_equals_the_reference(gold):
    z = gold.z
    H2, W2 = z["meta.shape"]
    img = synth.uniform(int(z["meta.seed"]), "raw.img4c", (1, 4, H2 // 2, W2 // 2), -0.1, 1.1).numpy()[0]
    for j, bl in enumerate(z["meta.black_levels"]):
        got = R.to_bayer(img, bl)
        assert got.dtype == np.uint16 and np.array_equal(got, z[f"bayer.{j}"])
    assert not np.array_equal(z["bayer.0"], z["bayer.1"])


# --------------------------------------------------------------------------- CPU 2: the normal draw

def test_box_muller_restatement_statistics():
    n = 1 << 20
    zs = R.normal64(1234, 3, 1, n)
    assert zs.dtype == np.float64 and np.isfinite(zs).all()
    zm = zs.mean() * math.sqrt(n)
    zv = (zs.var() - 1.0) / math.sqrt(2.0 / n)
    zc = (zs[:-1] * zs[1:]).mean() * math.sqrt(n - 1)
    other = R.normal64(1234, 4, 1, n)
    zo = (zs * other).mean() * math.sqrt(n)
    print(f"Box-Muller z-scores: mean {zm:.2f} variance {zv:.2f} neighbour {zc:.2f} other sample {zo:.2f}")
    assert abs(zm) < 5 and abs(zv) < 5 and abs(zc) < 5 and abs(zo) < 5
    assert abs((np.abs(zs) > 3).mean() - 0.0026998) < 5 * math.sqrt(0.0027 / n)        # the tails are there
    assert np.array_equal(zs, R.normal64(1234, 3, 1, n)) and not np.array_equal(zs[:64], R.normal64(1235, 3, 1, 64))
    assert not np.array_equal(zs[:64], R.normal64(1234, 3, 2, 64))


# --------------------------------------------------------------------------- CPU 3: arguments

def test_entry_points_check_arguments_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    f, odd, odd4 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # never dereferenced: every call below fails its checks first
    assert C.sizeof(L.RawSample) == 6 * 4 + 3 * 4 + 4 + 3 * 8

    def pack(frames=f, N=2, H2=64, W2=96, maps=(None, None, None, None), mh=0, mw=0, table=f, mode=0, flags=1, black=512.0, white=16383.0, out=f,
             clean=None, B=2, h=16, w=24):
        return lib.nd_raw_pack_u16_f32(frames, N, H2, W2, *maps, mh, mw, table, mode, flags, black, white, out, clean, B, h, w, None)

    m4 = (f, f, f, f)
    assert pack(frames=None) == -1 and pack(table=None) == -1 and pack(out=None) == -1 and pack(mode=3) == -1 and pack(flags=4) == -1
    assert pack(N=0) == -1 and pack(B=0) == -1 and pack(B=65536) == -1 and pack(h=0) == -1 and pack(white=512.0) == -1 and pack(white=70000.0) == -1
    assert pack(clean=f) == -1 and pack(mode=2) == -1 and pack(mode=1) == -1 and pack(maps=m4, mh=32, mw=48) == -1
    assert pack(maps=(f, f, f, None), mode=1, mh=32, mw=48) == -1
    assert b"all four" in lib.nd_last_error()
    assert pack(H2=63) == -2 and pack(W2=95) == -2 and pack(h=33) == -2 and pack(w=49) == -2
    assert pack(maps=m4, mode=1, mh=15, mw=48) == -2 and pack(maps=m4, mode=2, clean=f, mh=32, mw=23) == -2
    assert pack(frames=odd) == -3 and pack(table=odd4) == -3 and pack(out=odd) == -3 and pack(mode=2, clean=odd) == -3
    assert pack(maps=(f, odd, f, f), mode=1, mh=32, mw=48) == -3

    def pg(frames=f, N=2, H2=64, W2=96, table=f, rng=None, draw=0, cin=None, nin=None, cout=None, nout=None, black=512.0, white=16383.0, noisy=f,
           clean=f, B=2, h=16, w=24):
        return lib.nd_raw_poisson_gaussian_f32(frames, N, H2, W2, table, rng, 1, 0, draw, cin, nin, cout, nout, black, white, noisy, clean, B, h, w, None)

    assert pg(frames=None) == -1 and pg(table=None) == -1 and pg(noisy=None) == -1 and pg(clean=None) == -1 and pg(draw=-1) == -1 and pg(B=0) == -1
    assert pg(black=-1.0) == -1 and pg(H2=62, h=32) == -2 and pg(W2=95) == -2 and pg(w=50) == -2
    assert pg(frames=odd) == -3 and pg(table=odd4) == -3 and pg(rng=odd4) == -3 and pg(noisy=odd) == -3 and pg(cin=odd) == -3 and pg(nout=odd) == -3
    bl = (C.c_int32 * 4)(512, 512, 512, 512)
    tb = lib.nd_raw_to_bayer_u16
    assert tb(None, f, bl, 16383, 1, 8, 8, None) == -1 and tb(f, None, bl, 16383, 1, 8, 8, None) == -1 and tb(f, f, None, 16383, 1, 8, 8, None) == -1
    assert tb(f, f, bl, 16383, 0, 8, 8, None) == -1 and tb(f, f, bl, 70000, 1, 8, 8, None) == -1 and tb(f, f, bl, 500, 1, 8, 8, None) == -1
    assert tb(f, f, (C.c_int32 * 4)(512, -1, 512, 512), 16383, 1, 8, 8, None) == -1
    assert tb(odd, f, bl, 16383, 1, 8, 8, None) == -3 and tb(f, odd, bl, 16383, 1, 8, 8, None) == -3


def test_builders_refuse_bad_parameters_on_the_host():
    from noisediff_amd import _lib as L, raw
    with pytest.raises(ValueError):
        raw.RealBatchBuilder(crop=0)
    b = raw.RealBatchBuilder(crop=16)
    shape = (2, 64, 96)
    ok = dict(short=[0, 1], long=[1, 0], xy=[(0, 0), (32, 16)], iso=[800, 3200], ratio=[100, 250], flip=[1, 0])
    host = b.check(2, shape, **ok)
    rows = host[32:].view(raw.ROW)
    assert rows["x0"].tolist() == [0, 32] and rows["branch"].tolist() == [0, 1] and rows["frame_clean"].tolist() == [1, 0] and rows["flip"].tolist() == [1, 0]
    b.check(2, shape, **{**ok, "xy": [(3, 5), (31, 15)]})                                      # any integer origin inside the frame
    for change in ({"xy": [(0, 0), (33, 16)]}, {"xy": [(0, 17), (0, 0)]}, {"xy": [(-1, 0), (0, 0)]}, {"short": [0, 2]}, {"long": [-1, 0]},
                   {"ratio": [0, 250]}, {"ratio": [100, NAN]}, {"iso": [800]}, {"xy": [(0, 0)]}):
        with pytest.raises(ValueError):
            b.check(2, shape, **{**ok, **change})
    for bad_shape in ((2, 63, 96), (2, 64, 95), (2, 30, 96), (64,)):
        with pytest.raises(ValueError):
            b.check(2, bad_shape, **ok)
    p = raw.PoissonGaussianBatchBuilder(crop=16)
    okp = dict(frame=[0, 1], xy=[(0, 0), (32, 16)], ratio=[100, 300], k=[0.76, 24.5], var=[2.5, 0.0])
    host = p.check(2, shape, **okp, seed=(5 << 32) + 7, first_sample=3, draw=2)
    assert host[:32].view(np.int64)[:3].tolist() == [(5 << 32) + 7, 3, 2] and host[32:].view(raw.ROW)["sd"].tolist() == [math.sqrt(2.5), 0.0]
    for change in ({"k": [0.0, 24.5]}, {"k": [0.76, -1.0]}, {"var": [-0.1, 0.0]}, {"ratio": [100, 0]}, {"ratio": [-100, 300]}, {"frame": [0, 2]},
                   {"xy": [(0, 0), (33, 16)]}, {"draw": -1}):
        with pytest.raises(ValueError):
            p.check(2, shape, **{**okp, **change})
    p.check(2, shape, **{**okp, "k": [1e-5, 24.5]})                  # 15871 / (100 * 1e-5) = 1.6e7 < 2^24: counts stay exact
    with pytest.raises(ValueError, match="2\\*\\*24"):
        p.check(2, shape, **{**okp, "k": [9e-6, 24.5]})              # 15871 / (100 * 9e-6) = 1.76e7 >= 2^24
    frames = np.zeros(shape, np.uint16)
    with pytest.raises(L.HipError):
        b(torch.zeros(shape, dtype=torch.int16), **ok)
    with pytest.raises(L.HipError):
        p(torch.zeros(shape, dtype=torch.int16), **okp)
    with pytest.raises(L.HipError):
        raw.pack_raw(torch.zeros(shape, dtype=torch.int16))
    with pytest.raises(L.HipError):
        raw.to_bayer(torch.zeros(1, 4, 8, 8), [512] * 4)
    with pytest.raises(L.HipError):
        raw.frames_on_device(frames, "cpu")
    with pytest.raises(TypeError):
        raw.frames_on_device(frames.astype(np.int32))
    with pytest.raises(ValueError):
        raw.to_bayer(torch.zeros(1, 3, 8, 8), [512] * 4)
    with pytest.raises(ValueError):
        raw.to_bayer(torch.zeros(1, 4, 8, 8), [512, 512, 512])
    with pytest.raises(ValueError):
        raw.load_pair(frames[0], frames[1], 800, 0)


def test_random_params_and_truncated_normals_draw_as_documented():
    from noisediff_amd import raw
    b, p = raw.RealBatchBuilder(crop=16), raw.PoissonGaussianBatchBuilder(crop=16)
    state = np.random.get_state()
    try:
        for seed in range(6):
            for builder in (b, p):
                np.random.seed(seed)
                got = builder.random_params(3, (32, 48))
                np.random.seed(seed)
                xy = []
                for _ in range(3):
                    x = np.random.randint(0, 48 - 16 + 1)
                    y = np.random.randint(0, 32 - 16 + 1)
                    xy.append((x // 2 * 2, y // 2 * 2))
                flip = np.random.randint(0, 2)
                assert got == {"xy": xy, "flip": [flip] * 3}
                after = np.random.randint(1 << 30)
                np.random.seed(seed)
                builder.random_params(3, (32, 48))
                assert np.random.randint(1 << 30) == after                  # no draw more and none less
        np.random.seed(11)
        ks = np.array([raw.poisson_gaussian_params(3.0, 0.5) for _ in range(4000)])
        assert (ks[:, 0] >= 2.1).all() and (ks[:, 0] <= 3.9).all() and (ks[:, 1] >= 0.35).all() and (ks[:, 1] <= 0.65).all()
        # N(3, 1) truncated to [2.1, 3.9]: mean 3, variance 1 - 2 a phi(a) / (2 Phi(a) - 1) at a = 0.9
        a, phi, Phi = 0.9, math.exp(-0.405) / math.sqrt(2 * math.pi), 0.5 * (1 + math.erf(0.9 / math.sqrt(2)))
        var = 1 - 2 * a * phi / (2 * Phi - 1)
        assert abs(ks[:, 0].mean() - 3.0) < 5 * math.sqrt(var / 4000) and abs(ks[:, 0].var() - var) < 0.1 * var
        assert abs(ks[:, 1].mean() - 0.5) < 5 * 0.15 / math.sqrt(3 * 4000)                   # nearly uniform on [0.35, 0.65]
        with pytest.raises(ValueError):
            raw.poisson_gaussian_params(0.0, 1.0)
    finally:
        np.random.set_state(state)


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


def _u16(t):
    return _np(t.view(torch.int16) if t.dtype != torch.int16 else t).view(np.uint16)


def _dev_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).to(DEV)


def _maps(seed, H2, W2, tag):
    rng = {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}
    return {k: synth.uniform(seed, f"raw.t.{tag}.{k}", (H2, W2), lo, hi).numpy() for k, (lo, hi) in rng.items()}


def _shading(bayer):
    from noisediff_amd import denoise_data as dd
    return dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], BLC, DEV), {k: R.pack_planes(v) for k, v in bayer.items()}


def _launch_pack(frames_dev, rows, mode, flags, sh, h, w, pad=3):
    """nd_raw_pack_u16_f32 into NaN-filled outputs `pad` samples longer than the kernel writes; returns (out, clean or None) as numpy, the written
    part, after checking that the rest is still NaN."""
    from noisediff_amd import _lib as L, raw
    from noisediff_amd._host import _stream
    B = len(rows)
    N, H2, W2 = frames_dev.shape
    real = mode == L.RAW_TRAIN_REAL
    out = torch.full((B + pad, 4, h, w), NAN, device=DEV)
    clean = torch.full((B + pad, 4, h, w), NAN, device=DEV) if real else None
    maps, mh, mw = raw._plane_ptrs(sh, DEV)
    table = torch.from_numpy(rows.view(np.uint8)).to(DEV)
    L.call("nd_raw_pack_u16_f32", frames_dev.data_ptr(), N, H2, W2, *maps, mh, mw, table.data_ptr(), mode, flags, 512.0, 16383.0, out.data_ptr(),
           L.ptr(clean), B, h, w, _stream(DEV))
    torch.cuda.synchronize()
    res = []
    for t in (out, clean):
        if t is None:
            res.append(None)
            continue
        a = _np(t)
        assert np.isnan(a[B:]).all(), "the kernel wrote past its output"
        res.append(a[:B])
    return res


def _rows(specs, blc=BLC):
    """specs: (frame, frame_clean, x0, y0, flip, iso, ratio) per sample."""
    from noisediff_amd import raw
    rows = np.zeros(len(specs), raw.ROW)
    for r, (fr, fc, x0, y0, flip, iso, ratio) in zip(rows, specs):
        r["frame"], r["frame_clean"], r["x0"], r["y0"], r["flip"], r["iso"], r["ratio"] = fr, fc, x0, y0, flip, iso, ratio
        r["branch"], r["blc"] = iso > 1600, blc.get(iso, 0.0)
    return rows


def _check_pack_sample(got, got_clean, frames, spec, mode, planes, h, w, what):
    fr, fc, x0, y0, flip, iso, ratio = spec
    name = {0: "pack", 1: "shaded", 2: "real"}[mode]
    want = ref_pack(name, frames[fr], x0, y0, h, w, flip, ratio, iso, planes)
    assert got.dtype == np.float32 and np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} elements differ"
    if mode == 2:
        assert np.array_equal(got_clean, ref_pack("pack", frames[fc], x0, y0, h, w, flip, 1, 0, clip=False)), what


@pytest.mark.gpu
def test_every_uint16_code_through_the_three_pack_modes():
    from noisediff_amd import _lib as L
    perm = np.argsort(synth.uniform01(5, "raw.t.codes", 65536), kind="stable").astype(np.uint16)
    assert np.array_equal(np.sort(perm), np.arange(65536, dtype=np.uint16))
    frames = np.stack([perm.reshape(256, 256), perm[::-1].reshape(256, 256)])
    sh, planes = _shading(_maps(5, 256, 256, "codes"))
    fd = _dev_frames(frames)
    for ratio, iso in CASES:
        spec = [(0, 1, 0, 0, 0, iso, ratio)]
        for mode, flags, use in ((L.RAW_PACK, L.RAW_RESCALE | L.RAW_CLIP, False), (L.RAW_PACK_SHADED, 0, True), (L.RAW_TRAIN_REAL, 0, True),
                                 (L.RAW_TRAIN_REAL, 0, False)):
            out, clean = _launch_pack(fd, _rows(spec), mode, flags, sh if use else None, 128, 128)
            _check_pack_sample(out[0], None if clean is None else clean[0], frames, spec[0], mode, planes if use else None, 128, 128,
                               f"mode {mode} shading {use} ratio {ratio} iso {iso}")
    for rescale in (True, False):                   # pack_raw itself: no clip
        out, _ = _launch_pack(fd, _rows([(1, 0, 0, 0, 0, 0, 1)]), L.RAW_PACK, L.RAW_RESCALE if rescale else 0, None, 128, 128)
        assert np.array_equal(out[0], R.pack(R.codes(frames[1]), rescale))


ADDRESSING = {
    "whole_frame_vector_path": ((136, 208), 68, 104, [(0, 1, 0, 0, 0, 800, 100)]),
    "rows_off_16_bytes_and_odd_width": ((66, 94), 33, 47, [(1, 0, 0, 0, 1, 25600, 300)]),
    "window_8_4": ((136, 208), 24, 40, [(0, 1, 8, 4, 0, 1600, 250)]),
    "window_6_5": ((136, 208), 24, 40, [(1, 0, 6, 5, 1, 800, 100)]),
    "window_3_2": ((136, 208), 24, 40, [(0, 0, 3, 2, 0, 25600, 300)]),
    "width_2_mod_4": ((136, 208), 24, 42, [(0, 1, 5, 7, 1, 800, 100)]),
    "two_workgroups_on_each_axis": ((136, 208), 36, 64, [(0, 1, 40, 32, 0, 800, 100), (1, 0, 7, 0, 1, 25600, 300)]),      # 36 * 16 = 576 threads > 256
    "three_samples_of_two_frames": ((136, 208), 24, 40, [(0, 1, 8, 4, 0, 800, 100), (1, 0, 31, 17, 1, 25600, 300), (1, 1, 64, 44, 0, 1600, 250)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ADDRESSING))
def test_pack_addressing(case):
    from noisediff_amd import _lib as L
    (H2, W2), h, w, specs = ADDRESSING[case]
    frames = np.floor(synth.uniform(9, f"raw.t.addr.{H2}", (2, H2, W2), 300.0, 2000.0).numpy()).astype(np.uint16)
    sh, planes = _shading(_maps(9, H2, W2, f"addr.{H2}"))
    fd = _dev_frames(frames)
    for mode, flags, use in ((L.RAW_PACK, L.RAW_RESCALE | L.RAW_CLIP, False), (L.RAW_PACK_SHADED, 0, True), (L.RAW_TRAIN_REAL, 0, True)):
        out, clean = _launch_pack(fd, _rows(specs), mode, flags, sh if use else None, h, w)
        for b, spec in enumerate(specs):
            _check_pack_sample(out[b], None if clean is None else clean[b], frames, spec, mode, planes if use else None, h, w, f"{case} mode {mode} b {b}")
            alone, alone_clean = _launch_pack(fd, _rows([spec]), mode, flags, sh if use else None, h, w)
            assert np.array_equal(alone[0], out[b]) and (clean is None or np.array_equal(alone_clean[0], clean[b]))         # the batch does not matter


@pytest.mark.gpu
def test_a_table_row_outside_the_frame_gives_nan_for_that_sample_only():
    from noisediff_amd import _lib as L
    frames = np.floor(synth.uniform(9, "raw.t.addr.136", (2, 136, 208), 300.0, 2000.0).numpy()).astype(np.uint16)
    sh, planes = _shading(_maps(9, 136, 208, "addr.136"))
    fd = _dev_frames(frames)
    good = (0, 1, 8, 4, 1, 800, 100)
    for bad in ((0, 1, 65, 4, 0, 800, 100), (0, 1, 8, 45, 0, 800, 100), (0, 1, -1, 4, 0, 800, 100), (2, 1, 8, 4, 0, 800, 100), (-1, 1, 8, 4, 0, 800, 100)):
        out, clean = _launch_pack(fd, _rows([good, bad, good]), L.RAW_TRAIN_REAL, 0, sh, 24, 40)
        assert np.isnan(out[1]).all() and np.isnan(clean[1]).all()
        for b in (0, 2):
            _check_pack_sample(out[b], clean[b], frames, good, 2, planes, 24, 40, f"next to {bad}")
    out, clean = _launch_pack(fd, _rows([good, (0, 2, 8, 4, 0, 800, 100)]), L.RAW_TRAIN_REAL, 0, sh, 24, 40)        # the clean frame index
    assert np.isnan(out[1]).all() and np.isnan(clean[1]).all() and np.isfinite(out[0]).all()


@pytest.mark.gpu
def test_public_pack_raw_and_load_pair_equal_the_reference_goldens(gold):
    from noisediff_amd import raw
    z, f = gold.z, gold.frames
    sh, _ = _shading(gold.bayer)
    assert np.array_equal(_np(raw.pack_raw(f["long"]))[0], z["pack_raw.long.1"])
    assert np.array_equal(_np(raw.pack_raw(_dev_frames(f["short"]), rescale=False))[0], z["pack_raw.short.0"])
    both = _np(raw.pack_raw(np.stack([f["short"], f["long"]])))
    assert both.shape == (2, 4, 68, 104) and np.array_equal(both[1], z["pack_raw.long.1"])
    for i, (ratio, iso) in enumerate(CASES):
        noisy, clean = raw.load_pair(f["short"], f["long"], iso, ratio, sh)
        assert noisy.shape == (1, 4, 68, 104) and np.array_equal(_np(noisy)[0], z[f"load_image.{i}.1.noisy"])
        assert np.array_equal(_np(clean)[0], z["load_image.clean"])
        noisy, _ = raw.load_pair(_dev_frames(f["short"]), _dev_frames(f["long"]), iso, ratio)
        assert np.array_equal(_np(noisy)[0], z[f"load_image.{i}.0.noisy"])
        for sub in (1, 0):
            b = raw.RealBatchBuilder(gold.crop, sh if sub else None)
            x0, y0 = (int(v) for v in z[f"real.{i}.{sub}.xy"])
            n, c = b(np.stack([f["short"], f["long"]]), [0], [1], [(x0, y0)], [iso], [ratio])
            assert np.array_equal(_np(n)[0], z[f"real.{i}.{sub}.noisy"]) and np.array_equal(_np(c)[0], z[f"real.{i}.{sub}.clean"])


def _pg_frames(n=2, H2=160, W2=200, seed=21):
    fr = np.floor(synth.uniform(seed, "raw.t.pg", (n, H2, W2), 0.0, 16384.0).numpy()).astype(np.uint16)
    return fr


def _launch_pg(frames_dev, builder, prm, key, counts=None, normals=None, pad=1):
    """PoissonGaussianBatchBuilder.launch into NaN-filled buffers one sample longer than written; (noisy, clean, counts_out, normals_out) numpy."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    B, c = len(prm["frame"]), builder.crop
    host = builder.check(B, tuple(frames_dev.shape), **prm, **key)
    block = torch.from_numpy(host).to(DEV)
    bufs = [torch.full((B + pad, 4, c, c), NAN, device=DEV) for _ in range(4)]
    N, H2, W2 = frames_dev.shape
    L.call("nd_raw_poisson_gaussian_f32", frames_dev.data_ptr(), N, H2, W2, block.data_ptr() + 32, None, key["seed"], key["first_sample"], key["draw"],
           L.ptr(counts), L.ptr(normals), bufs[2].data_ptr(), bufs[3].data_ptr(), 512.0, 16383.0, bufs[0].data_ptr(), bufs[1].data_ptr(), B, c, c,
           _stream(DEV))
    torch.cuda.synchronize()
    res = [_np(t) for t in bufs]
    assert all(np.isnan(a[B:]).all() for a in res), "the kernel wrote past its output"
    return [a[:B] for a in res]


@pytest.mark.gpu
def test_poisson_gaussian_from_explicit_counts_and_normals_is_bitwise():
    from noisediff_amd import raw
    frames = _pg_frames()
    fd = _dev_frames(frames)
    b = raw.PoissonGaussianBatchBuilder(64)
    prm = dict(frame=[1, 0], xy=[(3, 2), (36, 16)], ratio=[100, 300], k=[0.76504, 24.48128], var=[2.5, 900.0], flip=[0, 1])
    counts = synth.uniform(21, "raw.t.pg.counts", (2, 4, 64, 64), 0.0, 300.0).numpy()
    counts[1] *= 0.01                                         # sample 1 (k = 24.5, ratio 300) is white at three counts: keep it inside [0, 1] as well
    counts = np.floor(counts).astype(np.float32)
    normals = synth.normal(21, "raw.t.pg.normals", (2, 4, 64, 64)).numpy().astype(np.float32)
    noisy, clean, cout, nout = _launch_pg(fd, b, prm, dict(seed=1, first_sample=0, draw=0), torch.from_numpy(counts).to(DEV), torch.from_numpy(normals).to(DEV))
    assert np.array_equal(cout, counts) and np.array_equal(nout, normals)
    for i in range(2):
        x = R.window(R.codes(frames[prm["frame"][i]]), *prm["xy"][i], 64, 64, prm["flip"][i])
        want = R.pg_noisy(counts[i], normals[i], prm["k"][i], math.sqrt(prm["var"][i]), prm["ratio"][i])
        assert np.array_equal(noisy[i], want), f"sample {i}: {int((noisy[i] != want).sum())} differ"
        assert np.array_equal(clean[i], R.pg_clean(x))
        assert float((want > 0).mean()) > 0.3 and float((want < 1).mean()) > 0.3
    n2, c2 = b(fd, **prm, counts=torch.from_numpy(counts).to(DEV), normals=torch.from_numpy(normals).to(DEV))          # the public call
    assert np.array_equal(_np(n2), noisy) and np.array_equal(_np(c2), clean)


PG_CASES = [(100, 0.76504), (250, 1.53008), (300, 24.48128), (300, 0.047815)]


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,k", PG_CASES)
def test_poisson_gaussian_drawn(ratio, k):
    from noisediff_amd import raw
    frames = _pg_frames(4, 96, 160, seed=23)
    frames[:, 0, :128] = 512                                  # the first 64 elements of every sample sit at the black level: rate 0
    fd = _dev_frames(frames)
    h, w, var = 48, 80, 4.0
    b = raw.PoissonGaussianBatchBuilder(48)                   # the builder is square; the 48 x 80 windows go through the entry point below
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    rows = np.zeros(4, raw.ROW)
    rows["frame"], rows["k"], rows["sd"], rows["ratio64"], rows["ratio"] = np.arange(4), k, math.sqrt(var), ratio, ratio
    table = torch.from_numpy(rows.view(np.uint8)).to(DEV)
    key = dict(seed=(7 << 32) + 99, first_sample=5, draw=3)

    def run(tab, B, cin=None, nin=None, **over):
        kk = {**key, **over}
        bufs = [torch.full((B + 1, 4, h, w), NAN, device=DEV) for _ in range(4)]
        L.call("nd_raw_poisson_gaussian_f32", fd.data_ptr(), 4, 96, 160, tab.data_ptr(), None, kk["seed"], kk["first_sample"], kk["draw"], L.ptr(cin),
               L.ptr(nin), bufs[2].data_ptr(), bufs[3].data_ptr(), 512.0, 16383.0, bufs[0].data_ptr(), bufs[1].data_ptr(), B, h, w, _stream(DEV))
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t[B:]).all()) for t in bufs)
        return bufs

    noisy, clean, cout, nout = run(table, 4)
    differ, n_el = 0, 4 * h * w
    for i in range(4):
        x = R.codes(frames[i])[:, :h, :w]
        c, lam = R.pg_rate(x, ratio, k)
        assert (lam.reshape(-1)[:64] == 0).all()
        want_n = R.poisson(lam, key["seed"], key["first_sample"] + i, key["draw"])
        got_n = _np(cout[i]).reshape(-1)
        differ += int((got_n != want_n).sum())
        assert (got_n[:64] == 0).all()
        z64 = R.normal64(key["seed"], key["first_sample"] + i, key["draw"], n_el)
        got_z = _np(nout[i]).reshape(-1)
        want_z = z64.astype(np.float32)
        bound = 8 * 2.0 ** -53 * np.maximum(1.0, np.abs(z64))
        ez = np.abs(got_z.astype(np.float64) - want_z.astype(np.float64))
        want = R.pg_noisy(want_n, want_z, k, math.sqrt(var), ratio).reshape(-1)
        same = got_n == want_n
        en = np.abs(_np(noisy[i]).reshape(-1).astype(np.float64) - want.astype(np.float64))[same]
        print(f"ratio {ratio} k {k} sample {i}: normals max err/bound {(ez / bound).max():.3f}, noisy max err {en.max():.3e} (bound {2.0 ** -24:.3e}), "
              f"lam max {lam.max():.1f}")
        assert (ez <= bound).all()
        assert (en <= 2.0 ** -24).all()
        assert np.array_equal(_np(clean[i]), R.pg_clean(x))
    print(f"ratio {ratio} k {k}: {differ} of {4 * n_el} counts differ from the restatement")
    assert differ <= 1
    again = run(table, 4)
    assert all(torch.equal(a[:4], g[:4]) for a, g in zip(again, (noisy, clean, cout, nout)))                         # a repeated call
    fed = run(table, 4, cin=cout[:4].contiguous(), nin=nout[:4].contiguous(), seed=1, first_sample=0, draw=0)      # the draws fed back: the key is idle
    assert torch.equal(fed[0][:4], noisy[:4]) and torch.equal(fed[2][:4], cout[:4]) and torch.equal(fed[3][:4], nout[:4])
    alone = run(torch.from_numpy(rows[2:3].copy().view(np.uint8)).to(DEV), 1, first_sample=key["first_sample"] + 2)
    assert all(torch.equal(a[0], g[2]) for a, g in zip(alone, (noisy, clean, cout, nout)))                           # a sample alone
    for other in (dict(seed=key["seed"] + 1), dict(seed=key["seed"] + (1 << 32)), dict(draw=4), dict(first_sample=6)):
        o = run(table, 4, **other)
        assert not torch.equal(o[2][:4], cout[:4]) and not torch.equal(o[3][:4], nout[:4]), other
    assert b.crop == 48


@pytest.mark.gpu
def test_bayer_write_is_bitwise():
    from noisediff_amd import raw
    j = np.arange(15872, dtype=np.float64)
    edge = (j / 15871).astype(np.float32)
    vals = np.concatenate([edge, np.nextafter(edge, np.float32(-1)), np.nextafter(edge, np.float32(2)),
                           np.array([-1.0, -0.0, 0.0, 1.0, 1.5, NAN, np.inf, -np.inf, 1e-30, 0.5], np.float32)])
    h, w = 72, 96
    n = 4 * h * w
    reps = -(-2 * n // vals.size)
    flat = np.tile(vals, reps)[:2 * n]
    flat = flat[np.argsort(synth.uniform01(3, "raw.t.bayer", flat.size), kind="stable")]
    img = flat.reshape(2, 4, h, w)
    assert vals.size <= n * 2 and np.isnan(img).any()
    for bl in ([512, 512, 512, 512], [510, 512, 514, 512]):
        out = torch.zeros(3, 2 * h, 2 * w, dtype=torch.int16, device=DEV)
        got = raw.to_bayer(torch.from_numpy(img).to(DEV), bl, out=out[:2])
        torch.cuda.synchronize()
        g = _u16(out)
        assert got.data_ptr() == out.data_ptr() and (g[2] == 0).all()
        for b in range(2):
            want = R.to_bayer(img[b], bl)
            assert np.array_equal(g[b], want), f"bl {bl}: {int((g[b] != want).sum())} codes differ"
    odd = synth.uniform(3, "raw.t.bayer.odd", (1, 4, 33, 47), -0.1, 1.1)                       # scalar path; and the allocation of the public call
    got = raw.to_bayer(odd.to(DEV), [510, 512, 514, 512])
    assert tuple(got.shape) == (1, 66, 94) and np.array_equal(_u16(got)[0], R.to_bayer(odd.numpy()[0], [510, 512, 514, 512]))
    two = synth.uniform(3, "raw.t.bayer.two", (4, 34, 46), -0.1, 1.1)                          # 8-byte path
    assert np.array_equal(_u16(raw.to_bayer(two.to(DEV), [512] * 4))[0], R.to_bayer(two.numpy(), [512] * 4))


@pytest.mark.gpu
def test_captured_launches_replay_with_rewritten_tables():
    """One launch in each graph; the device block is rewritten between replays."""
    from noisediff_amd import raw
    frames = np.floor(synth.uniform(9, "raw.t.graph", (2, 136, 208), 300.0, 4000.0).numpy()).astype(np.uint16)
    sh, _ = _shading(_maps(9, 136, 208, "graph"))
    fd = _dev_frames(frames)
    shape, c = tuple(fd.shape), 32
    rb, pb = raw.RealBatchBuilder(c, sh), raw.PoissonGaussianBatchBuilder(c)
    r1 = dict(short=[0, 1], long=[1, 0], xy=[(0, 0), (72, 36)], iso=[800, 25600], ratio=[100, 300], flip=[1, 0])
    r2 = dict(short=[1, 1], long=[0, 0], xy=[(7, 3), (20, 30)], iso=[1600, 800], ratio=[250, 100], flip=[0, 0])
    p1 = dict(frame=[0, 1], xy=[(0, 0), (72, 36)], ratio=[100, 300], k=[0.76504, 24.48128], var=[2.5, 900.0], flip=[1, 0], seed=1, first_sample=0, draw=0)
    p2 = dict(frame=[1, 1], xy=[(5, 9), (40, 2)], ratio=[250, 300], k=[1.53008, 0.047815], var=[6.0, 0.0], flip=[0, 1], seed=(9 << 32) + 2,
              first_sample=40, draw=7)
    ri, pi = rb.capture_inputs(2, DEV), pb.capture_inputs(2, DEV)
    rb.update(ri, shape, **r1)
    pb.update(pi, shape, **p1)
    bufs = [torch.empty(2, 4, c, c, device=DEV) for _ in range(6)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rb.launch(ri, fd, bufs[0], bufs[1])
        pb.launch(pi, fd, bufs[2], bufs[3], counts_out=bufs[4], normals_out=bufs[5])
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr, gp = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        rb.launch(ri, fd, bufs[0], bufs[1])
    with torch.cuda.graph(gp):
        pb.launch(pi, fd, bufs[2], bufs[3], counts_out=bufs[4], normals_out=bufs[5])
    for rp, pp in ((r1, p1), (r2, p2), (r1, p2)):
        rb.update(ri, shape, **rp)
        pb.update(pi, shape, **pp)
        for t in bufs:
            t.fill_(NAN)
        gr.replay()
        gp.replay()
        torch.cuda.synchronize()
        want = rb(fd, **rp) + pb(fd, **pp, return_draws=True)
        assert all(torch.equal(a, b) for a, b in zip(bufs, want))
    assert float(bufs[4].abs().max()) > 0


@pytest.mark.gpu
def test_evaluate_raw_scores_a_full_size_frame_as_evaluate_does():
    from noisediff_amd import LSID, io, metrics
    from noisediff_amd.spec import lsid_param_spec
    H, W = io.PACKED_H, io.PACKED_W
    ratio, iso = 250, 25600
    long = np.floor(synth.uniform(31, "raw.t.full.long", (2 * H, 2 * W), 400.0, 17500.0).clamp(max=16383.0).numpy()).astype(np.uint16)
    short = np.floor(512.0 + (long.astype(np.float64) - 512.0) / ratio + 3.0 * synth.normal(31, "raw.t.full.noise", (2 * H, 2 * W)).numpy())
    short = np.clip(short, 0, 16383).astype(np.uint16)
    bayer = _maps(31, 2 * H, 2 * W, "full")
    sh, planes = _shading(bayer)
    net = LSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    net = net.to(DEV).eval()
    sd, ld = _dev_frames(short), _dev_frames(long)
    clean = torch.from_numpy(ref_pack("pack", long, 0, 0, H, W, 0, 1, 0)[None]).to(DEV)
    for use in (True, False):
        noisy = ref_pack("shaded" if use else "pack", short, 0, 0, H, W, 0, ratio, iso, planes if use else None)
        want = metrics.evaluate(net, torch.from_numpy(noisy[None]).to(DEV), clean)
        got = metrics.evaluate_raw(net, sd, ld, iso, ratio, sh if use else None)
        for key in ("PSNR", "SSIM", "MSE"):
            assert got[key].shape == (1,) and got[key].tobytes() == want[key].tobytes(), (use, key, got[key], want[key])
        assert np.isfinite(got["PSNR"]).all()


@pytest.mark.gpu
def test_a_training_step_runs_on_a_real_and_on_a_poisson_gaussian_batch():
    import torch.nn.functional as F
    from noisediff_amd import TrainableLSID, raw, train
    from noisediff_amd.spec import lsid_param_spec
    frames = np.floor(synth.uniform(9, "raw.t.step", (2, 160, 200), 400.0, 3000.0).numpy()).astype(np.uint16)
    sh, _ = _shading(_maps(9, 160, 200, "step"))
    fd = _dev_frames(frames)
    state = np.random.get_state()
    try:
        np.random.seed(3)
        rb, pb = raw.RealBatchBuilder(64, sh), raw.PoissonGaussianBatchBuilder(64)
        rp, pp = rb.random_params(2, (80, 100)), pb.random_params(2, (80, 100))
        k, var = raw.poisson_gaussian_params(0.76504, 2.5)
    finally:
        np.random.set_state(state)
    batches = [rb(fd, [0, 1], [1, 0], iso=[800, 25600], ratio=[100, 300], **rp), pb(fd, [0, 1], ratio=[100, 300], k=k, var=var, seed=5, **pp)]
    net = TrainableLSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    net = net.to(DEV).hip()
    opt = train.Adam(net.parameters(), lr=1e-4)
    for noisy, target in batches:
        assert noisy.shape == (2, 4, 64, 64) and torch.isfinite(noisy).all() and torch.isfinite(target).all() and float(noisy.std()) > 0
        opt.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(noisy), target)
        loss.backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        opt.step()
        torch.cuda.synchronize()
        assert math.isfinite(float(loss.detach())) and float(loss.detach()) > 0
