"""noisediff_amd.denoise_data: the denoiser's training batch (compose, dark shading, crop, flip, shot-noise augmentation) in one HIP launch.

CPU: the numpy restatement (tests/denoise_data_ref.py) equals the reference's own functions (tests/golden/denoise_data.npz, captured by
tests/golden/capture_denoise_data.py) bit for bit in float32 and within the device's bound in float64; the augmentation's host parameters equal
the reference's; the numpy Philox-Poisson draw passes mean / variance / chi-square / correlation tests; bad arguments are refused without a GPU.
GPU: the device draw equals the restatement element for element; the batch equals the float64 restatement and the reference goldens within
the fp32 bounds; the drawn path is replayable and batch-independent; the launch captures into a graph; a training step runs on a built batch."""
import ctypes as C
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import denoise_data_ref as R
from noisediff_amd import synth

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E24 = 2.0 ** -24
RATES = [0.01, 0.3, 1.0, 3.7, 9.99, 10.0, 12.5, 40.0, 300.0, 6640.0, 1e5]
N_STAT = 1 << 20


def exact_sum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def shading_bound(ratio):
    """The fp32 evaluation's rounding at magnitude 512 + 15871 / ratio, scaled back by ratio / 15871."""
    return 8 * E24 * (1 + 512 * ratio / 15871)


def sna_bound(ref):
    return 4 * E24 * np.maximum(1.0, np.abs(ref))


def batch_bounds(ratio, shading, sna, ref_noisy, ref_clean):
    """(bound on noisy, bound on clean_out) against the float64 restatement.  Neither stage: noisy is one fp32 addition of magnitude < 2
    (half an ulp: 2^-24) and clean_out a clip (exact)."""
    if not shading and not sna:
        return np.full(ref_noisy.shape, E24), np.zeros(ref_clean.shape)
    bn = np.full(ref_noisy.shape, shading_bound(ratio) if shading else 0.0)
    if sna:
        return bn + sna_bound(ref_noisy), sna_bound(ref_clean)
    return bn, np.zeros(ref_clean.shape)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "sna_gain.json")) as f:
        meta = json.load(f)
    return SimpleNamespace(z=np.load(os.path.join(GOLDEN, "denoise_data.npz")), meta=meta["meta"], gains=meta["gains"])


def _maps(meta):
    """The four synthetic Bayer maps of the capture, as planes (4, H, W)."""
    s, (fh, fw) = meta["seed"], meta["frame"]
    rng = {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}
    bayer = {k: synth.uniform(s, f"dd.ds_{k}", (2 * fh, 2 * fw), lo, hi).numpy() for k, (lo, hi) in rng.items()}
    return bayer, {k: R.pack_planes(v) for k, v in bayer.items()}


def _case_inputs(meta, i):
    s, P = meta["seed"], meta["patch"]
    noise = (0.2 * synth.normal(s, f"dd.noise.{i}", (4, P, P))).numpy()
    clean = synth.uniform(s, f"dd.clean.{i}", (4, P, P), -0.05, 1.1).numpy()
    return noise, clean


def _case_counts(meta, i):
    return np.floor(synth.uniform(meta["seed"], f"dd.counts.{i}", (4, meta["crop"], meta["crop"]), 0.0, 64.0).numpy())


def _blc(meta):
    return {int(k): v for k, v in meta["blc_mean"].items()}


# --------------------------------------------------------------------------- CPU 1: the restatement against the reference

@pytest.mark.parametrize("i", [0, 1, 2])
def test_restated_dark_shading_equals_the_reference(gold, i):
    meta = gold.meta
    ratio, iso, (x0, y0) = meta["cases"][i]
    P, st = meta["patch"], meta["step"]
    noise, clean = _case_inputs(meta, i)
    _, planes = _maps(meta)
    pair = "high" if iso > 1600 else "low"
    dk, db = planes["k_" + pair][:, y0:y0 + P, x0:x0 + P], planes["b_" + pair][:, y0:y0 + P, x0:x0 + P]
    want = gold.z[f"shaded.{i}"]
    v32, _ = R.compose(noise, clean, np.float32)
    got32 = R.remove_dark_shading(v32, ratio, iso, dk, db, _blc(meta)[iso], np.float32)
    assert got32.dtype == np.float32
    assert np.array_equal(got32[:, ::st, ::st], want)
    assert exact_sum(got32) == float(gold.z[f"shaded.{i}.sum"])                       # every pixel, not the lattice alone
    v64, _ = R.compose(noise, clean, np.float64)
    got64 = R.remove_dark_shading(v64, ratio, iso, dk, db, _blc(meta)[iso], np.float64)
    err = np.abs(got64[:, ::st, ::st] - want.astype(np.float64)).max()
    print(f"dark shading ratio {ratio} iso {iso}: float64 restatement vs reference fp32 max-abs {err:.3e}, bound {shading_bound(ratio):.3e}")
    assert err <= shading_bound(ratio)
    assert 0.05 < float((want > 0).mean()) and float((want < 1).mean()) > 0.05          # the stage is not clipped flat


@pytest.mark.parametrize("i", [0, 1, 2])
def test_restated_batch_equals_the_reference_from_the_recorded_counts(gold, i):
    meta, z = gold.meta, gold.z
    ratio, iso, (x0, y0) = meta["cases"][i]
    c, st = meta["crop"], meta["step"]
    noise, clean = _case_inputs(meta, i)
    _, planes = _maps(meta)
    (cx, cy), flip, wb = z[f"crop_xy.{i}"], int(z[f"flip.{i}"]), z["wb.used"][i]
    sna = bool(np.abs(wb).max() != 0)
    assert sna == (f"K.{i}" in z.files)
    K = float(z[f"K.{i}"]) if sna else None
    counts = _case_counts(meta, i) if sna else None
    if sna:
        assert np.array_equal(counts[:, ::st, ::st], z[f"counts.{i}"])
    kw = dict(planes=planes, blc_mean=_blc(meta), wb=wb, K=K, counts=counts)
    n32, c32 = R.build_sample(noise, clean, x0, y0, int(cx), int(cy), flip, iso, ratio, c, c, dtype=np.float32, **kw)
    assert n32.dtype == np.float32 and c32.dtype == np.float32
    assert np.array_equal(n32[:, ::st, ::st], z[f"noisy.{i}"]) and np.array_equal(c32[:, ::st, ::st], z[f"clean.{i}"])
    assert exact_sum(n32) == float(z[f"noisy.{i}.sum"]) and exact_sum(c32) == float(z[f"clean.{i}.sum"])          # every pixel, not the lattice alone
    n64, c64 = R.build_sample(noise, clean, x0, y0, int(cx), int(cy), flip, iso, ratio, c, c, dtype=np.float64, **kw)
    bn, bc = batch_bounds(ratio, True, sna, n64[:, ::st, ::st], c64[:, ::st, ::st])
    en, ec = np.abs(n64[:, ::st, ::st] - z[f"noisy.{i}"]), np.abs(c64[:, ::st, ::st] - z[f"clean.{i}"])
    print(f"sample {i}: noisy max err/bound {(en / bn).max():.3f}, clean max err {ec.max():.3e}")
    assert (en <= bn).all() and (ec <= bc).all()
    if sna:          # the reference's fp32 rate is the fp64 rate up to fp32 roundings
        lam = R.sample_rates(clean, int(cx), int(cy), flip, ratio, c, c, wb, K)[:, ::st, ::st]
        assert np.abs(lam - z[f"rate.{i}"]).max() <= 6 * E24 * max(1.0, float(lam.max()))        # four fp32 operations and fp32(K)


def test_white_balance_from_draws_equals_the_reference_with_both_gates(gold):
    from noisediff_amd import denoise_data as dd
    z = gold.z
    got = dd.sna_white_balance_from_draws(int(z["wb.open.r_idx"]), int(z["wb.open.gate"]), z["wb.open.n_g"], z["wb.open.n_r"], z["wb.open.n_b"])
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), z["wb.open"])
    assert float(np.abs(z["wb.open"]).max()) > 0
    shut = dd.sna_white_balance_from_draws(0, 0, z["wb.open.n_g"], z["wb.open.n_r"], z["wb.open.n_b"])
    assert np.array_equal(shut.numpy(), z["wb.closed"]) and float(shut.abs().max()) == 0.0
    state, tstate = np.random.get_state(), torch.get_rng_state()
    try:
        np.random.seed(5)
        torch.manual_seed(5)
        wb = dd.sna_white_balance(6)
        np.random.seed(5)
        torch.manual_seed(5)
        r_idx, gate = int(np.random.randint(2)), int(np.random.randint(4))
        n = [torch.randn(6) for _ in range(3)] if gate else [torch.zeros(6)] * 3
        assert torch.equal(wb, dd.sna_white_balance_from_draws(r_idx, gate, *n)) and wb.shape == (6, 4)
    finally:
        np.random.set_state(state)
        torch.set_rng_state(tstate)


def test_sna_gain_equals_the_reference(gold):
    from noisediff_amd import denoise_data as dd
    assert sum(g["in_table"] for g in gold.gains) == 28 and sum(not g["in_table"] for g in gold.gains) == 2
    assert sorted(g["iso"] for g in gold.gains if g["in_table"]) == sorted(dd.TABLE_ISOS)
    for g in gold.gains:
        assert dd.sna_gain(g["iso"], g["jitter"]) == pytest.approx(g["K"], rel=1e-12), g


# --------------------------------------------------------------------------- CPU 2: the numpy Poisson

def _assert_poisson_stats(x, lam, what):
    zm, zv, zc, dof = R.poisson_stats(x, lam)
    print(f"{what} lam={lam:g}: z(mean) {zm:+.2f} z(var) {zv:+.2f} z(chi2) {zc:+.2f} dof {dof}")
    assert np.isfinite(x).all() and (x >= 0).all() and (x == np.floor(x)).all()
    assert abs(zm) <= 5 and abs(zv) <= 5 and abs(zc) <= 5, (what, lam, zm, zv, zc)


@pytest.mark.parametrize("lam", RATES)
def test_numpy_poisson_statistics(lam):
    x, tries = R.poisson(np.full(N_STAT, lam), 1234, 3, 1, return_tries=True)
    _assert_poisson_stats(x, lam, "numpy")
    if lam >= 10:
        assert tries.max() <= 16 and 1.0 <= tries.mean() <= 1.4


def _assert_uncorrelated(x, y, what):
    n = x.size
    z1 = np.corrcoef(x[:-1], x[1:])[0, 1] * math.sqrt(n)
    z2 = np.corrcoef(x, y)[0, 1] * math.sqrt(n)
    print(f"{what}: lag-1 z {z1:+.2f}, cross-sample z {z2:+.2f}")
    assert abs(z1) <= 5 and abs(z2) <= 5


def test_numpy_poisson_neighbours_and_samples_are_uncorrelated():
    for lam in (3.7, 40.0):
        _assert_uncorrelated(R.poisson(np.full(N_STAT, lam), 99, 0, 1), R.poisson(np.full(N_STAT, lam), 99, 1, 1), f"numpy lam={lam}")


def test_numpy_poisson_edges():
    x = R.poisson(np.array([0.0, -1.0, np.nan, np.inf, 5.0, 50.0]), 7, 0, 0)
    assert x[0] == 0 and np.isnan(x[1:4]).all() and np.isfinite(x[4:]).all()
    a = R.poisson(np.full(4096, 25.0), 7, 2, 3)
    assert np.array_equal(a, R.poisson(np.full(4096, 25.0), 7, 2, 3))
    assert not np.array_equal(a, R.poisson(np.full(4096, 25.0), 8, 2, 3))
    assert not np.array_equal(a, R.poisson(np.full(4096, 25.0), 7, 2, 4))
    assert not np.array_equal(a, R.poisson(np.full(4096, 25.0), 7 + (1 << 32), 2, 3))       # the high word of the seed is part of the key


# --------------------------------------------------------------------------- CPU 3: arguments

def test_entry_points_check_arguments_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    f = C.c_void_p(4096)                            # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4100)

    def batch(noise=f, clean=f, maps=(None, None, None, None), mh=0, mw=0, table=f, sna=None, rng=None, draw=0, cin=None, cout=None, noisy=f,
              clean_out=f, B=2, P=128, h=64, w=64):
        return lib.nd_denoise_batch_f32(noise, clean, *maps, mh, mw, table, sna, rng, 1, 0, draw, cin, cout, noisy, clean_out, B, P, h, w, None)

    assert batch(noise=None) == -1 and batch(clean=None) == -1 and batch(table=None) == -1 and batch(noisy=None) == -1 and batch(clean_out=None) == -1
    assert batch(B=0) == -1 and batch(B=65536) == -1 and batch(P=0) == -1 and batch(h=0) == -1 and batch(draw=-1) == -1
    assert batch(maps=(f, f, f, None), mh=256, mw=256) == -1
    assert b"all four" in lib.nd_last_error()
    assert batch(h=130) == -2 and batch(w=130) == -2 and batch(w=62, h=63) == -2 and batch(P=127) == -2 and batch(w=63) == -2
    assert batch(maps=(f, f, f, f), mh=127, mw=256) == -2 and batch(maps=(f, f, f, f), mh=256, mw=64) == -2
    assert batch(noise=odd) == -3 and batch(clean=odd) == -3 and batch(noisy=odd) == -3 and batch(cin=odd) == -3 and batch(cout=odd) == -3
    assert batch(rng=odd) == -3 and batch(table=C.c_void_p(4098)) == -3
    p = lib.nd_philox_poisson_f32
    assert p(None, f, 0, 0, 0, 1, 16, None) == -1 and p(f, None, 0, 0, 0, 1, 16, None) == -1
    assert p(f, f, 0, 0, 0, 0, 16, None) == -1 and p(f, f, 0, 0, 0, 1, 0, None) == -1 and p(f, f, 0, 0, -1, 1, 16, None) == -1
    assert p(f, f, 0, 0, 0, 1, 1 << 32, None) == -2 and p(C.c_void_p(4098), f, 0, 0, 0, 1, 16, None) == -3
    k = lib.nd_pack_darkshading_f32
    assert k(None, f, 8, 8, None) == -1 and k(f, None, 8, 8, None) == -1 and k(f, f, 0, 8, None) == -1
    assert k(f, f, 7, 8, None) == -2 and k(f, f, 8, 9, None) == -2 and k(f, C.c_void_p(4098), 8, 8, None) == -3


def test_builder_refuses_bad_parameters_on_the_host():
    from noisediff_amd import _lib as L, denoise_data as dd
    for bad in ((0, 8), (8, 0), (10, 8), (7, 8), (6, 9)):
        with pytest.raises(ValueError):
            dd.BatchBuilder(crop=bad[0], patch=bad[1])
    b = dd.BatchBuilder(crop=64, patch=128)
    ok = dict(xy=[(0, 0), (5, 7)], iso=[800, 3200], ratio=[100, 250], crop_xy=[(64, 0), (2, 62)], flip=[1, 0], wb=[[0.1, 0.2, 0.3, 0.2], [0, 0, 0, 0]],
              K=[0.7, 3.0])
    host, sna = b.check(2, **ok)
    assert sna and host.dtype == np.int32
    assert b.check(2, **{**ok, "wb": None, "K": None})[1] is False
    for change in ({"crop_xy": [(63, 0), (2, 62)]}, {"crop_xy": [(66, 0), (2, 62)]}, {"crop_xy": [(64, -2), (2, 62)]}, {"crop_xy": [(64, 0)]},
                   {"K": [0.0, 3.0]}, {"K": [0.7, -1.0]}, {"K": None}, {"wb": [[0.1, -0.2, 0.3, 0.2], [0, 0, 0, 0]]}, {"ratio": [0, 250]},
                   {"draw": -1}, {"iso": [800]}):
        with pytest.raises(ValueError):
            b.check(2, **{**ok, **change})
    b.check(2, **{**ok, "K": [1e-5, 3.0]})                   # 15871 * 0.3 / (100 * 1e-5) = 4.8e6 < 2^24: counts stay exact
    with pytest.raises(ValueError, match="2\\*\\*24"):
        b.check(2, **{**ok, "K": [2e-6, 3.0]})               # 15871 * 0.3 / (100 * 2e-6) = 2.4e7 >= 2^24
    noise = torch.zeros(2, 4, 128, 128)
    with pytest.raises(L.HipError):
        b(noise, noise, **ok)
    with pytest.raises(ValueError):
        b(noise, torch.zeros(2, 4, 128, 64), **ok)
    with pytest.raises(ValueError):
        b(noise, noise, **{**ok, "K": [0.0, 3.0]})
    with pytest.raises(L.HipError):
        dd.philox_poisson(torch.ones(2, 8))
    with pytest.raises(L.HipError):
        dd.DarkShading(np.zeros((8, 8)), np.zeros((8, 8)), np.zeros((8, 8)), np.zeros((8, 8)), {800: 0.0}, "cpu")


def test_random_params_draws_as_the_reference_does():
    from noisediff_amd import denoise_data as dd
    b = dd.BatchBuilder(crop=64, patch=128)
    state, tstate = np.random.get_state(), torch.get_rng_state()
    try:
        for seed in range(6):
            np.random.seed(seed)
            torch.manual_seed(seed)
            p = b.random_params(3, [800, 1600, 300])
            np.random.seed(seed)
            torch.manual_seed(seed)
            crops = []
            for _ in range(3):
                x = np.random.randint(0, 65)
                y = np.random.randint(0, 65)
                crops.append((x // 2 * 2, y // 2 * 2))
            flip = np.random.randint(0, 2)
            wb = dd.sna_white_balance(3)
            K = [dd.sna_gain(iso, np.random.uniform(low=-0.01, high=0.01) if float(wb[i].abs().max()) != 0 else 0.0)
                 for i, iso in enumerate([800, 1600, 300])]
            assert p["crop_xy"] == crops and p["flip"] == [flip] * 3 and torch.equal(p["wb"], wb) and p["K"] == K
            b.check(3, [(0, 0)] * 3, [800, 1600, 300], [100, 250, 300], **p)
    finally:
        np.random.set_state(state)
        torch.set_rng_state(tstate)


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.gpu
def test_device_poisson_equals_the_restatement_element_for_element():
    from noisediff_amd import denoise_data as dd
    n = 1 << 22
    u = synth.uniform01(41, "dd.rates", n)
    rate = np.concatenate([(6640.0 * u ** 3).astype(np.float32), np.array(RATES, np.float32)])
    got = _np(dd.philox_poisson(torch.from_numpy(rate)[None].to(DEV), seed=(5 << 32) + 77, first_sample=9, draw=2))[0]
    want = R.poisson(rate.astype(np.float64), (5 << 32) + 77, 9, 2)
    differ = int((got != want).sum())
    print(f"device Poisson vs numpy restatement: {differ} of {rate.size} elements differ")
    assert np.isfinite(got).all() and differ <= 4
    edge = _np(dd.philox_poisson(torch.tensor([[0.0, -1.0, float("nan"), float("inf"), 5.0, 50.0]], device=DEV), seed=7))[0]
    assert edge[0] == 0 and np.isnan(edge[1:4]).all() and np.array_equal(edge[4:], R.poisson(np.array([0, -1, np.nan, np.inf, 5.0, 50.0]), 7, 0, 0)[4:])


@pytest.mark.gpu
def test_device_poisson_statistics():
    from noisediff_amd import denoise_data as dd
    rate = torch.tensor(RATES, dtype=torch.float32, device=DEV)[:, None].expand(len(RATES), N_STAT).contiguous()
    x = _np(dd.philox_poisson(rate, seed=1234, first_sample=3, draw=1)).astype(np.float64)
    for i, lam in enumerate(RATES):
        _assert_poisson_stats(x[i], float(np.float32(lam)), "device")
    other = _np(dd.philox_poisson(rate[7:8], seed=1234, first_sample=4, draw=1))[0].astype(np.float64)       # lam = 40 as another sample
    _assert_uncorrelated(x[7], other, "device lam=40")
    alone = _np(dd.philox_poisson(rate[5:6], seed=1234, first_sample=8, draw=1))[0]
    assert np.array_equal(alone, x[5])                   # sample 5 of a batch that starts at 3 is global sample 8


def _shading(meta):
    from noisediff_amd import denoise_data as dd
    bayer, planes = _maps(meta)
    sh = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], _blc(meta), DEV)
    return sh, planes


@pytest.mark.gpu
def test_packed_shading_planes_equal_the_restatement(gold):
    sh, planes = _shading(gold.meta)
    for k in ("k_high", "b_high", "k_low", "b_low"):
        assert np.array_equal(_np(getattr(sh, k)), planes[k]), k


@pytest.mark.gpu
def test_batch_equals_the_reference_goldens(gold):
    """The captured batch itself: 3 x 256^2 from 512^2 with the reference's crops, flips, gains and the recorded counts."""
    from noisediff_amd import denoise_data as dd
    meta, z = gold.meta, gold.z
    sh, planes = _shading(meta)
    c, st = meta["crop"], meta["step"]
    ins = [_case_inputs(meta, i) for i in range(3)]
    noise, clean = (torch.from_numpy(np.stack([p[j] for p in ins])).to(DEV) for j in (0, 1))
    wb = z["wb.used"]
    K = [float(z[f"K.{i}"]) if f"K.{i}" in z.files else 1.0 for i in range(3)]
    counts = np.stack([_case_counts(meta, i) for i in range(3)])
    cases = meta["cases"]
    build = dd.BatchBuilder(crop=c, patch=meta["patch"], shading=sh)
    noisy, clean_out, used = build(noise, clean, xy=[cs[2] for cs in cases], iso=[cs[1] for cs in cases], ratio=[cs[0] for cs in cases],
                                   crop_xy=[z[f"crop_xy.{i}"] for i in range(3)], flip=[int(z[f"flip.{i}"]) for i in range(3)], wb=wb, K=K,
                                   counts=torch.from_numpy(counts).to(DEV), return_counts=True)
    noisy, clean_out, used = _np(noisy), _np(clean_out), _np(used)
    for i, (ratio, iso, (x0, y0)) in enumerate(cases):
        sna = bool(np.abs(wb[i]).max() != 0)
        assert np.array_equal(used[i], counts[i] if sna else np.zeros_like(counts[i]))
        gn, gc = z[f"noisy.{i}"].astype(np.float64), z[f"clean.{i}"].astype(np.float64)
        bn, bc = batch_bounds(ratio, True, sna, gn, gc)
        en, ec = np.abs(noisy[i][:, ::st, ::st] - gn), np.abs(clean_out[i][:, ::st, ::st] - gc)
        print(f"sample {i} vs reference: noisy max err/bound {(en / bn).max():.3f} (bitwise equal: {(en == 0).mean():.4f}), clean max err {ec.max():.3e}")
        assert (en <= bn).all() and (ec <= bc).all()
        cx, cy = (int(v) for v in z[f"crop_xy.{i}"])
        n64, c64 = R.build_sample(*ins[i], x0, y0, cx, cy, int(z[f"flip.{i}"]), iso, ratio, c, c, planes=planes, blc_mean=_blc(meta), wb=wb[i], K=K[i],
                                  counts=counts[i], dtype=np.float64)
        bn, bc = batch_bounds(ratio, True, sna, n64, c64)
        assert (np.abs(noisy[i] - n64) <= bn).all() and (np.abs(clean_out[i] - c64) <= bc).all()
        assert float(noisy[i].sum(dtype=np.float64)) == pytest.approx(float(z[f"noisy.{i}.sum"]), rel=1e-6)


def _small_frame(seed, Hm, Wm):
    rng = {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}
    return {k: synth.uniform(seed, f"dd.small.{k}", (2 * Hm, 2 * Wm), lo, hi).numpy() for k, (lo, hi) in rng.items()}


BLC = {100: 0.5, 800: 0.25, 1600: -0.5, 3200: 1.0, 25600: 1.75}
SHAPES = {"4x256_from_512": (4, 512, 256, 600, 640), "2x64_from_128": (2, 128, 64, 150, 170)}


def _params(B, P, c, Hm, Wm, sna):
    """Odd-looking even offsets (cx = P - w with cy = 0, and the reverse), odd patch origins, flips on and off, one all-zero row of gains."""
    xy = [(0, 0), (Wm - P, Hm - P), (13, 7), (Wm - P - 1, 3)][:B]
    crop_xy = [(P - c, 0), (0, P - c), (2, P - c - 2), ((P - c) // 2 // 2 * 2, 6)][:B]
    iso, ratio = [800, 3200, 1600, 25600][:B], [100, 250, 300, 100][:B]
    flip = [1, 0, 1, 0][:B]
    wb = K = None
    if sna:
        wb = np.array([[0.31, 0.12, 0.55, 0.12], [0, 0, 0, 0], [1.0, 0.4, 0.0, 0.4], [0.02, 0.9, 0.7, 0.9]], np.float32)[:B]
        K = [0.76, 3.06, 1.53, 24.4][:B]
    return dict(xy=xy, iso=iso, ratio=ratio, crop_xy=crop_xy, flip=flip, wb=wb, K=K)


def _images(seed, B, P):
    noise = 0.2 * synth.normal(seed, f"dd.t.noise.{P}", (B, 4, P, P))
    noise[:, :, ::17, ::13] *= 8.0                                            # some of it beyond the [-1, 1] clip
    clean = synth.uniform(seed, f"dd.t.clean.{P}", (B, 4, P, P), -0.05, 1.1)
    return noise.contiguous(), clean.contiguous()


def _reference_batch(noise, clean, prm, c, planes, counts, dtype=np.float64):
    outs = []
    for b in range(noise.shape[0]):
        (x0, y0), (cx, cy) = prm["xy"][b], prm["crop_xy"][b]
        outs.append(R.build_sample(noise[b], clean[b], x0, y0, cx, cy, prm["flip"][b], prm["iso"][b], prm["ratio"][b], c, c, planes=planes, blc_mean=BLC,
                                   wb=None if prm["wb"] is None else prm["wb"][b], K=None if prm["K"] is None else prm["K"][b],
                                   counts=None if counts is None else counts[b], dtype=dtype))
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("shading", [True, False])
@pytest.mark.parametrize("sna", [True, False])
def test_batch_with_explicit_counts_equals_the_float64_restatement(shape, shading, sna):
    from noisediff_amd import denoise_data as dd
    B, P, c, Hm, Wm = SHAPES[shape]
    bayer = _small_frame(3, Hm, Wm)
    planes = {k: R.pack_planes(v) for k, v in bayer.items()} if shading else None
    sh = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], BLC, DEV) if shading else None
    noise, clean = _images(5, B, P)
    prm = _params(B, P, c, Hm, Wm, sna)
    counts = np.floor(synth.uniform(5, f"dd.t.counts.{c}", (B, 4, c, c), 0.0, 200.0).numpy()) if sna else None
    build = dd.BatchBuilder(crop=c, patch=P, shading=sh)
    inputs = build.update(build.capture_inputs(B, DEV), **prm)
    noisy = torch.full((B, 4, c, c), float("nan"), device=DEV)
    clean_out = torch.full((B, 4, c, c), float("nan"), device=DEV)
    used = torch.full((B, 4, c, c), float("nan"), device=DEV)
    r = build.launch(inputs, noise.to(DEV), clean.to(DEV), noisy, clean_out, counts=None if counts is None else torch.from_numpy(counts).to(DEV),
                     counts_out=used)
    assert r[0] is noisy and r[1] is clean_out
    noisy, clean_out, used = _np(noisy), _np(clean_out), _np(used)
    assert np.isfinite(noisy).all() and np.isfinite(clean_out).all() and np.isfinite(used).all()          # every element written
    n64, c64 = _reference_batch(noise.numpy(), clean.numpy(), prm, c, planes, counts)
    for b in range(B):
        on = sna and bool(np.abs(prm["wb"][b]).max() != 0)
        assert np.array_equal(used[b], counts[b] if on else np.zeros((4, c, c), np.float32))
        bn, bc = batch_bounds(prm["ratio"][b], shading, on, n64[b], c64[b])
        en, ec = np.abs(noisy[b] - n64[b]), np.abs(clean_out[b] - c64[b])
        print(f"{shape} shading={shading} sna={on} sample {b}: noisy max err/bound {(en / bn).max():.3f}, clean max err {ec.max():.3e}")
        assert (en <= bn).all() and (ec <= bc).all()
    n32, c32 = _reference_batch(noise.numpy(), clean.numpy(), prm, c, planes, counts, dtype=np.float32)
    # one IEEE operation per step and no contraction: numpy float32 repeats the kernel bit for bit
    assert np.array_equal(n32, noisy) and np.array_equal(c32, clean_out)
    # the same call through the builder's front door
    a, b_ = build(noise.to(DEV), clean.to(DEV), **prm, counts=None if counts is None else torch.from_numpy(counts).to(DEV))
    assert np.array_equal(_np(a), noisy) and np.array_equal(_np(b_), clean_out)
    if shading:
        with pytest.raises(ValueError):
            build.check(B, **{**prm, "xy": [(Wm - P + 1, 0)] + prm["xy"][1:]})
    nan_in = clean.clone()
    nan_in[0, 1, prm["crop_xy"][0][1] + 3, prm["crop_xy"][0][0] + 5] = float("nan")                    # NaN passes the clips
    a, b_ = build(noise.to(DEV), nan_in.to(DEV), **{**prm, "wb": None, "K": None})
    assert int(torch.isnan(a).sum()) == 1 and int(torch.isnan(b_).sum()) == 1


@pytest.mark.gpu
def test_drawn_counts_equal_the_restatement_and_replay():
    from noisediff_amd import denoise_data as dd
    B, P, c, Hm, Wm = SHAPES["2x64_from_128"]
    B = 4
    bayer = _small_frame(3, Hm, Wm)
    sh = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], BLC, DEV)
    noise, clean = _images(6, B, P)
    clean[0] *= 40.0 / 15871 * 100                       # sample 0: rates below and around 10, the inversion branch and the switch
    prm = _params(B, P, c, Hm, Wm, True)
    build = dd.BatchBuilder(crop=c, patch=P, shading=sh)
    nd, cd = noise.to(DEV), clean.to(DEV)
    key = dict(seed=(3 << 32) + 11, first_sample=5, draw=4)
    noisy, clean_out, used = build(nd, cd, **prm, **key, return_counts=True)
    differ, total, small = 0, 0, 0
    for b in range(B):
        lam = R.sample_rates(clean[b].numpy(), *prm["crop_xy"][b], prm["flip"][b], prm["ratio"][b], c, c, prm["wb"][b], prm["K"][b])
        if lam is None:
            assert float(used[b].abs().max()) == 0
            continue
        want = R.poisson(lam.reshape(-1), key["seed"], key["first_sample"] + b, key["draw"]).reshape(4, c, c)
        differ += int((_np(used[b]) != want).sum())
        total += want.size
        small += int(((lam > 0) & (lam < 10)).sum())
    print(f"drawn counts vs restatement: {differ} of {total} differ ({small} rates in (0, 10))")
    assert differ <= 4 and small > 1000
    again = build(nd, cd, **prm, **key, return_counts=True)
    assert all(torch.equal(x, y) for x, y in zip((noisy, clean_out, used), again))
    fed = build(nd, cd, **prm, counts=used)
    assert torch.equal(fed[0], noisy) and torch.equal(fed[1], clean_out)
    one = {k: (v[2:3] if v is not None else None) for k, v in prm.items()}
    alone = build(nd[2:3], cd[2:3], **one, seed=key["seed"], first_sample=key["first_sample"] + 2, draw=key["draw"], return_counts=True)
    assert torch.equal(alone[0][0], noisy[2]) and torch.equal(alone[1][0], clean_out[2]) and torch.equal(alone[2][0], used[2])
    for other in (dict(key, draw=5), dict(key, seed=key["seed"] + 1), dict(key, seed=key["seed"] + (1 << 32)), dict(key, first_sample=6)):
        assert not torch.equal(build(nd, cd, **prm, **other, return_counts=True)[2], used), other


@pytest.mark.gpu
def test_a_captured_build_replays_with_rewritten_parameters():
    """One launch in the graph (a single chain); the device table and the rng triple are rewritten between replays."""
    from noisediff_amd import denoise_data as dd
    B, P, c, Hm, Wm = SHAPES["2x64_from_128"]
    bayer = _small_frame(3, Hm, Wm)
    sh = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], BLC, DEV)
    noise, clean = (t.to(DEV) for t in _images(7, B, P))
    build = dd.BatchBuilder(crop=c, patch=P, shading=sh)
    p1 = _params(B, P, c, Hm, Wm, True)
    p2 = dict(p1, crop_xy=[(10, 20), (P - c, P - c)], flip=[0, 1], wb=np.array([[0, 0, 0, 0], [0.5, 0.25, 0.125, 0.25]], np.float32), K=[0.8, 2.9],
              xy=[(3, 5), (0, 1)], iso=[25600, 100], ratio=[300, 100])
    k1, k2 = dict(seed=1, first_sample=0, draw=0), dict(seed=(9 << 32) + 2, first_sample=40, draw=7)
    inputs = build.capture_inputs(B, DEV)
    build.update(inputs, **p1, **k1)
    noisy, clean_out, used = (torch.empty(B, 4, c, c, device=DEV) for _ in range(3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        build.launch(inputs, noise, clean, noisy, clean_out, counts_out=used)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        build.launch(inputs, noise, clean, noisy, clean_out, counts_out=used)
    for prm, key in ((p1, k1), (p2, k2), (p1, k2)):
        build.update(inputs, **prm, **key)
        noisy.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        want = build(noise, clean, **prm, **key, return_counts=True)
        assert torch.equal(noisy, want[0]) and torch.equal(clean_out, want[1]) and torch.equal(used, want[2])
    assert float(used[0].abs().max()) > 0                 # the last replay augmented sample 0 again


@pytest.mark.gpu
def test_a_training_step_runs_on_a_built_batch():
    import torch.nn.functional as F
    from noisediff_amd import TrainableLSID, denoise_data as dd, train
    from noisediff_amd.spec import lsid_param_spec
    B, P, c, Hm, Wm = SHAPES["2x64_from_128"]
    bayer = _small_frame(3, Hm, Wm)
    sh = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], BLC, DEV)
    noise, clean = (t.to(DEV) for t in _images(8, B, P))
    build = dd.BatchBuilder(crop=c, patch=P, shading=sh)
    state, tstate = np.random.get_state(), torch.get_rng_state()
    try:
        np.random.seed(3)
        torch.manual_seed(3)
        prm = build.random_params(B, [800, 3200])
    finally:
        np.random.set_state(state)
        torch.set_rng_state(tstate)
    noisy, target = build(noise, clean, xy=[(0, 0), (13, 7)], iso=[800, 3200], ratio=[100, 250], **prm, seed=1)
    assert noisy.shape == (B, 4, c, c) and torch.isfinite(noisy).all() and torch.isfinite(target).all()
    net = TrainableLSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    net = net.to(DEV).hip()
    opt = train.Adam(net.parameters(), lr=1e-4)
    w0 = net.conv5_2.weight.detach().clone()
    opt.zero_grad(set_to_none=True)
    loss = F.l1_loss(net(noisy), target)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    assert not torch.equal(w0, net.conv5_2.weight.detach())
