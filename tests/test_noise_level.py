"""noisediff_amd.noise_level: the exact per-level moments, the curve and the all-pairs Theil-Sen fit, on the HIP library.

CPU: the module, the translation unit and every entry point exist (without the feature every test of this file fails at import or at symbol
lookup); the restatement (tests/noise_level_ref.py) equals the reference's results (tests/golden/noise_level.npz) within four times the gap
that the capture script measured between the reference's fp32 torch.std and the fp64 std; it equals sklearn's TheilSenRegressor, stored and
(where sklearn is installed) live; the C entry points refuse each bad argument before any HIP call.
GPU: the table against the Python-integer table (exact), the statistics against float64 numpy on the exact inputs within the derived bound,
the curve against the restatement, the fit against the restatement with equal step counts, the reference's numbers end to end, the packer's
grid, bitwise repeats and a captured graph."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import noise_level_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
ENTRIES = ["nd_level_table_bytes", "nd_level_moments_reset", "nd_level_moments_f32", "nd_level_stats_f64", "nd_level_curve_f64",
           "nd_theil_sen_workspace_bytes", "nd_theil_sen_f64"]
NAMES = ["LevelMoments", "level_curve", "theil_sen", "get_poisson_lambda", "get_poisson_lambda_all_images", "get_regression_result_all_images"]
# gelss solves a pair with cond([[1, x_i], [1, x_j]]) eps <= 2 * 15871 * 2.2e-16 = 7e-12 relative where the restatement uses the closed form,
# and the spatial median moves by no more than its points do
SKLEARN_RTOL, SKLEARN_ATOL = 1e-10, 1e-13


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(REPO, "tests", "golden", "noise_level.npz"))
    return {k: z[k] for k in z.files}


# --------------------------------------------------------------------------- CPU

def test_the_module_and_its_entry_points_exist():
    """Fails without the feature: the module, the translation unit and the declared, exported and bound entry points."""
    from noisediff_amd import _lib as L, build, noise_level
    import noisediff_amd
    assert "noise_level" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "noise_level.hip"))
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    for name in NAMES:
        assert getattr(noisediff_amd, name) is getattr(noise_level, name) and name in noisediff_amd.__all__, name
    assert lib.nd_level_table_bytes(15872) == 15872 * 32 and lib.nd_theil_sen_workspace_bytes(15872, 0) > 0


def test_restatement_equals_the_reference_goldens(gold):
    for key, below in (("a", True), ("b", False)):
        lam, sig, steps, fitted = R.get_poisson_lambda(gold[f"{key}.clean"], gold[f"{key}.noisy"], below_median=below)
        assert fitted <= 141                                                    # above that the reference is not repeatable
        assert [lam, sig, steps, fitted] == gold[f"{key}.restated"].tolist()
        gap = gold[f"{key}.gap"]
        print(key, "lambda", lam, gold[f"{key}.lambda"], "sigma", sig, gold[f"{key}.sigma"], "gap", gap)
        assert abs(lam - gold[f"{key}.lambda"]) <= 4 * gap[0] and abs(sig - gold[f"{key}.sigma"]) <= 4 * gap[1]
        assert 0 < gap[0] < 1e-7 and 0 < gap[1] < 1e-8                          # fp32 rounding of the reference's std, nothing larger
    assert np.unique(gold["a.clean"]).size == 163 and gold["a.restated"][3] == 81
    ca, na = R.level_frame(int(gold["meta.seed"]), (4, 24, 40), 160)
    assert np.array_equal(ca, gold["a.clean"]) and np.array_equal(na, gold["a.noisy"])


def test_restatement_equals_the_stored_fits_and_sklearns(gold):
    for name in R.FIT_CASES:
        x, y, pairs, max_iter, tol = R.fit_case(name)
        assert np.array(R.theil_sen(x, y, pairs, max_iter, tol), np.float64).tobytes() == gold[f"fit.{name}"].tobytes(), name
    assert gold["fit.m100.exhausted"][2] == 3 and gold["fit.m141.tight"][2] > 3
    for name, (m, seed, pairs) in R.SKLEARN_CASES.items():
        x, y = R.synthetic_curve(m, seed)
        slope, icpt, steps = R.theil_sen(x, y, R.sklearn_pairs(m) if pairs == "sk" else None)
        want = gold[f"sklearn.{name}"]
        print(name, slope - want[0], icpt - want[1])
        np.testing.assert_allclose([slope, icpt], want[:2], rtol=SKLEARN_RTOL, atol=SKLEARN_ATOL)
        assert steps == want[2]
    assert R.theil_sen(np.zeros(0), np.zeros(0)) == (0.0, 0.0, 0) and np.isnan(R.theil_sen(np.ones(1), np.ones(1))[0])


@pytest.mark.parametrize("name", list(R.SKLEARN_CASES))
def test_restatement_equals_sklearn(name):
    lm = pytest.importorskip("sklearn.linear_model")
    m, seed, pairs = R.SKLEARN_CASES[name]
    x, y = R.synthetic_curve(m, seed)
    assert (pairs is None) == (m * (m - 1) // 2 <= 10000)                       # sklearn fits all pairs up to max_subpopulation
    reg = lm.TheilSenRegressor(random_state=0).fit(x.reshape(-1, 1), y)
    slope, icpt, steps = R.theil_sen(x, y, R.sklearn_pairs(m) if pairs == "sk" else None)
    print(name, slope - reg.coef_[0], icpt - reg.intercept_)
    np.testing.assert_allclose([slope, icpt], [reg.coef_[0], reg.intercept_], rtol=SKLEARN_RTOL, atol=SKLEARN_ATOL)
    assert steps == reg.n_iter_ + 1


def test_entry_points_refuse_each_bad_argument_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    fake, odd8, odd4 = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4098)     # never dereferenced: every call below fails its checks first
    tb = lib.nd_level_table_bytes
    assert tb(1) == 32 and tb(8) == 256 and tb(1 << 24) == 32 << 24 and tb(0) == -1 and tb(-4) == -1 and tb((1 << 24) + 1) == -1
    rs = lambda t, nl, c: lib.nd_level_moments_reset(t, nl, c, None)  # noqa: E731
    assert rs(None, 8, fake) == -1 and b"null" in lib.nd_last_error() and rs(fake, 8, None) == -1
    assert rs(fake, 0, fake) == -1 and rs(fake, (1 << 24) + 1, fake) == -1 and rs(odd8, 8, fake) == -1 and rs(fake, 8, odd8) == -1
    mo = lambda c, v, n, s, nl, t, k: lib.nd_level_moments_f32(c, v, n, s, nl, t, k, None)  # noqa: E731
    for bad in range(4):
        a = [fake, fake, fake, fake]
        a[bad] = None
        assert mo(a[0], a[1], 8, 15871.0, 15872, a[2], a[3]) == -1 and b"null" in lib.nd_last_error(), bad
    assert mo(fake, fake, 0, 15871.0, 15872, fake, fake) == -1 and mo(fake, fake, -1, 15871.0, 15872, fake, fake) == -1
    assert mo(fake, fake, 1 << 31, 15871.0, 15872, fake, fake) == -1 and b"2^31" in lib.nd_last_error()
    assert mo(fake, fake, 8, 0.0, 15872, fake, fake) == -1 and mo(fake, fake, 8, -1.0, 15872, fake, fake) == -1
    assert mo(fake, fake, 8, float("nan"), 15872, fake, fake) == -1 and mo(fake, fake, 8, float("inf"), 15872, fake, fake) == -1
    assert mo(fake, fake, 8, 15871.0, 0, fake, fake) == -1 and mo(fake, fake, 8, 15871.0, (1 << 24) + 1, fake, fake) == -1
    assert mo(odd4, fake, 8, 15871.0, 15872, fake, fake) == -1 and b"aligned" in lib.nd_last_error()
    assert mo(fake, odd4, 8, 15871.0, 15872, fake, fake) == -1 and mo(fake, fake, 8, 15871.0, 15872, odd8, fake) == -1
    assert mo(fake, fake, 8, 15871.0, 15872, fake, odd8) == -1
    st = lambda t, nl, c, m, s: lib.nd_level_stats_f64(t, nl, c, m, s, None)  # noqa: E731
    for bad in range(4):
        a = [fake, fake, fake, fake]
        a[bad] = None
        assert st(a[0], 8, a[1], a[2], a[3]) == -1, bad
        a[bad] = odd8
        assert st(a[0], 8, a[1], a[2], a[3]) == -1 and b"aligned" in lib.nd_last_error(), bad
    assert st(fake, 0, fake, fake, fake) == -1 and st(fake, (1 << 24) + 1, fake, fake, fake) == -1
    cu = lambda c, s, nl, sc, bm, x, y, m: lib.nd_level_curve_f64(c, s, nl, sc, bm, x, y, m, None)  # noqa: E731
    for bad in range(5):
        a = [fake] * 5
        a[bad] = None
        assert cu(a[0], a[1], 8, 7.0, 1, a[2], a[3], a[4]) == -1, bad
        a[bad] = odd4
        assert cu(a[0], a[1], 8, 7.0, 1, a[2], a[3], a[4]) == -1 and b"aligned" in lib.nd_last_error(), bad
    assert cu(fake, fake, 0, 7.0, 1, fake, fake, fake) == -1 and cu(fake, fake, 8, 0.0, 1, fake, fake, fake) == -1
    assert cu(fake, fake, 8, 7.0, 2, fake, fake, fake) == -1 and cu(fake, fake, 8, 7.0, -1, fake, fake, fake) == -1
    wb = lib.nd_theil_sen_workspace_bytes
    assert wb(1, 0) > 0 and wb(1, 0) % 8 == 0 and wb(0, 0) == -1 and wb((1 << 24) + 1, 0) == -1 and wb(8, -1) == -1
    ts = lambda x, y, m, mm, p, n, it, tol, o, w: lib.nd_theil_sen_f64(x, y, m, mm, p, n, it, tol, o, w, None)  # noqa: E731
    for bad in range(5):
        a = [fake] * 5
        a[bad] = None
        assert ts(a[0], a[1], a[2], 8, None, 0, 300, 1e-3, a[3], a[4]) == -1 and b"null" in lib.nd_last_error(), bad
        a[bad] = odd4 if bad == 2 else odd8
        if bad == 2:
            a[bad] = C.c_void_p(4097)
        assert ts(a[0], a[1], a[2], 8, None, 0, 300, 1e-3, a[3], a[4]) == -1 and b"aligned" in lib.nd_last_error(), bad
    ok = lambda **kw: ts(fake, fake, fake, kw.get("mm", 8), kw.get("p"), kw.get("n", 0), kw.get("it", 300), kw.get("tol", 1e-3), fake, fake)  # noqa: E731
    assert ok(mm=0) == -1 and ok(mm=(1 << 24) + 1) == -1
    assert ok(p=fake, n=0) == -1 and b"n_pairs" in lib.nd_last_error() and ok(p=None, n=5) == -1 and ok(p=fake, n=-2) == -1
    assert ok(p=C.c_void_p(4098), n=4) == -1
    assert ok(it=0) == -1 and ok(it=(1 << 16) + 1) == -1 and b"max_iter" in lib.nd_last_error()
    assert ok(tol=-1e-3) == -1 and ok(tol=float("nan")) == -1 and ok(tol=float("inf")) == -1


def test_python_layer_refuses_cpu_tensors():
    from noisediff_amd import _lib as L, noise_level as nl
    x = torch.zeros(8)
    with pytest.raises(L.HipError):
        nl.get_poisson_lambda(x, x)
    with pytest.raises(L.HipError):
        nl.theil_sen(x.double(), x.double())
    with pytest.raises(L.HipError):
        nl.LevelMoments(device="cpu")


# --------------------------------------------------------------------------- GPU

def _mixed(n, n_levels, scale, seed, specials=True):
    """n elements on the grid of n_levels, noisy about 0.5 (q^2 passes 2^64: the low word carries on about every second add), levels 0 and
    n_levels - 1 among them; with ``specials`` (n >= 16) off-grid and out-of-range clean values and NaN, inf and too large noisy values."""
    rs = np.random.RandomState(seed)
    lv = rs.randint(0, n_levels, n)
    lv[0] = n_levels - 1
    if n > 1:
        lv[1] = 0
    clean = lv.astype(np.float32) / np.float32(scale)
    noisy = (0.5 + 0.3 * rs.standard_normal(n)).astype(np.float32)
    if specials and n >= 16:
        clean[2] += np.float32(0.3 / scale)                                      # between two levels
        clean[3], clean[4], clean[5], clean[6] = 1.0 + 2.0 / scale, -1.0 / scale, np.nan, np.inf
        noisy[7], noisy[8], noisy[9], noisy[10], noisy[11] = np.nan, np.inf, -np.inf, 4.0, -5.5
        noisy[12], noisy[13] = np.float32(3.9999998), -0.75
        clean[14], noisy[14] = np.nan, np.nan                                    # off grid is asked first
    return clean, noisy


def _moments(clean, noisy, n_levels=R.N_LEVELS, scale=R.SCALE, mom=None, misalign=False):
    from noisediff_amd import noise_level as nl
    mom = nl.LevelMoments(n_levels, scale, DEV) if mom is None else mom

    def up(a):
        a = np.asarray(a, np.float32).ravel()
        if not misalign:
            return torch.from_numpy(a).to(DEV)
        buf = torch.zeros(a.size + 1, device=DEV)
        buf[1:].copy_(torch.from_numpy(a))
        assert buf[1:].data_ptr() % 16 == 4
        return buf[1:]
    mom.add(up(clean), up(noisy))
    return mom


def _words(mom):
    torch.cuda.synchronize()
    return mom.table.cpu().numpy().view(np.uint64), mom.counters().cpu().numpy().tolist()


def _check_table(clean, noisy, n_levels=R.N_LEVELS, scale=R.SCALE, **kw):
    t, counters = R.table(clean, noisy, n_levels, scale)
    got, got_counters = _words(_moments(clean, noisy, n_levels, scale, **kw))
    assert got_counters == counters
    assert np.array_equal(got, R.words(t, n_levels))
    return t, counters


@pytest.mark.gpu
@pytest.mark.parametrize("n_levels", [8, 15872])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_table_is_exact_around_one_wave(n, n_levels):
    clean, noisy = _mixed(n, n_levels, n_levels - 1.0, 100 + n)
    t, counters = _check_table(clean, noisy, n_levels, n_levels - 1.0)
    assert 0 in t or n == 1
    assert (n_levels - 1) in t and (counters == [6, 5] if n >= 16 else counters == [0, 0])


@pytest.mark.gpu
def test_table_is_exact_on_the_golden_input_and_carries(gold):
    t, counters = _check_table(gold["a.clean"], gold["a.noisy"])
    assert counters == [0, 0] and len(t) == 163 and sum(e[0] for e in t.values()) == 3840
    clean, noisy = _mixed(3840, 15872, 15871.0, 5)
    t, _ = _check_table(clean, noisy)
    assert any(e[2] >> 64 for e in t.values())                                  # the high word is in use


@pytest.mark.gpu
def test_table_is_exact_off_alignment_with_a_scalar_tail():
    n = 4 * 33 * 257
    assert n % 1024 != 0
    clean, noisy = _mixed(n, 15872, 15871.0, 6)
    _check_table(clean, noisy, misalign=True)
    _check_table(clean, noisy, 8, 7.0, misalign=True)                           # nearly everything off the grid of eight levels


@pytest.mark.gpu
def test_table_is_exact_when_waves_sit_on_one_level():
    """70 000 elements on one level: 68 full trips on the wave-uniform path over 18 workgroups, and a tail.  Then two levels, with one element
    that is left out in the middle of a wave, so that this wave alone takes the general path."""
    rs = np.random.RandomState(7)
    n = 70000
    noisy = (0.5 + 0.3 * rs.standard_normal(n)).astype(np.float32)
    clean = np.full(n, np.float32(100) / np.float32(15871.0), np.float32)
    t, counters = _check_table(clean, noisy)
    assert list(t) == [100] and t[100][0] == n and counters == [0, 0]
    _check_table(clean, noisy, misalign=True)                                    # the same path behind the lane-strided scalar loads
    clean[35000:] = np.float32(15871) / np.float32(15871.0)
    noisy[20001] = np.nan
    clean[50003] = 0.5 / 15871.0
    t, counters = _check_table(clean, noisy)
    assert sorted(t) == [100, 15871] and counters == [1, 1]
    _check_table(np.zeros(n, np.float32), np.zeros(n, np.float32))               # a dark frame: level 0, q = 2^32 exactly


@pytest.mark.gpu
def test_table_does_not_depend_on_order_split_or_repeat():
    clean, noisy = _mixed(4 * 33 * 257, 15872, 15871.0, 8)
    whole, counters = _words(_moments(clean, noisy))
    again, _ = _words(_moments(clean, noisy))
    assert np.array_equal(whole, again)
    p = np.random.RandomState(9).permutation(clean.size)
    permuted, pc = _words(_moments(clean[p], noisy[p]))
    assert np.array_equal(whole, permuted) and pc == counters
    k = 12345
    mom = _moments(clean[:k], noisy[:k])
    split, sc = _words(_moments(clean[k:], noisy[k:], mom=mom))
    assert np.array_equal(whole, split) and sc == counters and mom.added == clean.size
    ta, tb = R.table(clean[:k], noisy[:k])[0], R.table(clean[k:], noisy[k:])[0]
    assert np.array_equal(R.words(R.merge(ta, tb)), whole)
    mom.reset()
    assert mom.added == 0 and not _words(mom)[0].any() and _words(mom)[1] == [0, 0]


@pytest.mark.gpu
def test_the_element_limit_is_checked_on_the_host_before_the_launch():
    from noisediff_amd import noise_level as nl
    mom = nl.LevelMoments(8, 7.0, DEV)
    mom.added = (1 << 31) - 1 - 5
    x = torch.zeros(6, device=DEV)
    with pytest.raises(ValueError, match="2147483647"):
        mom.add(x, x)
    assert mom.added == (1 << 31) - 6 and not _words(mom)[0].any()
    mom.add(x[:5], x[:5])
    assert mom.added == (1 << 31) - 1 and _words(mom)[0][0, 0] == 5


@pytest.mark.gpu
def test_stats_against_float64_numpy_on_the_exact_inputs(gold):
    """|d mean| <= 2^-31 = 4.7e-10 and |d std| <= sqrt(2) 2^-31 = 6.6e-10: rounding to the quantum 2^-30 moves every value by h = 2^-31 at
    most, so the mean by h at most; the unbiased std is |centred values| / sqrt(n - 1), a norm, so it moves by |d| / sqrt(n - 1) <=
    h sqrt(n / (n - 1)) <= h sqrt(2) for n >= 2.  The float64 evaluation on either side adds some 1e-16.  Asserted: 1e-9."""
    for clean, noisy, n_levels, scale in ((gold["a.clean"], gold["a.noisy"], 15872, 15871.0), (*_mixed(20000, 15872, 15871.0, 10), 15872, 15871.0),
                                          (*_mixed(5000, 8, 7.0, 11), 8, 7.0)):
        mom = _moments(clean, noisy, n_levels, scale)
        count, mean, std = [a.cpu().numpy() for a in mom.stats()]
        c64, m64, s64 = R.stats_float64(clean, noisy, n_levels, scale)
        assert np.array_equal(count, c64)
        assert np.array_equal(np.isnan(mean), c64 == 0) and np.array_equal(np.isnan(std), c64 < 2)
        dm, ds = np.nanmax(np.abs(mean - m64)), np.nanmax(np.abs(std - s64))
        print("stats: max |d mean|", dm, "max |d std|", ds)
        assert dm <= 1e-9 and ds <= 1e-9
        rc, rm, rstd = R.stats(R.table(clean, noisy, n_levels, scale)[0], n_levels)
        np.testing.assert_allclose(mean, rm, rtol=1e-15, atol=0, equal_nan=True)
        np.testing.assert_allclose(std, rstd, rtol=1e-15, atol=0, equal_nan=True)
        if clean is gold["a.clean"]:
            assert (c64 == 1).sum() == 1 and np.isnan(std[c64 == 1]).all() and not np.isnan(mean[c64 == 1]).any()      # NaN at n = 1, as torch.std


@pytest.mark.gpu
@pytest.mark.parametrize("below_median", [True, False])
def test_curve_is_the_restatements(gold, below_median):
    from noisediff_amd import noise_level as nl
    for clean, noisy, n_levels, scale in ((gold["a.clean"], gold["a.noisy"], 15872, 15871.0), (*_mixed(300, 8, 7.0, 12), 8, 7.0),
                                          (*_mixed(6000, 2500, 2499.0, 13), 2500, 2499.0)):      # 2500 levels: three trips of the one workgroup
        mom = _moments(clean, noisy, n_levels, scale)
        x, y, m = nl.level_curve(mom, below_median)
        count, _, std = R.stats(R.table(clean, noisy, n_levels, scale)[0], n_levels)
        levels, rx, ry = R.curve(count, std, scale, below_median)
        assert m.dtype == torch.int32 and int(m) == levels.size and x.shape == y.shape == (n_levels,)
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(x[:levels.size], rx) and np.isnan(x[levels.size:]).all() and np.isnan(y[levels.size:]).all()
        np.testing.assert_allclose(y[:levels.size], ry, rtol=1e-15, atol=0)
    assert levels.size > 512
    empty = nl.LevelMoments(8, 7.0, DEV)
    assert int(nl.level_curve(empty, below_median)[2]) == 0


def _fit_gpu(x, y, pairs=None, max_iter=300, tol=1e-3, pad=0):
    from noisediff_amd import noise_level as nl
    xd = torch.full((len(x) + pad,), float("nan"), dtype=torch.float64, device=DEV)
    yd = xd.clone()
    xd[:len(x)] = torch.from_numpy(np.asarray(x, np.float64))
    yd[:len(y)] = torch.from_numpy(np.asarray(y, np.float64))
    m = torch.tensor(len(x), dtype=torch.int32, device=DEV) if pad else None
    slope, icpt, steps = nl.theil_sen(xd, yd, m, pairs, max_iter, tol)
    assert slope.dtype == icpt.dtype == torch.float64 and steps.dtype == torch.int64
    return float(slope), float(icpt), int(steps)


def _close(got, want, gap, what):
    """16 x the gap between the restatement summing the pairs forwards and backwards, floor 1e-12 relative (the sums are long and can cancel:
    their conditioning is a property of the input)."""
    for k in range(2):
        tol = max(16 * float(gap[k]), 1e-12 * abs(want[k]))
        print(what, "slope" if k == 0 else "intercept", "got", got[k], "want", want[k], "diff", abs(got[k] - want[k]), "allowed", tol)
        assert abs(got[k] - want[k]) <= tol, (what, k)
    assert got[2] == want[2], what                                              # the step counts


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.FIT_CASES))
def test_theil_sen_against_the_restatement(gold, name):
    x, y, pairs, max_iter, tol = R.fit_case(name)
    got = _fit_gpu(x, y, pairs, max_iter, tol, pad=0 if name == "m8" else 37)
    _close(got, gold[f"fit.{name}"], gold[f"fit.{name}.gap"], name)
    assert got == _fit_gpu(x, y, pairs, max_iter, tol, pad=5)                   # the same bits, whatever the capacity of x and y
    if name == "m100.exhausted":
        assert got[2] == 3
    if name == "m700":
        assert len(x) * (len(x) - 1) // 2 == 244650


@pytest.mark.gpu
def test_theil_sen_on_the_golden_curve_and_the_small_cases(gold):
    count, _, std = R.stats(R.table(gold["a.clean"], gold["a.noisy"])[0])
    levels, x, y = R.curve(count, std)
    assert levels.size == 81
    want = R.theil_sen(x, y)
    assert list(want[:2]) == gold["a.restated"][:2].tolist()
    _close(_fit_gpu(x, y, pad=11), want, gold["fit.a.gap"], "golden curve")
    for pad in (0, 3):
        one = _fit_gpu(np.ones(1), np.ones(1), pad=pad)
        assert np.isnan(one[0]) and np.isnan(one[1]) and one[2] == 0              # the reference raises there
    from noisediff_amd import noise_level as nl
    z = torch.zeros(4, dtype=torch.float64, device=DEV)
    slope, icpt, steps = nl.theil_sen(z, z, torch.tensor(0, dtype=torch.int32, device=DEV))
    assert (float(slope), float(icpt), int(steps)) == (0.0, 0.0, 0)
    assert not any(np.isfinite(v) for v in _fit_gpu([0.25, 0.25, 0.5], [1.0, 2.0, 3.0])[:2])            # equal x: the caller's contract, nothing finite


@pytest.mark.gpu
def test_get_poisson_lambda_end_to_end_against_the_reference(gold):
    from noisediff_amd import noise_level as nl
    clean, noisy = torch.from_numpy(gold["a.clean"]).to(DEV), torch.from_numpy(gold["a.noisy"]).to(DEV)
    lam, sig = nl.get_poisson_lambda(clean, noisy)
    assert lam.device.type == "cuda" and lam.dtype == sig.dtype == torch.float64
    gap = gold["a.gap"]
    print("lambda", float(lam), "reference", gold["a.lambda"], "sigma", float(sig), "reference", gold["a.sigma"], "gap", gap)
    assert abs(float(lam) - gold["a.lambda"]) <= 4 * gap[0] and abs(float(sig) - gold["a.sigma"]) <= 4 * gap[1]
    lam2, sig2 = nl.get_poisson_lambda(clean, noisy)
    assert torch.equal(lam, lam2) and torch.equal(sig, sig2)                    # bitwise
    mom = nl.LevelMoments(device=DEV)
    cb, nb = torch.from_numpy(gold["b.clean"]).to(DEV), torch.from_numpy(gold["b.noisy"]).to(DEV)
    assert nl.get_poisson_lambda_all_images(cb[:2], nb[:2], mom) is mom
    nl.get_poisson_lambda_all_images(cb[2:], nb[2:], mom)                       # one image in two parts: the table of the whole
    lam, sig = nl.get_regression_result_all_images(mom)
    gap = gold["b.gap"]
    assert abs(float(lam) - gold["b.lambda"]) <= 4 * gap[0] and abs(float(sig) - gold["b.sigma"]) <= 4 * gap[1]
    none = nl.get_poisson_lambda(torch.full((8,), 2.0, device=DEV), torch.zeros(8, device=DEV))           # nothing on the grid
    assert (float(none[0]), float(none[1])) == (0.0, 0.0)


@pytest.mark.gpu
def test_the_level_grid_is_the_packers_grid():
    """raw.load_pair on a small synthetic uint16 pair: every clean value it produces is on the grid (counters()[0] == 0), the codes above white
    and below black on the two end levels, and the fit equals the restatement's on the same tensors."""
    from noisediff_amd import noise_level as nl, raw
    rs = np.random.RandomState(21)
    H2, W2 = 48, 64
    codes = rs.choice(np.arange(raw.BLACK + 1, raw.BLACK + 2500), 90, replace=False)
    long_ = rs.choice(codes, (H2, W2)).astype(np.uint16)
    long_.ravel()[:12] = [0, 100, raw.BLACK, raw.BLACK, raw.BLACK, raw.WHITE, raw.WHITE, raw.WHITE + 1, 65535, raw.WHITE - 1, raw.WHITE - 1, raw.BLACK + 1]
    ratio = 100.0
    lam = (long_.astype(np.float64) - raw.BLACK).clip(0) / ratio
    short = np.clip(np.rint(raw.BLACK + lam + np.sqrt(lam + 4.0) * rs.standard_normal((H2, W2))), 0, 65535).astype(np.uint16)
    noisy, clean = raw.load_pair(short, long_, 100, ratio)
    mom = nl.LevelMoments(device=DEV).add(clean, noisy)
    assert mom.counters().cpu().tolist() == [0, 0]
    count = mom.stats()[0].cpu().numpy()
    assert count.sum() == clean.numel() and count[0] >= 5 and count[15871] >= 4 and count[15870] == 2 and count[1] >= 1
    got = nl.get_poisson_lambda(clean, noisy)
    want = R.get_poisson_lambda(clean.cpu().numpy(), noisy.cpu().numpy())
    assert want[3] <= 141
    count, _, std = R.stats(R.table(clean.cpu().numpy(), noisy.cpu().numpy())[0])
    gap = R.order_gap(*R.curve(count, std)[1:])
    _close((float(got[0]), float(got[1]), want[2]), want, gap, "load_pair")
    again = nl.get_poisson_lambda(clean, noisy)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


@pytest.mark.gpu
def test_a_captured_graph_replays_to_the_eager_result():
    from noisediff_amd import noise_level as nl
    n = 5000
    clean, noisy = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    mom = nl.LevelMoments(device=DEV)

    def run():
        mom.reset()
        mom.add(clean, noisy)
        x, y, m = nl.level_curve(mom, True)
        return (m,) + nl.theil_sen(x, y, m, max_iter=20)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run()
    for seed in (31, 32):
        c, v = R.level_frame(seed, (n,), 60)
        clean.copy_(torch.from_numpy(c))
        noisy.copy_(torch.from_numpy(v))
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in res]
        table = mom.table.clone()
        eager = run()
        torch.cuda.synchronize()
        print("graph", seed, "replayed", [t.tolist() for t in replayed], "eager", [t.tolist() for t in eager], "table words that differ",
              int((table != mom.table).sum()))
        assert torch.equal(table, mom.table)
        for a, b, what in zip(replayed, eager, ("m", "slope", "intercept", "steps")):
            assert torch.equal(a, b), what
        count, _, std = R.stats(R.table(c, v)[0])
        levels, x, y = R.curve(count, std)
        assert int(replayed[0]) == levels.size <= 141
        _close((float(replayed[1]), float(replayed[2]), int(replayed[3])), R.theil_sen(x, y, max_iter=20), R.order_gap(x, y, max_iter=20), f"graph {seed}")
