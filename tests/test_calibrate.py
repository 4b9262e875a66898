"""noisediff_amd.calibrate: the physics-based model's table row from dark frames (csrc/calibrate.hip).

CPU: the numpy restatement (tests/calibrate_ref.py) against scipy (the order-statistic medians bit for bit, the Tukey-lambda quantile, the
probability plot and the ppcc objective); every refusal of the host checks; the header, the ctypes signatures and the exports; ``table_row``.
GPU: the integer sums, the row sums, the residual and the mean frame bit for bit against the restatement at the frame readers' three vector
widths; the objective at fixed shapes; the search against scipy's bounded Brent on the restated objective; the probability plots against
``scipy.stats.probplot``; determinism and independence of the stack; the public path.  Outputs are pre-filled with NaN (integers: a sentinel),
one frame longer than written, and the tail is checked.

Tolerances (none fitted to a GPU result).  For r: ``tol_r = 2 |dq|_2 / |q - mean q|_2 + (log2 n + 8) 2^-53 4``: a perturbation dq of the quantiles
turns the unit vector (q - mean q) / |q - mean q| by at most |dq| / |q - mean q| and r is a cosine, twice for the two sides; the second term is
the rounding of sums of n terms formed as a tree (log2 n levels, plus the short serial runs and the closing operations).  dq is the bound of
the quantile's own error per element (``calibrate_ref.quantile_tolerance``).  Slope and intercept take the same relative bound times |slope| and
times max |x|.  The standard normal quantile of the device (ocml's normcdfinv) was measured ONCE on an MI355X against ``scipy.special.ndtri`` on
the medians of this file's sizes (n = 1872, 14784, 20480, 139264): the largest absolute difference was 1.7764e-15 (NDTRI_MEASURED); dq of the normal
plot is four times that, because the measurement sees a few grids and not all arguments."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import calibrate_ref as CR

DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI, XTOL, MAX_EVAL = -0.45, 0.5, 1e-6, 32
LAMS = (LO, -0.0441, 0.0, 1e-9, 0.1474653, HI)
# max |normcdfinv(m) - ndtri(m)| on an MI355X over the medians of n = 1872, 14784, 20480, 139264: 8.88e-16, 1.33e-15, 1.78e-15, 1.78e-15 (4 ulp of
# a quantile in [2, 4); 8.4e-16 relative to |q| at the most)
NDTRI_MEASURED = 1.7764e-15
A, B, C25600 = (0.1474653, 0.707, 0.14), (-0.0441, 3.228, 0.989), (-0.0909, 12.18, 2.276)
# name: (N, H2, W2, the (lam, sTL, sR) of its frames in turn)
TUKEY_CASES = {"w78": (1, 12, 156, [(0.02, 1.18, 0.36)]), "w77": (3, 96, 154, [A, B, A]), "w80": (2, 128, 160, [C25600]), "big": (1, 256, 544, [A])}
SEARCH_CASES = tuple(TUKEY_CASES) + ("uniform",)
ALL_CASES = SEARCH_CASES + ("const",)


def to_mosaic(packed):
    """(N, 4, h, w) -> (N, 2h, 2w)."""
    N, _, h, w = packed.shape
    out = np.empty((N, 2 * h, 2 * w), packed.dtype)
    for c, (r, q) in enumerate(CR.SITES):
        out[:, r::2, q::2] = packed[:, c]
    return out


@functools.lru_cache(maxsize=None)
def frames_of(name):
    """The integer codes of a case: rint(512 + sTL Q(u, lam) + sR g[c, Y]) from numpy's generator, fixed seeds; many ties, as dark frames have."""
    if name == "const":
        return np.full((1, 96, 154), 512, np.uint16)
    seed = 20240 + ALL_CASES.index(name)
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return to_mosaic(np.rint(512 + rng.uniform(-8, 8, (1, 4, 64, 80))).astype(np.uint16))
    N, H2, W2, params = TUKEY_CASES[name]
    h, w = H2 // 2, W2 // 2
    packed = np.empty((N, 4, h, w))
    for n in range(N):
        lam, sTL, sR = params[n % len(params)]
        packed[n] = 512 + sTL * CR.tukey_quantile(rng.uniform(1e-9, 1 - 1e-9, (4, h, w)), lam) + sR * rng.standard_normal((4, h, 1))
    return to_mosaic(np.clip(np.rint(packed), 0, 65535).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def sorted_ref(name):
    """The restatement's residual of a case, black subtracted, sorted per frame: (N, n) float64.  Read-only."""
    xs = np.sort(CR.residuals(frames_of(name)), axis=1)
    xs.setflags(write=False)
    return xs


def tol_r(n, lam=None, dq=None):
    m = CR.medians(n)
    if dq is None:
        q, dq = CR.tukey_quantile(m, lam), CR.quantile_tolerance(m, lam)
    else:
        from scipy.special import ndtri
        q, dq = ndtri(m), np.full(n, dq)
    return 2 * np.linalg.norm(dq) / np.linalg.norm(q - q.mean()) + (math.log2(n) + 8) * 2.0 ** -53 * 4


@functools.lru_cache(maxsize=None)
def scipy_search(name, frame):
    """scipy's bounded Brent on the restated objective: (lam, f, nfev, f'' by a central second difference of step 1e-3)."""
    optimize = pytest.importorskip("scipy.optimize")
    xs = sorted_ref(name)[frame]
    f = functools.lru_cache(maxsize=None)(lambda lam: CR.objective(xs, float(lam)))
    res = optimize.minimize_scalar(f, bounds=(LO, HI), method="bounded", options={"xatol": XTOL})
    d = 1e-3
    return float(res.x), float(res.fun), int(res.nfev), (f(res.x + d) - 2 * f(res.x) + f(res.x - d)) / d ** 2, f


# --------------------------------------------------------------------------- CPU 1: the restatement against scipy

def test_medians_equal_scipy_bit_for_bit():
    morestats = pytest.importorskip("scipy.stats._morestats")
    for n in (3, 4, 1872, 14784, 20480, 139264):
        assert np.array_equal(CR.medians(n), morestats._calc_uniform_order_statistic_medians(n)), n


def test_quantile_agrees_with_scipy_within_the_model():
    stats = pytest.importorskip("scipy.stats")
    for n in (1872, 14784):
        m = CR.medians(n)
        for lam in LAMS:
            want, got = stats.tukeylambda.ppf(m, lam), CR.tukey_quantile(m, lam)
            nz = want != 0
            print(f"n {n} lam {lam}: max relative difference to scipy {np.abs(got[nz] / want[nz] - 1).max():.2e}")
            assert (np.abs(got - want) <= CR.quantile_tolerance(m, lam)).all(), (n, lam)


@pytest.mark.parametrize("name", ["w78", "w77"])
def test_restated_plot_agrees_with_scipy(name):
    stats = pytest.importorskip("scipy.stats")
    special = pytest.importorskip("scipy.special")
    for x in sorted_ref(name):
        n = len(x)
        for lam in LAMS:
            (osm, osr), (slope, icpt, r) = stats.probplot(x, sparams=(lam,), dist="tukeylambda")
            got = CR.probplot(x, lam)
            t = tol_r(n, lam)
            assert abs(got[2] - r) <= t and abs(got[0] - slope) <= t * abs(slope) and abs(got[1] - icpt) <= t * np.abs(x).max(), (name, lam, got, (slope, icpt, r))
            r2 = stats.pearsonr(stats.tukeylambda.ppf(CR.medians(n), lam), x)[0]                 # ppcc_max's objective
            assert abs(CR.objective(x, lam) - (1 - r2)) <= t, (name, lam)
        _, (slope, icpt, r) = stats.probplot(x)
        got = CR.probplot(x, normal_quantile=special.ndtri)
        t = tol_r(n, dq=4 * 2.0 ** -53)
        assert abs(got[2] - r) <= t and abs(got[0] - slope) <= t * abs(slope) and abs(got[1] - icpt) <= t * np.abs(x).max(), (name, got, (slope, icpt, r))


def test_restated_residual_is_row_centred():
    f = frames_of("w77")
    for mode in ("black", "mean"):
        x = CR.residuals(f, 512, mode).reshape(3, 4, 48, 77)
        assert np.abs(x.sum(axis=3)).max() < 1e-9
    t, D = CR.pixel_values(f, 512, "mean")
    assert D == 3 and (t.sum(axis=0) == 0).all()                               # N code - T sums to zero over the stack, exactly


# --------------------------------------------------------------------------- CPU 2: refusals, the binding, table_row

def test_refusals_before_any_device_call():
    from noisediff_amd import calibrate as K
    from noisediff_amd._lib import HipError
    ok = np.zeros((2, 8, 12), np.uint16)
    for shape in ((2, 7, 12), (2, 8, 11), (0, 8, 12), (2, 2, 12), (2, 8, 2)):          # odd sides, N < 1, a side too small for the row statistics
        with pytest.raises(ValueError):
            K.calibrate_dark_frames(np.zeros(shape, np.uint16))
    for kw in (dict(black=512.5), dict(black=-1), dict(lo=0.5, hi=0.5), dict(lo=0.6), dict(lo=-0.5), dict(lo=-0.7), dict(xtol=0.0), dict(xtol=-1e-6),
               dict(max_eval=2), dict(max_eval=65), dict(subtract="median")):
        with pytest.raises(ValueError):
            K.calibrate_dark_frames(ok, **kw)
    with pytest.raises(ValueError, match="32767"):
        K.check_subtract((32768, 8, 12))
    with pytest.raises(ValueError):
        K.check_subtract((1, 8, 12), 512, "mean")                               # one frame minus its own mean
    stack = K.DarkStack.__new__(K.DarkStack)                                    # (a stack without a device: the checks read these three)
    stack.count, stack.H2, stack.W2 = 3, 8, 12
    assert K.check_subtract((3, 8, 12), 512, "mean", stack) == (3, 8, 12, 512, 3)
    for shape in ((2, 8, 12), (3, 8, 16), (3, 10, 12)):                         # a count or a shape that is not the stack's
        with pytest.raises(ValueError):
            K.check_subtract(shape, 512, "mean", stack)
    with pytest.raises(ValueError):
        K.check_subtract((3, 8, 12), 512, "black", stack)
    stack.device, stack.sums = torch.device("cuda", 0), None
    stack.count = 32766
    with pytest.raises(ValueError, match="32767"):
        stack.add(np.zeros((2, 8, 12), np.uint16))
    x = torch.zeros(2, 16, dtype=torch.float64)
    for bad in (torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 16, dtype=torch.float32)):                   # n < 3, not float64
        with pytest.raises(ValueError):
            K.ppcc_max(bad)
        with pytest.raises(ValueError):
            K.probplot(bad)
    for kw in (dict(lo=-0.5), dict(lo=0.3, hi=0.2), dict(xtol=0), dict(max_eval=2), dict(max_eval=65)):
        with pytest.raises(ValueError):
            K.ppcc_max(x, **kw)
    for call in (lambda: K.ppcc_max(x), lambda: K.probplot(x), lambda: K.calibrate_dark_frames(torch.zeros(2, 8, 12, dtype=torch.int16))):
        with pytest.raises(HipError):                                           # CPU tensors: no fallback
            call()


def test_header_signatures_and_exports_agree():
    import ctypes
    import noisediff_amd
    from noisediff_amd import _lib as L
    from noisediff_amd import build, calibrate
    assert "calibrate" in build.SOURCES
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    ctype = lambda decl: (L.vp if "*" in decl else {"int": L.i32, "int64_t": L.i64, "double": L.f64}[decl.replace("const", "").split()[0]])  # noqa: E731
    names = ("nd_dark_stack_add_u16", "nd_dark_stack_mean_f64", "nd_calib_row_sums_i64", "nd_calib_residual_f64", "nd_calib_row_stats_f64",
             "nd_calib_quantiles_f64", "nd_ppcc_workspace_bytes", "nd_probplot_f64", "nd_ppcc_max_f64")
    for name in names:
        ret, args = re.search(r"^(int|int64_t) " + name + r"\(([^)]*)\);", header, re.M).groups()
        want = (ctype(ret), [ctype(a) for a in args.split(",")])
        assert L.SIGNATURES[name] == want, (name, L.SIGNATURES[name], want)
    assert ("nd_ppcc_workspace_bytes" in L._UNCHECKED) and not (set(names) - {"nd_ppcc_workspace_bytes"}) & L._UNCHECKED
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in names)
    for name in ("DarkStack", "calibrate_dark_frames", "table_row", "ppcc_max", "probplot"):
        assert name in noisediff_amd.__all__ and getattr(noisediff_amd, name) is getattr(calibrate, name), name


def test_table_row_feeds_the_camera_model():
    from noisediff_amd import calibrate as K
    from noisediff_amd.physics_noise import TABLE_KEYS, CameraNoiseModel
    many = {"lam": np.array([0.1, 0.2, 0.3]), "sigTL": np.array([1.0, 2.0, 3.0]), "sigGs": np.array([2.0, 2.0, 2.0]), "sigR": np.array([0.1, 0.3, 0.2]),
            "sigR_pmn": np.array([0.2, 0.4, 0.3]), "bias": np.array([[0.0, 1.0, 2.0, 3.0]] * 3) + np.arange(3)[:, None]}
    row = K.table_row(many, K=1.5, q=1 / 16384)
    assert tuple(row) == TABLE_KEYS and row["Kmax"] == 1.5 and row["q"] == 1 / 16384
    assert row["lam"] == pytest.approx(0.2) and row["sigTL"] == pytest.approx(2.0) and row["sigTLsig"] == pytest.approx(1.0) and row["sigGssig"] == 0.0
    assert row["sigR"] == pytest.approx(0.2) and row["sigRsig"] == pytest.approx(0.1) and row["bias"] == pytest.approx(2.5) and row["biassig"] == pytest.approx(1.0)
    assert K.table_row(many, 1.5, 0.0, row="pmn")["sigR"] == pytest.approx(0.3)
    one = {k: v[:1] for k, v in many.items()}
    row1 = K.table_row(one, K=1.5, q=0.0)
    assert tuple(row1) == TABLE_KEYS and all(row1[k] == 0.0 for k in TABLE_KEYS if k.endswith("sig")) and row1["sigTL"] == 1.0
    params = CameraNoiseModel({100: row}).draw([100, 100], seed=3, read="tukey")
    assert params["lam"].tolist() == [row["lam"]] * 2 and (params["s_read"] > 0).all() and np.isfinite(params["bias"]).all()
    for bad in (dict(K=0.0, q=0.0), dict(K=1.0, q=-1.0), dict(K=1.0, q=0.0, row="raw")):
        with pytest.raises(ValueError):
            K.table_row(many, **bad)


# --------------------------------------------------------------------------- GPU 1: the exact quantities

SENTINEL = -(1 << 62)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w78", "w77", "w80"])                        # w = 78, 77, 80: two, one and four packed columns per thread
def test_sums_row_sums_and_residual_bit_for_bit(name):
    from noisediff_amd import calibrate as K
    f = frames_of(name)
    N, H2, W2 = f.shape
    h, w = H2 // 2, W2 // 2
    dev_f = torch.from_numpy(f.view(np.int16)).to(DEV)
    stack = K.DarkStack(H2, W2, DEV).add(dev_f)
    assert stack.count == N and np.array_equal(stack.sums.cpu().numpy(), CR.stack_sums(f))
    assert np.array_equal(stack.mean().cpu().numpy(), CR.stack_mean(CR.stack_sums(f), N))
    split = K.DarkStack(H2, W2, DEV)
    for n in range(N):
        split.add(f[n])                                                         # one frame per call, from the host
    assert split.count == N and torch.equal(split.sums, stack.sums)
    for mode in ("black", "mean") if N > 1 else ("black",):
        R = torch.full((N + 1, 4, h), SENTINEL, dtype=torch.int64, device=DEV)
        x = torch.full((N + 1, 4 * h * w), float("nan"), dtype=torch.float64, device=DEV)
        st = stack if mode == "mean" else None
        assert K.row_sums(dev_f, 512, mode, st, out=R) is R and K.residuals(dev_f, R[:N], 512, mode, st, out=x) is x
        assert np.array_equal(R[:N].cpu().numpy(), CR.row_sums(f, 512, mode)), (name, mode)
        got, want = x[:N].cpu().numpy(), CR.residuals(f, 512, mode)
        assert np.array_equal(got, want), (name, mode, np.abs(got - want).max())
        assert (R[N] == SENTINEL).all() and torch.isnan(x[N]).all()
        if mode == "mean":                                                      # the stack made inside equals the one given
            assert torch.equal(K.residuals(dev_f, K.row_sums(dev_f, 512, "mean"), 512, "mean"), x[:N])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["black", "mean"])
def test_row_statistics(mode):
    """sigR_pmn and the bias come from integers and exact divisors: bit for bit.  V_x is a sum of n squares formed as a tree: relative
    (log2 n + 8) 2^-53 4, and sigR^2 = v - V_x / (w - 1) inherits it, plus the subtraction's own rounding."""
    from noisediff_amd import calibrate as K
    f = frames_of("w77")
    N, w, n = 3, 77, 4 * 48 * 77
    res = K.calibrate_dark_frames(f, 512, mode).cpu()
    undo = math.sqrt(N / (N - 1.0)) if mode == "mean" else 1.0
    for i, want in enumerate(CR.row_stats(f, 512, mode)):
        assert np.array_equal(res["bias"][i], want["bias"])
        assert res["sigR_pmn"][i] == want["sigR_pmn"] * undo
        v, tol_v = want["sigR_pmn"] ** 2, (math.log2(n) + 8) * 2.0 ** -53 * 4
        print(f"{mode} frame {i}: sigR_pmn {want['sigR_pmn']:.6f} sigR {want['sigR']:.6f} gpu {res['sigR'][i]:.6f} V_x {want['V_x']:.6f}")
        assert abs((res["sigR"][i] / undo) ** 2 - want["sigR"] ** 2) <= tol_v * want["V_x"] / (w - 1) + 8 * 2.0 ** -53 * v
        assert 0 < want["sigR"] < want["sigR_pmn"]


# --------------------------------------------------------------------------- GPU 2: the objective, the search, the plots

def _check_plot(got, want, t, xmax, what):
    slope, icpt, r = (float(v) for v in got)
    print(f"{what}: r {r:.17g} want {want[2]:.17g} |d| {abs(r - want[2]):.2e} tol {t:.2e}; slope |d| / |slope| {abs(slope - want[0]) / abs(want[0]):.2e}; "
          f"intercept |d| / max|x| {abs(icpt - want[1]) / xmax:.2e}")
    assert abs(r - want[2]) <= t and abs(slope - want[0]) <= t * abs(want[0]) and abs(icpt - want[1]) <= t * xmax, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_objective_at_fixed_shapes(name):
    from noisediff_amd import calibrate as K
    xs = sorted_ref(name)
    N, n = xs.shape
    dev_x = torch.from_numpy(np.array(xs)).to(DEV)
    for lam in LAMS:
        out = torch.full((N + 1, 6), float("nan"), dtype=torch.float64, device=DEV)
        slope, icpt, r = K.probplot(dev_x, torch.full((N,), lam, dtype=torch.float64, device=DEV), out=out)
        assert torch.isnan(out[N]).all()
        for i in range(N):
            want = CR.probplot(xs[i], lam)
            if name == "const":
                assert math.isnan(want[2]) and math.isnan(float(r[i])) and float(slope[i]) == 0.0 and float(icpt[i]) == 0.0
                continue
            _check_plot((slope[i], icpt[i], r[i]), want, tol_r(n, lam), np.abs(xs[i]).max(), f"{name}[{i}] lam {lam}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEARCH_CASES)
def test_search_against_scipy_bounded(name):
    """n_eval < max_eval is a condition; optimality f_ref(lam_gpu) <= f_ref(lam_scipy) + 2 tol_r + f'' (3 xtol)^2 / 2 and location
    |lam_gpu - lam_scipy| <= 3 xtol + sqrt(4 tol_r / f''): two searches that stop within 3 xtol of their own minimum of objectives that differ by
    tol_r at most cannot lie further apart on a parabola of curvature f''."""
    from noisediff_amd import calibrate as K
    xs = sorted_ref(name)
    N, n = xs.shape
    out = torch.full((N + 1, 3), float("nan"), dtype=torch.float64, device=DEV)
    lam, r, n_eval = K.ppcc_max(torch.from_numpy(np.array(xs)).to(DEV), LO, HI, XTOL, MAX_EVAL, out=out)
    assert torch.isnan(out[N]).all() and n_eval.dtype == torch.int64
    for i in range(N):
        lam_s, f_s, nfev, curv, f = scipy_search(name, i)
        lam_g, t = float(lam[i]), tol_r(n, lam_s)
        print(f"{name}[{i}]: lam gpu {lam_g:.9f} scipy {lam_s:.9f} |d| {abs(lam_g - lam_s):.2e}; n_eval gpu {int(n_eval[i])} scipy {nfev}; f'' {curv:.3f}; "
              f"f_ref(gpu) - f_ref(scipy) {f(lam_g) - f_s:.2e}; tol_r {t:.2e}")
        assert 3 <= int(n_eval[i]) < MAX_EVAL
        assert LO < lam_g < HI and curv > 0
        assert f(lam_g) <= f_s + 2 * t + 0.5 * curv * (3 * XTOL) ** 2
        assert abs(lam_g - lam_s) <= 3 * XTOL + math.sqrt(4 * t / curv)
        assert abs((1 - float(r[i])) - f(lam_g)) <= tol_r(n, lam_g)


@pytest.mark.gpu
def test_constant_frame_and_determinism():
    from noisediff_amd import calibrate as K
    xs = sorted_ref("w77")
    dev_x = torch.from_numpy(np.array(xs)).to(DEV)
    first = [t.clone() for t in K.ppcc_max(dev_x)]
    again = K.ppcc_max(dev_x)
    alone = K.ppcc_max(dev_x[1:2].clone())
    mixed = K.ppcc_max(torch.cat([dev_x[1:2], torch.from_numpy(np.array(sorted_ref("const"))).to(DEV)]))
    for a, b, c, d in zip(first, again, alone, mixed):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))           # the same bits on a repeated call
        assert torch.equal(a[1:2].view(torch.int64), c.view(torch.int64))      # frame 1 alone equals frame 1 in the stack
        assert torch.equal(a[1:2].view(torch.int64), d[:1].view(torch.int64))  # and next to a constant frame
    lam, r, n_eval = mixed
    assert math.isnan(float(lam[1])) and math.isnan(float(r[1])) and 1 <= int(n_eval[1]) <= MAX_EVAL
    lam_t = first[0]
    p1, p2 = K.probplot(dev_x, lam_t), K.probplot(dev_x, lam_t)
    alone_p = K.probplot(dev_x[1:2].clone(), lam_t[1:2].clone())
    for a, b, c in zip(p1, p2, alone_p):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a[1:2].view(torch.int64), c.view(torch.int64))
    res1, res2 = K.calibrate_dark_frames(frames_of("w77")).cpu(), K.calibrate_dark_frames(frames_of("w77")).cpu()
    assert all(np.array_equal(res1[k], res2[k]) for k in res1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEARCH_CASES)
def test_probability_plots_against_scipy(name):
    """At the GPU's own shape, so that the search's freedom does not enter; the normal plot with dq = 4 NDTRI_MEASURED."""
    stats = pytest.importorskip("scipy.stats")
    from noisediff_amd import calibrate as K
    xs = sorted_ref(name)
    N, n = xs.shape
    dev_x = torch.from_numpy(np.array(xs)).to(DEV)
    lam = K.ppcc_max(dev_x)[0]
    tukey, gauss = K.probplot(dev_x, lam), K.probplot(dev_x)
    for i in range(N):
        lam_g = float(lam[i])
        _, want = stats.probplot(xs[i], sparams=(lam_g,), dist="tukeylambda")
        _check_plot([v[i] for v in tukey], want, tol_r(n, lam_g), np.abs(xs[i]).max(), f"{name}[{i}] tukeylambda at {lam_g:.7f}")
        _, want = stats.probplot(xs[i])
        _check_plot([v[i] for v in gauss], want, tol_r(n, dq=4 * NDTRI_MEASURED), np.abs(xs[i]).max(), f"{name}[{i}] normal")


@pytest.mark.gpu
def test_normal_quantile_within_four_times_the_measurement():
    special = pytest.importorskip("scipy.special")
    from noisediff_amd import calibrate as K
    for n in (1872, 14784, 20480, 139264):
        m = CR.medians(n)
        err = np.abs(K.quantiles(n, device=DEV).cpu().numpy() - special.ndtri(m)).max()
        print(f"n {n}: max |normcdfinv - ndtri| {err:.3e}")
        assert err <= 4 * NDTRI_MEASURED
        for lam in (LO, 0.0, HI):
            q = K.quantiles(n, lam, device=DEV).cpu().numpy()
            assert (np.abs(q - CR.tukey_quantile(m, lam)) <= CR.quantile_tolerance(m, lam)).all(), (n, lam)


# --------------------------------------------------------------------------- GPU 3: the public path

@pytest.mark.gpu
def test_public_path_dark_frames_to_batches():
    """physics_frames draws dark frames from the ISO 1600 fixture row; they are rounded to codes and calibrated; the row feeds the generator.
    The assertions are GPU against scipy on the same codes; recovered against true parameters is reported, not asserted."""
    import json
    stats = pytest.importorskip("scipy.stats")
    from noisediff_amd import calibrate as K
    from noisediff_amd.physics_noise import TABLE_KEYS, CameraNoiseModel, PhysicsNoiseBatchBuilder, physics_frames
    with open(os.path.join(REPO, "tests", "golden", "physics_params.json")) as fh:
        true = json.load(fh)["rows"]["1600"]
    H2, W2, Bn, wb = 96, 128, 3, 15871.0
    black = np.full((1, H2, W2), 512, np.uint16)
    params = dict(K=true["Kmax"], s_read=true["sigTL"], read_kind="tukey", lam=true["lam"], s_row=true["sigR"], q=true["q"], bias=true["bias"])
    noisy, _ = physics_frames(black, [0] * Bn, 1.0, params, seed=11, clip01=False)
    codes = to_mosaic(np.clip(np.rint(noisy.double().cpu().numpy() * wb + 512.0), 0, 65535).astype(np.uint16))
    res = K.calibrate_dark_frames(codes)
    got = res.cpu()
    xs = np.sort(CR.residuals(codes), axis=1)
    n = xs.shape[1]
    for i in range(Bn):
        f = lambda lam: CR.objective(xs[i], float(lam))                         # noqa: E731
        from scipy.optimize import minimize_scalar
        s = minimize_scalar(f, bounds=(LO, HI), method="bounded", options={"xatol": XTOL})
        curv, t = (f(s.x + 1e-3) - 2 * f(s.x) + f(s.x - 1e-3)) / 1e-6, tol_r(n, float(s.x))
        lam_g = float(got["lam"][i])
        assert int(got["n_eval"][i]) < MAX_EVAL and abs(lam_g - s.x) <= 3 * XTOL + math.sqrt(4 * t / curv)
        _, want = stats.probplot(xs[i], sparams=(lam_g,), dist="tukeylambda")
        _check_plot((got["sigTL"][i], got["uTL"][i], got["rTL"][i]), want, tol_r(n, lam_g), np.abs(xs[i]).max(), f"frame {i} tukeylambda")
        _, want = stats.probplot(xs[i])
        _check_plot((got["sigGs"][i], got["uGs"][i], got["rGs"][i]), want, tol_r(n, dq=4 * NDTRI_MEASURED), np.abs(xs[i]).max(), f"frame {i} normal")
    row = K.table_row(res, K=true["Kmax"], q=true["q"])
    print("recovered", {k: round(row[k], 5) for k in TABLE_KEYS}, "true", {k: true[k] for k in TABLE_KEYS})
    assert tuple(row) == TABLE_KEYS and all(math.isfinite(v) for v in row.values())
    model = CameraNoiseModel({1600: row})
    builder = PhysicsNoiseBatchBuilder(32, clip01=False)
    out_noisy, out_clean = builder(black, [0, 0], [[0, 0], [8, 4]], 250.0, model.draw([1600, 1600], seed=5, read="tukey"), seed=3)
    assert out_noisy.shape == (2, 4, 32, 32) and torch.isfinite(out_noisy).all() and (out_clean == 0).all() and float(out_noisy.std()) > 0
