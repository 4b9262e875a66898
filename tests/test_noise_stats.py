"""noisediff_amd.noise_stats: value histograms, KL divergences and the 3 x 3 patch statistics with their line fit, on the HIP library.

CPU: the module and its entry points exist (without the feature every test of this file fails at import or at symbol lookup); the restatement
(tests/noise_stats_ref.py) equals every array captured from the reference (tests/golden/noise_stats.npz); the C entry points refuse each bad
argument before any HIP call and the Python layer refuses bad edges.
GPU: counts against the restatement (exact), the builders against the goldens, the divergences within the a-priori bound of an n_bins-term
fp64 sum, the patch statistics within util.derived, bitwise repeats, a captured graph and a generation run scored end to end."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import noise_stats_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
ENTRIES = ["nd_histogram_workspace_bytes", "nd_histogram_f32", "nd_histogram_chunk_elements", "nd_kl_div_f64", "nd_kl_div_hist_f64",
           "nd_patch_std_mean_workspace_bytes", "nd_patch_std_mean_f32"]
SENTINEL = -7
FIT_SHAPES = [(1, 1, 1, 7), (1, 2, 3, 3), (2, 4, 24, 40), (1, 1, 33, 257)]          # (1, 1, 33, 257): three rows and five columns of 16 x 64 tiles


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(REPO, "tests", "golden", "noise_stats.npz"))
    return {k: z[k] for k in z.files}


def _key(shape):
    return "x".join(map(str, shape))


# --------------------------------------------------------------------------- CPU

def test_the_module_and_its_entry_points_exist():
    """Fails without the feature: the module, the translation unit and the declared, exported and bound entry points."""
    from noisediff_amd import _lib as L, build, noise_stats
    import noisediff_amd
    assert "noise_stats" in build.SOURCES
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("kld_edges", "get_histogram", "histogram_counts", "kl_div_forward", "kl_div_inverse", "kl_div_sym", "kl_div_3", "noise_kld",
                 "patch_std_mean", "poisson_lambda_by_patch"):
        assert getattr(noisediff_amd, name) is getattr(noise_stats, name), name
    assert lib.nd_histogram_chunk_elements() > 0


def test_kld_edges_are_the_reference_bits(gold):
    from noisediff_amd import noise_stats
    e = noise_stats.kld_edges()
    assert e.dtype == np.float64 and e.shape == (67,) and e.tobytes() == gold["kld_edges"].tobytes() == R.kld_edges().tobytes()
    assert gold["kld_edges"][33] == 8.326672684688674e-17 and gold["kld_edges"][65] == 0.10000000000000017       # np.arange's edges are not round
    assert gold["kld_edges"][0] == -1000.0 and gold["kld_edges"][66] == 1000.0
    assert np.arange(0.0, 1.0 + 1e-3, 1e-3).shape == (1001,) and R.default_edges().shape == (1001,)


def test_restatement_equals_every_golden_array(gold):
    e = gold["kld_edges"]
    assert np.array_equal(R.counts(gold["special"], e), gold["special.counts"])
    assert gold["special.counts"].sum() == 4 and [int(gold["special.counts"][i]) for i in (0, 32, 65)] == [1, 2, 1]
    for name in ("generated", "real"):
        x = gold[name]
        assert np.array_equal(R.counts(x, e), gold[f"{name}.counts"])
        h, centers = R.get_histogram(x, bin_edges=e)
        assert np.array_equal(h, gold[f"{name}.hist"]) and np.array_equal(centers, gold["kld_centers"])
        for s in range(x.shape[0]):
            assert np.array_equal(R.counts(x[s], e), gold[f"{name}.counts.per_sample"][s])
            assert np.array_equal(R.get_histogram(x[s], bin_edges=e)[0], gold[f"{name}.hist.per_sample"][s])
    h, centers = R.get_histogram(gold["unit"])
    assert np.array_equal(h, gold["unit.hist"]) and np.array_equal(centers, gold["unit.centers"])
    assert np.array_equal(R.counts(gold["unit"], R.default_edges()), gold["unit.counts"])
    for s in range(2):
        assert np.array_equal(R.get_histogram(gold["unit"][s])[0], gold["unit.hist.per_sample"][s])
    assert np.array(R.kl_div_3(gold["real.hist"], gold["generated.hist"])).tobytes() == gold["kl3"].tobytes()
    for s in range(3):
        got = np.array(R.kl_div_3(gold["real.hist.per_sample"][s], gold["generated.hist.per_sample"][s]))
        assert got.tobytes() == gold["kl3.per_sample"][s].tobytes()
    assert np.array(R.kl_div_3(gold["unit.hist.per_sample"][0], gold["unit.hist.per_sample"][1])).tobytes() == gold["kl3.unit"].tobytes()
    for shape in ((1, 2, 3, 3), (2, 4, 24, 40)):
        x = gold[f"fit.{_key(shape)}.x"]
        assert torch.equal(R.ramp_image(61 + sum(shape), shape), torch.from_numpy(x))
        std, mean = R.patch_std_mean(x, torch.float32)
        assert np.array_equal(std.numpy(), gold[f"fit.{_key(shape)}.std"]) and np.array_equal(mean.numpy(), gold[f"fit.{_key(shape)}.mean"])
    for shape in FIT_SHAPES:                  # sklearn's fit of the fp32 maps against the closed form on the same maps in float64
        x = gold[f"fit.{_key(shape)}.x"]
        std, mean = R.patch_std_mean(x, torch.float32)
        slope, icpt = R.line_fit(mean.numpy(), std.numpy())
        np.testing.assert_allclose(slope, gold[f"fit.{_key(shape)}.lambda"], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(icpt, gold[f"fit.{_key(shape)}.intercept"], rtol=2e-5, atol=1e-6)


def test_entry_points_refuse_each_bad_argument_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    fake, odd = C.c_void_p(4096), C.c_void_p(4100)        # never dereferenced: every call below fails its checks first
    chunk = lib.nd_histogram_chunk_elements()
    assert chunk > 0 and chunk % 4 == 0
    wsb = lib.nd_histogram_workspace_bytes
    assert wsb(1, 1, 66) == 66 * 4 and wsb(3, 1, 66) == 3 * wsb(1, 1, 66) and wsb(1, 2 * chunk + 3, 1000) >= 1000 * 4
    assert wsb(5, 24 * 4 * 512 * 512, 66) == 5 * wsb(1, 24 * 4 * 512 * 512, 66)
    assert wsb(0, 8, 66) == -1 and wsb(1, 0, 66) == -1 and wsb(1, -3, 66) == -1
    assert wsb(1, 8, 0) == -2 and wsb(1, 8, 4097) == -2 and wsb(1, 8, 4096) > 0
    h = lambda x, S, n, e, ne, c, w: lib.nd_histogram_f32(x, S, n, e, ne, c, w, None)  # noqa: E731
    for bad in range(4):
        a = [fake, fake, fake, fake]
        a[bad] = None
        assert h(a[0], 1, 8, a[1], 67, a[2], a[3]) == -1 and b"null" in lib.nd_last_error(), bad
    assert h(fake, 0, 8, fake, 67, fake, fake) == -1 and h(fake, 1, 0, fake, 67, fake, fake) == -1 and h(fake, -1, 8, fake, 67, fake, fake) == -1
    assert h(fake, 1, 8, fake, 1, fake, fake) == -2 and b"n_bins" in lib.nd_last_error()            # n_bins 0
    assert h(fake, 1, 8, fake, 4098, fake, fake) == -2                                              # n_bins 4097
    assert h(fake, 1, 8, odd, 67, fake, fake) == -1 and b"aligned" in lib.nd_last_error()
    assert h(fake, 1, 8, fake, 67, odd, fake) == -1 and b"aligned" in lib.nd_last_error()
    kl = lambda p, q, n_p, n_q, nb, S, qs, o: lib.nd_kl_div_f64(p, q, n_p, n_q, nb, S, qs, o, None)  # noqa: E731
    assert kl(None, fake, 8, 8, 66, 1, 1, fake) == -1 and kl(fake, None, 8, 8, 66, 1, 1, fake) == -1 and kl(fake, fake, 8, 8, 66, 1, 1, None) == -1
    assert kl(fake, fake, 8, 8, 66, 0, 1, fake) == -1 and kl(fake, fake, 8, 8, 0, 1, 1, fake) == -1
    assert kl(fake, fake, 0, 8, 66, 1, 1, fake) == -1 and kl(fake, fake, 8, -1, 66, 1, 1, fake) == -1
    assert kl(fake, fake, 8, 8, 66, 3, 2, fake) == -1 and b"q_sets" in lib.nd_last_error()
    assert kl(fake, fake, 8, 8, 66, 3, 0, fake) == -1 and kl(odd, fake, 8, 8, 66, 1, 1, fake) == -1
    assert lib.nd_kl_div_hist_f64(fake, fake, 66, 3, 2, fake, None) == -1 and lib.nd_kl_div_hist_f64(fake, None, 66, 3, 3, fake, None) == -1
    pw = lib.nd_patch_std_mean_workspace_bytes
    assert pw(1, 1, 1, 1) == 32 and pw(3, 2, 33, 257) == 6 * pw(1, 1, 33, 257)
    assert pw(0, 1, 8, 8) == -1 and pw(1, 0, 8, 8) == -1 and pw(1, 1, 0, 8) == -1 and pw(1, 1, 8, 0) == -1 and pw(1, 1, -8, 8) == -1
    ps = lambda x, f, w, B, Cc, H, W: lib.nd_patch_std_mean_f32(x, fake, fake, f, w, B, Cc, H, W, None)  # noqa: E731
    assert ps(None, fake, fake, 1, 1, 8, 8) == -1 and ps(fake, None, fake, 1, 1, 8, 8) == -1 and ps(fake, fake, None, 1, 1, 8, 8) == -1
    assert ps(fake, fake, fake, 0, 1, 8, 8) == -1 and ps(fake, fake, fake, 1, 0, 8, 8) == -1
    assert ps(fake, fake, fake, 1, 1, 0, 8) == -1 and ps(fake, fake, fake, 1, 1, 8, 0) == -1 and ps(fake, fake, fake, 1, 1, 8, -2) == -1
    assert ps(fake, odd, fake, 1, 1, 8, 8) == -1 and b"aligned" in lib.nd_last_error()


def test_python_layer_refuses_bad_edges_and_cpu_tensors():
    from noisediff_amd import _lib as L, noise_stats as ns
    for bad in ([0.0, 0.5, 0.5, 1.0], [0.0, 0.6, 0.5, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [-np.inf, 0.0, 1.0], [0.0], np.zeros((2, 2)),
                np.arange(4098.0)):
        with pytest.raises(ValueError):
            ns.check_edges(bad)
    assert ns.check_edges([0, 1]).dtype == np.float64 and ns.check_edges(np.arange(4097.0)).size == 4097
    x = torch.zeros(2, 4, 8, 8)
    for call in (lambda: ns.histogram_counts(x, ns.kld_edges()), lambda: ns.get_histogram(x), lambda: ns.noise_kld(x, x), lambda: ns.patch_std_mean(x),
                 lambda: ns.poisson_lambda_by_patch(x), lambda: ns.kl_div_3(torch.zeros(66, dtype=torch.float64), torch.zeros(66, dtype=torch.float64))):
        with pytest.raises(L.HipError, match="no CPU path"):
            call()


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


LAYOUTS = {1: lambda: np.array([-0.25, 0.5]), 2: lambda: np.array([-1.0, 0.0, 1.0]), 66: R.kld_edges, 1000: R.default_edges,
           4096: lambda: -0.3 + np.cumsum(np.concatenate(([0.0], np.random.RandomState(4).uniform(0.5, 1.5, 4096)))) * (0.6 / 4096)}     # uneven widths


def _values(seed, n, edges):
    """n fp32 values around the edges: a Gaussian spanning the interior, some edges themselves, some values outside, a NaN and an inf."""
    rs = np.random.RandomState(seed)
    lo, hi = (edges[1], edges[-2]) if edges.size > 3 else (edges[0], edges[-1])
    v = rs.normal((lo + hi) / 2, (hi - lo) / 4 + 1e-3, n)
    k = rs.randint(0, n, max(n // 8, 1))
    v[k] = edges[rs.randint(0, edges.size, k.size)]
    v = v.astype(np.float32)
    if n >= 16:
        v[rs.randint(0, n, 3)] = [np.nan, np.inf, -np.inf]
    return v


def _hist_raw(x_np, S, n, edges_d, offset=0, tail=5):
    """nd_histogram_f32 on a copy of x that starts ``offset`` floats into its buffer; counts are sentinel-filled and ``tail`` rows too long."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    n_bins = edges_d.numel() - 1
    buf = torch.full((S * n + offset + 4,), float("nan"), device=DEV)
    buf[offset:offset + S * n] = torch.from_numpy(np.ascontiguousarray(x_np).reshape(-1)).to(DEV)
    counts = torch.full((S + tail, n_bins), SENTINEL, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(L.call("nd_histogram_workspace_bytes", S, n, n_bins)), dtype=torch.uint8, device=DEV)
    L.call("nd_histogram_f32", buf.data_ptr() + 4 * offset, S, n, edges_d.data_ptr(), n_bins + 1, counts.data_ptr(), ws.data_ptr(), _stream(DEV))
    torch.cuda.synchronize()
    got = _np(counts)
    assert (got[S:] == SENTINEL).all(), "wrote past the S x n_bins counts"
    return got[:S]


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", sorted(LAYOUTS))
def test_histogram_counts_equal_the_restatement(n_bins):
    from noisediff_amd import _lib as L, noise_stats as ns
    chunk = L.load().nd_histogram_chunk_elements()
    edges = LAYOUTS[n_bins]()
    assert edges.size == n_bins + 1
    ed = ns.device_edges(edges, DEV)
    for n in (1, 63, 64, 65, 255, 1025, chunk, chunk + 1, 2 * chunk + 3):
        x = _values(n_bins + n, 3 * n, edges).reshape(3, n)
        ref = np.stack([R.counts(x[s], edges) for s in range(3)])
        alone = _hist_raw(x[:1], 1, n, ed)
        assert np.array_equal(alone, ref[:1]), (n, "S=1")
        for offset in (0, 1, 2, 3):                       # off 16 bytes: the scalar loads; with n odd the later sets are off 16 bytes anyway
            got = _hist_raw(x, 3, n, ed, offset)
            assert np.array_equal(got, ref), (n, offset)
        for s in (1, 2):                                  # a set in a call of three equals the set alone
            assert np.array_equal(_hist_raw(x[s:s + 1], 1, n, ed), ref[s:s + 1]), (n, s)


@pytest.mark.gpu
def test_histogram_at_the_edges_all_equal_and_one_per_bin():
    from noisediff_amd import _lib as L, noise_stats as ns
    chunk = L.load().nd_histogram_chunk_elements()
    both = np.concatenate([R.kld_edges(), R.default_edges()]).astype(np.float32)
    v = np.concatenate([both, np.nextafter(both, np.float32(np.inf)), np.nextafter(both, np.float32(-np.inf)),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1000, -1000, 1000.5, -1000.5], np.float32)])
    for edges in (R.kld_edges(), R.default_edges()):
        ed = ns.device_edges(edges, DEV)
        ref = R.counts(v, edges)
        assert 0 < ref.sum() < v.size
        for offset in (0, 1):
            assert np.array_equal(_hist_raw(v, 1, v.size, ed, offset)[0], ref)
        # all n values equal: one bin holds exactly n (the worst case of the LDS atomics)
        for n in (1025, 2 * chunk + 3):
            for value in (0.0, np.float32(edges[5])):
                x = np.full(n, value, np.float32)
                ref1 = R.counts(x, edges)
                assert ref1.max() == n and ref1.sum() == n
                assert np.array_equal(_hist_raw(x, 1, n, ed)[0], ref1)
        # a single value in each interior bin
        mid = ((edges[1:-2] + edges[2:-1]) / 2).astype(np.float32)
        ref2 = R.counts(mid, edges)
        assert (ref2[1:-1] == 1).all() and ref2[0] == 0 and ref2[-1] == 0
        assert np.array_equal(_hist_raw(mid, 1, mid.size, ed)[0], ref2)
    special = np.array([np.nan, 1000, -1000, 1000.5, -1001, np.inf, -np.inf, 0.0, -0.0], np.float32)
    got = _hist_raw(special, 1, special.size, ns.device_edges(R.kld_edges(), DEV))[0]
    assert got.sum() == 4 and [int(got[i]) for i in (0, 32, 65)] == [1, 2, 1]


@pytest.mark.gpu
def test_builders_equal_the_reference_goldens(gold):
    from noisediff_amd import noise_stats as ns
    gen, real, unit = (torch.from_numpy(gold[k]).to(DEV) for k in ("generated", "real", "unit"))
    h, centers = ns.get_histogram(unit)
    assert h.dtype == torch.float64 and h.device == DEV and np.array_equal(_np(h), gold["unit.hist"]) and np.array_equal(centers, gold["unit.centers"])
    h, _ = ns.get_histogram(unit, per_sample=True)
    assert np.array_equal(_np(h), gold["unit.hist.per_sample"])
    assert np.array_equal(_np(ns.histogram_counts(unit, R.default_edges())), gold["unit.counts"])
    for name, x in (("generated", gen), ("real", real)):
        h, centers = ns.get_histogram(x, bin_edges=ns.kld_edges())
        assert np.array_equal(_np(h), gold[f"{name}.hist"]) and np.array_equal(centers, gold["kld_centers"])
        c = ns.histogram_counts(x, ns.kld_edges(), per_sample=True)
        assert c.dtype == torch.int64 and np.array_equal(_np(c), gold[f"{name}.counts.per_sample"])
    bound = R.kl_bound(gold["real.hist"], gold["generated.hist"])
    r = ns.noise_kld(gen, real)
    assert all(r[k].dtype == torch.float64 and r[k].device == DEV for k in r) and r["kl_fwd"].shape == ()
    got = np.array([float(r[k]) for k in ("kl_fwd", "kl_inv", "kl_sym")])
    print("noise_kld", got, "golden", gold["kl3"], "bound", bound)
    assert (np.abs(got - gold["kl3"]) <= bound).all()
    assert np.array_equal(_np(r["hist_real"]), gold["real.hist"]) and np.array_equal(_np(r["hist_generated"]), gold["generated.hist"])
    r = ns.noise_kld(gen, real, per_sample=True)
    got = np.stack([_np(r[k]) for k in ("kl_fwd", "kl_inv", "kl_sym")], axis=1)
    assert got.shape == (3, 3)
    for s in range(3):
        b = R.kl_bound(gold["real.hist.per_sample"][s], gold["generated.hist.per_sample"][s])
        assert (np.abs(got[s] - gold["kl3.per_sample"][s]) <= b).all(), s
    # the reference's functions on hists, and on counts with their n
    hr, hg = torch.from_numpy(gold["real.hist"]).to(DEV), torch.from_numpy(gold["generated.hist"]).to(DEV)
    cr, cg = torch.from_numpy(gold["real.counts"]).to(DEV), torch.from_numpy(gold["generated.counts"]).to(DEV)
    n = gold["real"].size
    for fn, i in ((ns.kl_div_forward, 0), (ns.kl_div_inverse, 1), (ns.kl_div_sym, 2)):
        assert abs(float(fn(hr, hg)) - gold["kl3"][i]) <= bound[i]
        assert torch.equal(fn(hr, hg), fn(cr, cg, n, n))                 # hist = counts / n exactly, so both routes see the same p and q
    assert torch.equal(torch.stack(ns.kl_div_3(hr, hg)), torch.stack([ns.kl_div_forward(hr, hg), ns.kl_div_inverse(hr, hg), ns.kl_div_sym(hr, hg)]))


@pytest.mark.gpu
def test_kl_divergence_within_the_a_priori_bound():
    from noisediff_amd import noise_stats as ns
    rs = np.random.RandomState(12)
    for n_bins, edges in ((66, R.kld_edges()), (1000, R.default_edges()), (4096, LAYOUTS[4096]())):
        S, n = 3, 16384
        lo, hi = edges[1], edges[-2]
        a = rs.normal((lo + hi) / 2, (hi - lo) / 6, (S, n)).astype(np.float32)
        b = rs.normal((lo + hi) / 2 + (hi - lo) / 20, (hi - lo) / 5, (S, n)).astype(np.float32)
        pc, qc = np.stack([R.counts(a[s], edges) for s in range(S)]), np.stack([R.counts(b[s], edges) for s in range(S)])
        pd, qd = torch.from_numpy(pc).to(DEV), torch.from_numpy(qc).to(DEV)
        got = _np(torch.stack(ns.kl_div_3(pd, qd, n, n), dim=1))
        one = _np(torch.stack(ns.kl_div_3(pd, qd[:1].contiguous(), n, n), dim=1))
        rep = _np(torch.stack(ns.kl_div_3(pd, qd[:1].expand(S, -1).contiguous(), n, n), dim=1))
        assert one.tobytes() == rep.tobytes()                                  # q_sets 1 == S with the target repeated
        for s in range(S):
            for g, q in ((got[s], qc[s]), (one[s], qc[0])):
                ref, bound = np.array(R.kl_div_3(pc[s] / n, q / n)), R.kl_bound(pc[s] / n, q / n)
                print(f"kl n_bins {n_bins} set {s}: err {np.abs(g - ref)} bound {bound}")
                assert (np.abs(g - ref) <= bound).all() and (ref[:2] > 0).all()
        # identical histograms and disjoint supports: exactly 0.0
        assert (_np(torch.stack(ns.kl_div_3(pd, pd, n, n))) == 0.0).all()
        left, right = pc.copy(), pc.copy()
        left[:, n_bins // 2:] = 0
        right[:, :n_bins // 2] = 0
        z = torch.stack(ns.kl_div_3(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), n, n))
        assert (_np(z) == 0.0).all() and not np.signbit(_np(z)).any()


def _patch_raw(x, want_std=True, want_mean=True):
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    B, Cc, H, W = x.shape
    xd = x.to(DEV).contiguous()
    pad = 7
    std, mean = (torch.full((x.numel() + pad,), float("nan"), device=DEV) for _ in range(2))
    fit = torch.full((B * Cc + 2, 7), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(L.call("nd_patch_std_mean_workspace_bytes", B, Cc, H, W)), dtype=torch.uint8, device=DEV)
    L.call("nd_patch_std_mean_f32", xd.data_ptr(), std.data_ptr() if want_std else None, mean.data_ptr() if want_mean else None, fit.data_ptr(),
           ws.data_ptr(), B, Cc, H, W, _stream(DEV))
    torch.cuda.synchronize()
    assert torch.isnan(std[x.numel():]).all() and torch.isnan(mean[x.numel():]).all() and torch.isnan(fit[B * Cc:]).all()
    return std[:x.numel()].view(x.shape).cpu(), mean[:x.numel()].view(x.shape).cpu(), fit[:B * Cc].cpu().view(B, Cc, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_patch_statistics_and_line_fit(gold, shape):
    from util import derived
    x = torch.from_numpy(gold[f"fit.{_key(shape)}.x"])
    std, mean, fit = _patch_raw(x)
    s64, m64 = R.patch_std_mean(x, torch.float64)
    s32, m32 = R.patch_std_mean(x, torch.float32)
    assert derived(std, s64, s32, "std") and derived(mean, m64, m32, "mean")
    N = shape[2] * shape[3]
    sums = np.stack([np.full(shape[:2], float(N))] + [t.double().reshape(shape[0], shape[1], -1).sum(-1).numpy()
                                                       for t in (mean, std, mean * mean.double(), mean.double() * std.double())], axis=-1)
    np.testing.assert_allclose(fit[..., :5].numpy(), sums, rtol=(N + 8) * 2.0 ** -53, atol=0)           # the fp64 sums of the kernel's own fp32 maps, in any order
    slope64, icpt64 = R.line_fit(m64.numpy(), s64.numpy())
    assert derived(fit[..., 5], slope64, gold[f"fit.{_key(shape)}.lambda"], "slope")
    assert derived(fit[..., 6], icpt64, gold[f"fit.{_key(shape)}.intercept"], "intercept")
    # the NULL-output forms write nothing there and change nothing else
    s2, m2, f2 = _patch_raw(x, want_std=False)
    assert torch.isnan(s2).all() and torch.equal(m2, mean) and torch.equal(f2, fit)
    s3, m3, f3 = _patch_raw(x, want_mean=False)
    assert torch.isnan(m3).all() and torch.equal(s3, std) and torch.equal(f3, fit)


@pytest.mark.gpu
def test_patch_statistics_of_one_pixel_and_the_public_functions(gold):
    from noisediff_amd import noise_stats as ns
    for v in (0.75, -3.0):
        std, mean, fit = _patch_raw(torch.full((1, 1, 1, 1), v))
        assert abs(float(mean) - v / 9) <= 2.0 ** -23 * abs(v) and abs(float(std) - abs(v) * np.sqrt(1 / 9)) <= 2.0 ** -22 * abs(v)
        assert float(fit[0, 0, 0]) == 1.0 and torch.isnan(fit[0, 0, 5]) and torch.isnan(fit[0, 0, 6])           # zero denominator
    shape = (2, 4, 24, 40)
    x = torch.from_numpy(gold[f"fit.{_key(shape)}.x"])
    std, mean, fit = _patch_raw(x)
    s, m = ns.patch_std_mean(x.to(DEV))
    lam, icpt = ns.poisson_lambda_by_patch(x.to(DEV))
    assert torch.equal(s.cpu(), std) and torch.equal(m.cpu(), mean) and lam.shape == (2, 4) and lam.dtype == torch.float64 and lam.device == DEV
    assert torch.equal(lam.cpu(), fit[..., 5]) and torch.equal(icpt.cpu(), fit[..., 6])
    one = ns.poisson_lambda_by_patch(x[1:, 2:3].contiguous().to(DEV))                          # a plane's fit does not depend on the batch it is in
    assert torch.equal(one[0].cpu(), fit[1:, 2:3, 5]) and torch.equal(one[1].cpu(), fit[1:, 2:3, 6])


@pytest.mark.gpu
def test_every_entry_point_repeats_bit_for_bit(gold):
    from noisediff_amd import _lib as L, noise_stats as ns
    chunk = L.load().nd_histogram_chunk_elements()
    x = torch.from_numpy(_values(3, 3 * (2 * chunk + 3), R.kld_edges())).view(3, -1).to(DEV)
    y = torch.from_numpy(_values(4, 3 * (2 * chunk + 3), R.kld_edges())).view(3, -1).to(DEV)
    a, b = ns.histogram_counts(x, ns.kld_edges(), per_sample=True), ns.histogram_counts(x, ns.kld_edges(), per_sample=True)
    assert torch.equal(a, b)
    q = ns.histogram_counts(y, ns.kld_edges(), per_sample=True)
    n = x.shape[1]
    assert torch.equal(torch.stack(ns.kl_div_3(a, q, n, n)), torch.stack(ns.kl_div_3(a, q, n, n)))
    assert torch.equal(torch.stack(ns.kl_div_3(a.double() / n, q.double() / n)), torch.stack(ns.kl_div_3(a.double() / n, q.double() / n)))
    r1, r2 = ns.noise_kld(x, y, per_sample=True), ns.noise_kld(x, y, per_sample=True)
    assert all(torch.equal(r1[k], r2[k]) for k in r1)
    img = torch.from_numpy(gold["fit.1x1x33x257.x"])
    p1, p2 = _patch_raw(img), _patch_raw(img)
    assert all(torch.equal(u, v) for u, v in zip(p1, p2))


@pytest.mark.gpu
def test_a_captured_graph_of_histogram_and_kl_replays_on_rewritten_input():
    from noisediff_amd import _lib as L, noise_stats as ns
    chunk = L.load().nd_histogram_chunk_elements()
    n, edges = chunk + 77, R.kld_edges()
    ed = ns.device_edges(edges, DEV)
    x, y = torch.zeros(2, n, device=DEV), torch.zeros(2, n, device=DEV)

    def run():
        p, q = ns.histogram_counts(x, ed, per_sample=True), ns.histogram_counts(y, ed, per_sample=True)
        return p, q, torch.stack(ns.kl_div_3(p, q, n, n), dim=1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p, q, kl = run()
    for seed in (1, 2):
        xn, yn = _values(seed, 2 * n, edges).reshape(2, n), _values(seed + 10, 2 * n, edges).reshape(2, n) * np.float32(1.2)
        x.copy_(torch.from_numpy(xn))
        y.copy_(torch.from_numpy(yn))
        g.replay()
        torch.cuda.synchronize()
        for s_ in range(2):
            pc, qc = R.counts(xn[s_], edges), R.counts(yn[s_], edges)
            assert np.array_equal(_np(p[s_]), pc) and np.array_equal(_np(q[s_]), qc)
            assert (np.abs(_np(kl[s_]) - np.array(R.kl_div_3(pc / n, qc / n))) <= R.kl_bound(pc / n, qc / n)).all()
        assert torch.equal(kl, run()[2])


@pytest.mark.gpu
def test_a_generation_run_is_scored_end_to_end():
    """A 3-step DDIM generation on NoiseDiffNet(dim=16), then noise_kld of the patches against a seeded Gaussian."""
    from noisediff_amd import GaussianDiffusion, NoiseDiffNet, noise_stats as ns, synth
    from util import state_dict
    dim, c, B = 16, 32, 2
    net = NoiseDiffNet(SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
    net.load_state_dict(state_dict(dim), strict=True)
    net = net.to(DEV).eval()
    gd = GaussianDiffusion(net, image_size=c, timesteps=1000, sampling_timesteps=3, beta_schedule="sigmoid2").to(DEV)
    cond = {k: v.to(DEV) for k, v in synth.make_condition(B, c, seed=1).items()}
    generated = gd.sample(batch_size=B, condition=cond, seed=11)
    assert generated.shape == (B, 4, c, c) and generated.device == DEV
    real = (0.3 * torch.randn(generated.shape, generator=torch.Generator().manual_seed(5))).to(DEV)
    r = ns.noise_kld(generated, real)
    got = np.array([float(r[k]) for k in ("kl_fwd", "kl_inv", "kl_sym")])
    assert np.isfinite(got).all() and (got >= 0).all()
    edges = R.kld_edges()
    hr, hg = R.get_histogram(_np(real), bin_edges=edges)[0], R.get_histogram(_np(generated), bin_edges=edges)[0]
    assert np.array_equal(_np(r["hist_real"]), hr) and np.array_equal(_np(r["hist_generated"]), hg)
    ref, bound = np.array(R.kl_div_3(hr, hg)), R.kl_bound(hr, hg)
    print("end to end", got, ref, bound)
    assert (np.abs(got - ref) <= bound).all()


@pytest.mark.gpu
def test_kl_entry_points_write_their_rows_only_and_mask_nan_and_inf():
    """Both C entry points on an ``out`` that is NaN-filled and two rows too long; the hist form with a NaN, an inf and a -inf among the bins:
    those bins are dropped, as kl_div_forward's first mask drops them."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    rs = np.random.RandomState(21)
    S, n_bins, n = 3, 66, 4096
    pc, qc = rs.multinomial(n, np.full(n_bins, 1 / n_bins), S).astype(np.int64), rs.multinomial(n, np.full(n_bins, 1 / n_bins), S).astype(np.int64)
    pc[:, :3] = 0                                                 # some bins outside the overlap
    ph, qh = pc / n, qc / n
    ph[0, 5], ph[1, 7], qh[2, 9], qh[0, 11] = np.nan, np.inf, -np.inf, np.nan
    for q_sets in (S, 1):
        outs = []
        for name, p, q, extra in (("nd_kl_div_f64", pc, qc, (n, n)), ("nd_kl_div_hist_f64", ph, qh, ())):
            pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(np.ascontiguousarray(q[:q_sets])).to(DEV)
            out = torch.full((S + 2, 3), float("nan"), dtype=torch.float64, device=DEV)
            L.call(name, pd.data_ptr(), qd.data_ptr(), *extra, n_bins, S, q_sets, out.data_ptr(), _stream(DEV))
            torch.cuda.synchronize()
            got = _np(out)
            assert np.isnan(got[S:]).all(), (name, "wrote past S rows")
            for s in range(S):
                pr, qr = (p[s] / n, q[s if q_sets == S else 0] / n) if extra else (p[s], q[s if q_sets == S else 0])
                ref, bound = np.array(R.kl_div_3(pr, qr)), R.kl_bound(pr, qr)
                assert np.isfinite(got[s]).all() and (np.abs(got[s] - ref) <= bound).all(), (name, q_sets, s, got[s], ref, bound)
            outs.append(got[:S])
        assert not np.array_equal(outs[0], outs[1])              # the masked bins changed the values
