"""noisediff_amd.physics_noise: the physics-based noise model of ELD / PMN (Poisson shot noise, Gaussian or Tukey-lambda read noise, row noise,
quantisation noise and a bias) drawn on windows of resident uint16 frames by one HIP launch (csrc/physics_noise.hip).

CPU: the Tukey-lambda quantile's identities and its agreement with scipy; the moments of the numpy restatement (tests/physics_noise_ref.py);
every refusal of the entry and of ``check``; the struct layout in the header, the numpy dtype and the ctypes binding; ``CameraNoiseModel.draw``.
GPU: bit for bit from explicit variates at all three vector widths; the drawn variates against the restatement's; the Poisson-Gaussian launch
as a special case; row variates shared by windows of one frame; an invalid table row; graph replay; the public path.  Outputs are pre-filled
with NaN, one sample longer than written, and the tail is checked.

The explicit-variate and the row tests take their frames larger than the windows (160 x 200 and 96 x 160 codes) so that a window origin
x0 = 3 and two overlapping windows fit."""
import ctypes as C
import json
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import physics_noise_ref as P
import raw_ref as R
from noisediff_amd import synth
from test_raw import PG_CASES, _pg_frames

DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
WB = 15871.0
ISOS = (100, 1600, 3200, 25600)
RATIOS = {100: 100, 1600: 250, 3200: 300, 25600: 300}
KEY = dict(seed=(7 << 32) + 99, first_sample=5, draw=3)
VARIATES = ("counts", "reads", "rows", "quants")
OUTPUTS = ("noisy", "clean", "noise") + VARIATES


def table():
    with open(os.path.join(REPO, "tests", "golden", "physics_params.json")) as f:
        return {int(k): v for k, v in json.load(f)["rows"].items()}


def model_params(iso, kind, lam=None, bias=None):
    """One sample's parameters straight from a fixture row (no jitter): K = Kmax, s_read = sigGs or sigTL, s_row = sigR."""
    r = table()[iso]
    return dict(K=r["Kmax"], s_read=r["sigTL"] if kind else r["sigGs"], read_kind=kind, lam=r["lam"] if lam is None else lam, s_row=r["sigR"], q=r["q"],
                bias=r["bias"] if bias is None else bias)


def ref_params(p):
    """What the restatement takes: the device row's K, s_read, s_row, qstep = q wb, bias."""
    return dict(K=p["K"], s_read=p["s_read"], s_row=p["s_row"], qstep=p["q"] * WB, bias=p["bias"])


def batch_params(ps):
    return {k: [p[k] for p in ps] for k in ps[0]}


# --------------------------------------------------------------------------- CPU 1: the quantile

def _grid():
    tails = np.array([10.0 ** -j for j in range(3, 10)])
    return np.sort(np.concatenate([tails, np.array([k / 1024 for k in range(1, 1024)]), 1.0 - tails]))


def _quantile_tolerance(u, lam):
    """log, log1p and expm1 are good to about an ulp and four more roundings follow; the difference of the two expm1 is taken between numbers no
    larger than max(1, e^(-lam log)), and the division by lam turns an error relative to lam log back into one relative to log: 64 ulp of
    max(1, |log u|, |log(1-u)|) e^max(0, -lam log) is generous and still 1e-14 of the value."""
    a = np.maximum(np.abs(np.log(u)), np.abs(np.log1p(-u)))
    return 64 * 2.0 ** -53 * np.maximum(1.0, a) * np.exp(np.maximum(0.0, -lam) * a)


def test_tukey_lambda_quantile_identities():
    u = _grid()
    dyadic = np.array([k / 1024 for k in range(1, 1024)])                  # 1 - u is exact
    lams = [table()[i]["lam"] for i in ISOS] + [1.0, 2.0, -0.3, 0.0026, 0.0, 1e-9]
    for lam in lams:
        q, qm = P.tukey_quantile(dyadic, lam), P.tukey_quantile(1.0 - dyadic, lam)
        tol = _quantile_tolerance(dyadic, lam)
        assert (np.abs(q + qm) <= 2 * tol).all(), lam                       # Q(1 - u) = -Q(u)
        assert abs(float(P.tukey_quantile(0.5, lam))) <= 64 * 2.0 ** -53, lam
        assert (np.diff(P.tukey_quantile(u, lam)) > 0).all(), lam           # a quantile function increases
    assert (np.abs(P.tukey_quantile(u, 1.0) - (2.0 * u - 1.0)) <= _quantile_tolerance(u, 1.0)).all()
    assert (np.abs(P.tukey_quantile(u, 2.0) - (u - 0.5)) <= _quantile_tolerance(u, 2.0)).all()
    logit = np.log(u) - np.log1p(-u)
    assert np.array_equal(P.tukey_quantile(u, 0.0), logit)
    # Q_lam - logit = lam (log(u)^2 - log(1-u)^2) / 2 + O(lam^2): 2.4e-8 at lam = 1e-9 on the dyadic grid (|log| <= 6.94), a true 2.1e-7 at u = 1e-9
    assert (np.abs(P.tukey_quantile(dyadic, 1e-9) - (np.log(dyadic) - np.log1p(-dyadic))) < 1e-7).all()
    from noisediff_amd.physics_noise import tukey_lambda_quantile             # the package's own numpy form
    for lam in lams:
        assert np.array_equal(tukey_lambda_quantile(u, lam), P.tukey_quantile(u, lam)), lam


def test_tukey_lambda_quantile_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    u = _grid()
    u = u[u != 0.5]
    for iso in ISOS:
        lam = table()[iso]["lam"]
        want = stats.tukeylambda.ppf(u, lam)
        rel = np.abs(P.tukey_quantile(u, lam) - want) / np.abs(want)
        print(f"lam {lam}: max relative difference to scipy {rel.max():.3e}")
        assert (rel <= 1e-10).all(), (lam, rel.max())


# --------------------------------------------------------------------------- CPU 2: moments of the restatement

def _z(x, mean, var):
    """z-scores of the sample's mean and variance, the variance's standard error from the sample's own fourth moment."""
    x = np.asarray(x, np.float64)
    n, m = x.size, x.mean()
    d = x - m
    v, m4 = (d ** 2).mean(), (d ** 4).mean()
    return (m - mean) / math.sqrt(v / n), (v - var) / math.sqrt((m4 - v * v) / n)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("iso", [100, 1600, 25600])
@pytest.mark.parametrize("level", [40.0, 3000.0])
def test_moments_of_the_restatement(level, iso, kind):
    """A constant level: mean of t - y against bias and variance against K y + s_read^2 Var_unit + qstep^2 / 12, both within 4 standard errors.
    y = level / ratio is the level at the short exposure; s_row = 0."""
    n, ratio = 4 * 64 * 64, 100
    p = dict(model_params(iso, kind, bias=0.25), s_row=0.0)
    c0, lam_p = P.rate(np.full(n, 512.0 + level, np.float32), ratio, p["K"])
    y = float(np.float64(c0[0] / np.float32(ratio)))
    counts = R.poisson(lam_p, KEY["seed"], KEY["first_sample"], KEY["draw"])
    reads = P.read64(kind, p["lam"], KEY["seed"], KEY["first_sample"], KEY["draw"], n).astype(np.float32)
    quants = P.quant(KEY["seed"], KEY["first_sample"], KEY["draw"], n)
    t = P.signal(counts, reads, np.zeros(()), quants, ref_params(p)).reshape(-1)
    unit = P.tukey_variance(p["lam"]) if kind else 1.0
    var = p["K"] * y + p["s_read"] ** 2 * unit + (p["q"] * WB) ** 2 / 12
    zm, zv = _z(t - y, p["bias"], var)
    print(f"level {level} iso {iso} kind {kind}: z(mean) {zm:+.2f} z(var) {zv:+.2f} min t {t.min():.1f} max t {t.max():.1f}")
    assert abs(zm) <= 4 and abs(zv) <= 4
    assert t.min() > -512 and t.max() < WB                               # the sensor clip is idle


def test_tukey_variance_and_row_variates():
    assert abs(P.tukey_variance(0.149) - 2.06) < 0.01 and abs(P.tukey_variance(-0.091) - 4.61) < 0.01
    g = P.row64(KEY["seed"], 5, KEY["draw"], np.arange(256)).astype(np.float32)
    assert g.shape == (4, 256) and np.unique(g).size == g.size
    zm, zv = _z(g, 0.0, 1.0)
    print(f"row variates: z(mean) {zm:+.2f} z(var) {zv:+.2f}")
    assert abs(zm) <= 4 and abs(zv) <= 4


# --------------------------------------------------------------------------- CPU 3: refusals and layout

def test_the_entry_refuses_bad_arguments_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    f, odd, odd4 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # never dereferenced: every call below fails its checks first

    def ph(frames=f, N=2, H2=64, W2=96, table=f, rng=None, draw=0, ins=(None,) * 4, outs=(None,) * 4, black=512.0, white=16383.0, flags=1, noisy=f,
           clean=f, noise=None, B=2, h=16, w=24):
        return lib.nd_raw_physics_noise_f32(frames, N, H2, W2, table, rng, 1, 0, draw, *ins, *outs, black, white, flags, noisy, clean, noise, B, h, w, None)

    # what nd_raw_poisson_gaussian_f32 refuses
    assert ph(frames=None) == -1 and ph(table=None) == -1 and ph(noisy=None) == -1 and ph(clean=None) == -1 and ph(draw=-1) == -1
    assert ph(N=0) == -1 and ph(B=0) == -1 and ph(B=65536) == -1 and ph(h=0) == -1 and ph(w=0) == -1 and ph(H2=0) == -1
    assert ph(black=-1.0) == -1 and ph(white=512.0) == -1 and ph(white=70000.0) == -1
    assert ph(H2=62, h=32) == -1 and ph(W2=95) == -1 and ph(H2=63) == -1 and ph(w=49) == -1 and ph(h=33) == -1
    assert ph(frames=odd) == -1 and ph(table=odd4) == -1 and ph(rng=odd4) == -1 and ph(noisy=odd) == -1 and ph(clean=odd) == -1 and ph(noise=odd) == -1
    for i in range(4):
        one = tuple(odd if j == i else None for j in range(4))
        assert ph(ins=one) == -1 and ph(outs=one) == -1, i
    # the element counter, and the flags
    assert ph(H2=1 << 17, W2=1 << 17, h=1 << 15, w=1 << 15) == -1 and b"32-bit" in lib.nd_last_error()
    assert ph(flags=2) == -1 and b"flags" in lib.nd_last_error() and ph(flags=3) == -1 and ph(flags=-1) == -1


def test_check_refuses_bad_parameters_on_the_host():
    from noisediff_amd import _lib as L, physics_noise as pn
    with pytest.raises(ValueError):
        pn.PhysicsNoiseBatchBuilder(crop=0)
    with pytest.raises(ValueError):
        pn.PhysicsNoiseBatchBuilder(crop=16, black=600, white=512)
    b = pn.PhysicsNoiseBatchBuilder(crop=16)
    shape = (2, 64, 96)
    prm = batch_params([model_params(100, 0), model_params(25600, 1, bias=-0.5)])
    ok = dict(frame=[0, 1], xy=[(0, 0), (32, 16)], ratio=[100, 300], params=prm, flip=[1, 0])
    host = b.check(2, shape, **ok, seed=(5 << 32) + 7, first_sample=3, draw=2)
    rows = host[32:].view(pn.ROW)
    assert host[:32].view(np.int64)[:3].tolist() == [(5 << 32) + 7, 3, 2]
    assert rows["x0"].tolist() == [0, 32] and rows["flip"].tolist() == [1, 0] and rows["read_kind"].tolist() == [0, 1] and rows["row_stream"].tolist() == [3, 4]
    assert rows["K"].tolist() == prm["K"] and rows["s_read"].tolist() == prm["s_read"] and rows["lam"].tolist() == prm["lam"]
    assert rows["qstep"].tolist() == [q * WB for q in prm["q"]] and rows["bias"].tolist() == [0.0, -0.5] and rows["ratio"].tolist() == [100.0, 300.0]
    assert b.check(2, shape, **ok, row_stream=9)[32:].view(pn.ROW)["row_stream"].tolist() == [9, 9]
    assert b.check(2, shape, **{**ok, "params": {**prm, "read_kind": ["gaussian", "tukey"]}})[32:].view(pn.ROW)["read_kind"].tolist() == [0, 1]
    b.check(2, shape, **{**ok, "xy": [(3, 5), (31, 15)]})                                      # any integer origin inside the frame
    b.check(2, shape, **{**ok, "params": {**prm, "lam": [-0.6, 0.0], "s_read": 0.0, "s_row": 0.0, "q": 0.0}})     # infinite variance, zero scales: not refused
    # what the window builders refuse
    for change in ({"xy": [(0, 0), (33, 16)]}, {"xy": [(0, 17), (0, 0)]}, {"xy": [(-1, 0), (0, 0)]}, {"frame": [0, 2]}, {"frame": [-1, 0]},
                   {"ratio": [0, 250]}, {"ratio": [100, NAN]}, {"ratio": [-100, 300]}, {"xy": [(0, 0)]}, {"draw": -1}):
        with pytest.raises(ValueError):
            b.check(2, shape, **{**ok, **change})
    for bad_shape in ((2, 63, 96), (2, 64, 95), (2, 30, 96), (64,)):
        with pytest.raises(ValueError):
            b.check(2, bad_shape, **ok)
    # the model's parameters
    for change in ({"K": [0.0, 24.5]}, {"K": [0.1, -1.0]}, {"K": [NAN, 1.0]}, {"s_read": [-0.1, 1.0]}, {"s_read": [math.inf, 1.0]}, {"s_row": -1.0},
                   {"s_row": [NAN, 0.0]}, {"q": -1e-5}, {"q": math.inf}, {"lam": [NAN, 0.0]}, {"lam": math.inf}, {"bias": NAN}, {"read_kind": 2},
                   {"read_kind": "cauchy"}, {"read_kind": [0, 1, 0]}):
        with pytest.raises(ValueError):
            b.check(2, shape, **{**ok, "params": {**prm, **change}})
    with pytest.raises(ValueError):
        b.check(2, shape, **{**ok, "params": {k: v for k, v in prm.items() if k != "lam"}})
    b.check(2, shape, **{**ok, "ratio": 100, "params": {**prm, "K": [1e-5, 24.5]}})          # 15871 / (100 * 1e-5) = 1.6e7 < 2^24: counts stay exact
    with pytest.raises(ValueError, match="2\\*\\*24"):
        b.check(2, shape, **{**ok, "ratio": 100, "params": {**prm, "K": [9e-6, 24.5]}})      # 15871 / (100 * 9e-6) = 1.76e7 >= 2^24
    with pytest.raises(L.HipError):
        b(torch.zeros(shape, dtype=torch.int16), **ok)
    with pytest.raises(L.HipError):
        pn.physics_frames(torch.zeros(shape, dtype=torch.int16), [0, 1], [100, 300], prm)
    with pytest.raises(ValueError):
        pn.physics_frames(torch.zeros(shape, dtype=torch.int16), [0, 2], [100, 300], prm)
    with pytest.raises(ValueError):
        pn.physics_frames(torch.zeros(shape, dtype=torch.int16), [0, 1], [100, 300], {**prm, "K": 0.0})


def _header_struct(name):
    """[(field, C type, count)] of a struct of include/noisediff_hip.h, comments removed."""
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    return fields


def test_the_struct_layout_agrees_in_the_header_the_dtype_and_the_binding():
    from noisediff_amd import _lib as L, physics_noise as pn
    size = {"int32_t": 4, "uint32_t": 4, "double": 8}
    np_kind = {"int32_t": "<i4", "uint32_t": "<u4", "double": "<f8"}
    c_kind = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}
    fields = _header_struct("nd_physics_sample")
    assert [f[0] for f in fields] == ["frame", "x0", "y0", "flip", "read_kind", "row_stream", "reserved", "ratio", "K", "s_read", "lam", "s_row", "qstep", "bias"]
    assert list(pn.ROW.names) == [f[0] for f in fields] == [f[0] for f in L.PhysicsSample._fields_]
    offset = 0
    for (name, ctype, count), (bname, btype) in zip(fields, L.PhysicsSample._fields_):
        offset = -(-offset // size[ctype]) * size[ctype]                  # natural alignment
        sub, at = pn.ROW.fields[name][:2]
        assert at == offset == getattr(L.PhysicsSample, name).offset, name
        assert sub.base == np.dtype(np_kind[ctype]) and int(np.prod(sub.shape or (1,))) == count, name
        assert btype is (c_kind[ctype] if count == 1 else c_kind[ctype] * count) or (count > 1 and C.sizeof(btype) == count * size[ctype]), name
        offset += size[ctype] * count
    assert offset == 88 == pn.ROW.itemsize == C.sizeof(L.PhysicsSample) and offset % 8 == 0
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    assert int(re.search(r"#define ND_PHYS_CLIP01 (\d+)", header).group(1)) == L.PHYS_CLIP01 == 1
    proto = re.search(r"int nd_raw_physics_noise_f32\((.*?)\);", header, re.S).group(1)
    kinds = []
    for arg in proto.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg else {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
                                                    "float": C.c_float}[arg.rsplit(" ", 1)[0]])
    res, args = L.SIGNATURES["nd_raw_physics_noise_f32"]
    assert res is C.c_int and args == kinds and len(args) == 27


# --------------------------------------------------------------------------- CPU 4: the camera model

def test_camera_noise_model_draws_per_sample_parameters():
    from noisediff_amd.physics_noise import CameraNoiseModel
    tab = table()
    m = CameraNoiseModel(tab)
    isos = [100, 1600, 3200, 25600, 100, 25600]
    g = m.draw(isos, seed=11, first_sample=40)
    t = m.draw(isos, seed=11, first_sample=40, read="tukey")
    assert set(g) == {"K", "s_read", "read_kind", "lam", "s_row", "q", "bias"} and all(len(v) == 6 for v in g.values())
    for b, iso in enumerate(isos):
        r = tab[iso]
        alone = m.draw(iso, seed=11, first_sample=40 + b)                  # a sample alone equals the same sample in a batch
        assert all(alone[k][0] == g[k][b] for k in g), (b, iso)
        assert abs(g["K"][b] / r["Kmax"] - 1) <= 0.01 and g["K"][b] != r["Kmax"]
        assert g["lam"][b] == r["lam"] and g["q"][b] == r["q"] and g["read_kind"][b] == 0 and t["read_kind"][b] == 1
        assert abs(g["s_read"][b] - r["sigGs"]) <= 6 * r["sigGssig"] and abs(t["s_read"][b] - r["sigTL"]) <= 6 * r["sigTLsig"]
        assert abs(g["s_row"][b] - r["sigR"]) <= 6 * r["sigRsig"] and abs(g["bias"][b] - r["bias"]) <= 6 * r["biassig"]
        assert t["K"][b] == g["K"][b] and t["s_row"][b] == g["s_row"][b] and t["bias"][b] == g["bias"][b]
    assert g["K"][0] != g["K"][4] and m.draw(isos, seed=12, first_sample=40)["K"][0] != g["K"][0]
    wide = CameraNoiseModel({7: {**tab[100], "sigGs": 0.001, "sigGssig": 1.0, "sigTL": 0.001, "sigTLsig": 1.0, "sigR": 0.001, "sigRsig": 1.0}})
    for read in ("gaussian", "tukey"):
        d = wide.draw([7] * 64, seed=3, read=read)
        assert (d["s_read"] >= 0).all() and (d["s_row"] >= 0).all() and (d["s_read"] == 0).any() and (d["s_row"] == 0).any()      # the floors hold
        assert (d["s_read"] > 0).any()
    with pytest.raises(KeyError):
        m.draw(200, seed=1)
    with pytest.raises(KeyError):
        m.draw([100, 200], seed=1)
    with pytest.raises(ValueError):
        m.draw(100, seed=1, read="cauchy")
    with pytest.raises(ValueError):
        CameraNoiseModel({100: {"Kmax": 1.0}})
    import noisediff_amd
    from noisediff_amd import physics_noise
    for name in ("PhysicsNoiseBatchBuilder", "CameraNoiseModel", "physics_frames", "tukey_lambda_quantile"):
        assert getattr(noisediff_amd, name) is getattr(physics_noise, name) and name in noisediff_amd.__all__, name


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


def _dev_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).to(DEV)


def _rows(specs, first_sample):
    """The device table from [(frame, x0, y0, flip, ratio, params[, row_stream])]: what PhysicsNoiseBatchBuilder.check writes, for h != w."""
    from noisediff_amd import physics_noise as pn
    rows = np.zeros(len(specs), pn.ROW)
    for b, s in enumerate(specs):
        p = s[5]
        rows[b]["frame"], rows[b]["x0"], rows[b]["y0"], rows[b]["flip"], rows[b]["ratio"] = s[:5]
        rows[b]["read_kind"], rows[b]["row_stream"] = p["read_kind"], (s[6] if len(s) > 6 else first_sample + b) & 0xFFFFFFFF
        for k in ("K", "s_read", "lam", "s_row", "bias"):
            rows[b][k] = p[k]
        rows[b]["qstep"] = p["q"] * WB
    return rows


def _run(fd, rows, h, w, flags=1, key=KEY, given=None, rng=None, offset=0, want=OUTPUTS):
    """nd_raw_physics_noise_f32 into NaN-filled buffers one sample longer than written, each ``offset`` bytes into its allocation; {name: numpy [B]}."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    B = len(rows)
    tab = torch.from_numpy(rows.view(np.uint8).copy()).to(DEV)
    shape = lambda k: (B + 1, 4, h) if k == "rows" else (B + 1, 4, h, w)          # noqa: E731
    bufs = {}
    for k in want:
        n = int(np.prod(shape(k)))
        flat = torch.full((n + offset // 4,), NAN, device=DEV)
        bufs[k] = flat[offset // 4:].view(shape(k))
        assert bufs[k].data_ptr() % 16 == offset
    given = given or {}
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    N, H2, W2 = fd.shape
    L.call("nd_raw_physics_noise_f32", fd.data_ptr(), N, H2, W2, tab.data_ptr(), ptr(rng), key["seed"], key["first_sample"], key["draw"],
           *[ptr(given.get(k)) for k in VARIATES], *[ptr(bufs.get(k)) for k in VARIATES], 512.0, 16383.0, flags, bufs["noisy"].data_ptr(),
           bufs["clean"].data_ptr(), ptr(bufs.get("noise")), B, h, w, _stream(DEV))
    torch.cuda.synchronize()
    res = {k: _np(t) for k, t in bufs.items()}
    assert all(np.isnan(a[B:]).all() for a in res.values()), "the kernel wrote past its output"
    return {k: a[:B] for k, a in res.items()}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("w,offset", [(80, 0), (78, 8), (77, 4)])
def test_from_explicit_variates_bit_for_bit(w, offset):
    """All four variate arrays given: noisy, clean_out and noise_out equal the restatement with zero difference, with and without ND_PHYS_CLIP01;
    w = 80 / 78 / 77 with the outputs 0 / 8 / 4 bytes off a 16-byte boundary take 4 / 2 / 1 columns per thread."""
    frames = _pg_frames(4, 160, 200, seed=21)
    fd = _dev_frames(frames)
    h = 48
    ps = [model_params(100, 0, bias=0.25), model_params(1600, 1, bias=-0.5), model_params(25600, 1, lam=0.0)]
    specs = [(1, 3, 2, 0, 100, ps[0]), (0, 10, 7, 1, 250, ps[1]), (3, 0, 32, 0, 300, ps[2])]
    B = len(specs)
    counts = synth.uniform(21, "physics.t.counts", (B, 4, h, w), 0.0, 1.2).numpy().astype(np.float64)
    for b, s in enumerate(specs):
        counts[b] *= WB / (s[4] * s[5]["K"])                          # up to 1.2 times the count that reaches white
    given = dict(counts=np.floor(counts).astype(np.float32), reads=synth.normal(21, "physics.t.reads", (B, 4, h, w)).numpy(),
                 rows=synth.normal(21, "physics.t.rows", (B, 4, h)).numpy(), quants=synth.uniform(21, "physics.t.quants", (B, 4, h, w), -0.5, 0.5).numpy())
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in given.items()}
    for flags in (1, 0):
        got = _run(fd, _rows(specs, 0), h, w, flags=flags, key=dict(seed=1, first_sample=0, draw=0), given=dev, offset=offset)
        for k in VARIATES:
            assert np.array_equal(got[k], given[k]), k
        for b, (frame, x0, y0, flip, ratio, p) in enumerate(specs):
            x = R.window(R.codes(frames[frame]), x0, y0, h, w, flip)
            want = P.noisy(*[given[k][b] for k in VARIATES], ref_params(p), ratio, clip01=bool(flags))
            clean = P.clean(x)
            assert np.array_equal(got["noisy"][b], want), f"flags {flags} sample {b}: {int((got['noisy'][b] != want).sum())} differ"
            assert np.array_equal(got["clean"][b], clean) and np.array_equal(got["noise"][b], P.noise(want, clean))
            inside = float(((want > 0) & (want < 1)).mean())
            assert inside > 0.3, (b, inside)
            if not flags:
                assert (want < 0).any() and (want > 1).any()           # the two forms do differ


@pytest.fixture(scope="module")
def drawn_frames():
    frames = _pg_frames(4, 96, 160, seed=23)
    frames[:, 0, :128] = 512                                  # the first 64 elements of every sample sit at the black level: rate 0
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 0], ids=["tukey", "gaussian"])
def test_drawn(drawn_frames, kind):
    frames, fd = drawn_frames, _dev_frames(drawn_frames)
    h, w = 48, 80
    n_el = 4 * h * w
    ps = [model_params(iso, kind) for iso in ISOS]
    specs = [(b, 0, 0, 0, RATIOS[iso], ps[b]) for b, iso in enumerate(ISOS)]
    rows = _rows(specs, KEY["first_sample"])
    got = _run(fd, rows, h, w)
    differ = unequal = 0
    worst = 0.0
    for b, (frame, _, _, _, ratio, p) in enumerate(specs):
        sample = KEY["first_sample"] + b
        x = R.codes(frames[frame])[:, :h, :w]
        c0, lam_p = P.rate(x, ratio, p["K"])
        assert (lam_p.reshape(-1)[:64] == 0).all()
        want_n = R.poisson(lam_p, KEY["seed"], sample, KEY["draw"])
        got_n = got["counts"][b].reshape(-1)
        differ += int((got_n != want_n).sum())
        assert (got_n[:64] == 0).all()
        r64 = P.read64(kind, p["lam"], KEY["seed"], sample, KEY["draw"], n_el)
        got_r, want_r = got["reads"][b].reshape(-1), r64.astype(np.float32)
        if kind == 0:                                               # the Poisson-Gaussian test's bound: the same fp32 unless fp64 sits on a tie
            assert (np.abs(got_r.astype(np.float64) - want_r.astype(np.float64)) <= 8 * 2.0 ** -53 * np.maximum(1.0, np.abs(r64))).all()
        else:                                                       # equal or adjacent: an fp64 error below half an fp32 ulp moves the rounding one step
            ulp = np.spacing(np.abs(want_r)).astype(np.float64)
            worst = max(worst, float((np.abs(got_r.astype(np.float64) - r64) / ulp).max()))
            unequal += int((got_r != want_r).sum())
            lo, hi = np.nextafter(want_r, np.float32(-np.inf)), np.nextafter(want_r, np.float32(np.inf))
            assert ((got_r == want_r) | (got_r == lo) | (got_r == hi)).all()
        g64 = P.row64(KEY["seed"], sample, KEY["draw"], P.source_rows(0, h, 0))
        assert (np.abs(got["rows"][b].astype(np.float64) - g64.astype(np.float32).astype(np.float64)) <= 8 * 2.0 ** -53 * np.maximum(1.0, np.abs(g64))).all()
        assert np.array_equal(got["quants"][b].reshape(-1), P.quant(KEY["seed"], sample, KEY["draw"], n_el))
        want = P.noisy(*[got[k][b] for k in VARIATES], ref_params(p), ratio)                 # the restatement fed the four returned arrays
        clean = P.clean(x)
        assert np.array_equal(got["noisy"][b], want) and np.array_equal(got["clean"][b], clean) and np.array_equal(got["noise"][b], P.noise(want, clean))
        assert float(((want > 0) & (want < 1)).mean()) > 0.05
    print(f"kind {kind}: {differ} of {4 * n_el} counts differ from the restatement")
    if kind:
        print(f"tukey variate: max |device fp32 - restated fp64| = {worst:.4f} fp32 ulp (0.5 is exact rounding); {unequal} of {4 * n_el} fp32 differ")
    assert differ <= 1
    assert _same(_run(fd, rows, h, w), got)                                                  # a repeated call
    alone = _run(fd, _rows([specs[2] + (KEY["first_sample"] + 2,)], 0), h, w, key={**KEY, "first_sample": KEY["first_sample"] + 2})
    assert all(np.array_equal(alone[k][0], got[k][2]) for k in OUTPUTS)                      # a sample alone, the same row_stream
    for other in (dict(seed=KEY["seed"] + 1), dict(seed=KEY["seed"] + (1 << 32)), dict(draw=4), dict(first_sample=6)):
        key = {**KEY, **other}
        o = _run(fd, _rows(specs, key["first_sample"]), h, w, key=key, want=("noisy", "clean") + VARIATES)
        assert not any(np.array_equal(o[k], got[k]) for k in VARIATES), other
        rng = torch.tensor([key["seed"] - (1 << 64) if key["seed"] >= 1 << 63 else key["seed"], key["first_sample"], key["draw"], 0], dtype=torch.int64,
                           device=DEV)
        via = _run(fd, _rows(specs, key["first_sample"]), h, w, key=dict(seed=1, first_sample=0, draw=0), rng=rng, want=("noisy", "clean") + VARIATES)
        assert _same(via, o), other                                                          # the device block overrides the arguments


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,k", PG_CASES)
def test_the_poisson_gaussian_launch_is_a_special_case(drawn_frames, ratio, k):
    """read_kind 0, s_row = qstep = bias = 0 and ND_PHYS_CLIP01: the values of nd_raw_poisson_gaussian_f32 for the same key, k = K, sd = s_read."""
    from noisediff_amd import _lib as L, raw
    from noisediff_amd._host import _stream
    fd = _dev_frames(drawn_frames)
    h, w, sd = 48, 80, 2.0
    p = dict(K=k, s_read=sd, read_kind=0, lam=0.0, s_row=0.0, q=0.0, bias=0.0)
    got = _run(fd, _rows([(b, 0, 0, b % 2, ratio, p) for b in range(4)], KEY["first_sample"]), h, w, want=("noisy", "clean", "counts", "reads"))
    rows = np.zeros(4, raw.ROW)
    rows["frame"], rows["flip"], rows["k"], rows["sd"], rows["ratio64"], rows["ratio"] = np.arange(4), np.arange(4) % 2, k, sd, ratio, ratio
    tab = torch.from_numpy(rows.view(np.uint8)).to(DEV)
    bufs = [torch.full((4, 4, h, w), NAN, device=DEV) for _ in range(4)]
    L.call("nd_raw_poisson_gaussian_f32", fd.data_ptr(), 4, 96, 160, tab.data_ptr(), None, KEY["seed"], KEY["first_sample"], KEY["draw"], None, None,
           bufs[2].data_ptr(), bufs[3].data_ptr(), 512.0, 16383.0, bufs[0].data_ptr(), bufs[1].data_ptr(), 4, h, w, _stream(DEV))
    torch.cuda.synchronize()
    for name, t in zip(("noisy", "clean", "counts", "reads"), bufs):
        assert np.array_equal(got[name], _np(t)), name
    assert float(((got["noisy"] > 0) & (got["noisy"] < 1)).mean()) > 0.05 and (got["noisy"] == 0).any()


@pytest.mark.gpu
def test_windows_of_one_frame_share_their_row_variates(drawn_frames):
    fd = _dev_frames(drawn_frames)
    p = model_params(1600, 1)
    h, w, stream = 32, 64, 77
    a, b = (1, 0, 4, 0, 250, p, stream), (1, 16, 12, 1, 250, p, stream)
    got = _run(fd, _rows([a, b], 0), h, w, want=("noisy", "clean", "rows"))["rows"]
    ya, yb = P.source_rows(4, h, 0), P.source_rows(12, h, 1)
    shared = np.intersect1d(ya, yb)
    assert shared.size == 24
    ia, ib = [int(np.nonzero(ya == Y)[0][0]) for Y in shared], [int(np.nonzero(yb == Y)[0][0]) for Y in shared]
    assert np.array_equal(got[0][:, ia], got[1][:, ib]) and not np.array_equal(got[0], got[1])
    whole = _run(fd, _rows([(1, 0, 0, 0, 250, p, stream)], 0), 48, 80, want=("noisy", "clean", "rows"))["rows"][0]
    assert np.array_equal(got[0], whole[:, ya]) and np.array_equal(got[1], whole[:, yb])
    assert np.unique(whole).size == whole.size
    other = _run(fd, _rows([a[:6] + (78,)], 0), h, w, want=("noisy", "clean", "rows"))["rows"][0]
    assert not (other == got[0]).any()


@pytest.mark.gpu
def test_a_table_row_outside_the_frame_gives_nan_for_that_sample_only(drawn_frames):
    fd = _dev_frames(drawn_frames)
    p = model_params(3200, 1)
    h, w = 32, 64
    good = [(0, 3, 5, 0, 300, p), (1, 16, 16, 1, 300, p), (2, 0, 0, 0, 300, p)]
    ref = _run(fd, _rows(good, 5), h, w)
    for bad in ((1, 17, 16, 1, 300, p), (1, 16, 17, 1, 300, p), (4, 16, 16, 1, 300, p), (-1, 0, 0, 0, 300, p), (1, -1, 0, 0, 300, p), (1, 0, -1, 0, 300, p)):
        got = _run(fd, _rows([good[0], bad, good[2]], 5), h, w)
        for k in OUTPUTS:
            assert np.isnan(got[k][1]).all(), (bad[:4], k)
            assert np.array_equal(got[k][0], ref[k][0]) and np.array_equal(got[k][2], ref[k][2]), (bad[:4], k)


@pytest.mark.gpu
def test_a_captured_launch_replays_with_a_rewritten_table_and_key():
    """One launch in the graph, a single stream; the device block (key and table) is rewritten between replays."""
    from noisediff_amd import physics_noise as pn
    frames = np.floor(synth.uniform(9, "physics.t.graph", (2, 136, 208), 300.0, 4000.0).numpy()).astype(np.uint16)
    fd = _dev_frames(frames)
    shape, c = tuple(fd.shape), 32
    b = pn.PhysicsNoiseBatchBuilder(c)
    p1 = dict(frame=[0, 1], xy=[(0, 0), (72, 36)], ratio=[100, 300], params=batch_params([model_params(100, 0), model_params(25600, 1)]), flip=[1, 0],
              seed=1, first_sample=0, draw=0)
    p2 = dict(frame=[1, 1], xy=[(5, 9), (40, 2)], ratio=[250, 300], params=batch_params([model_params(1600, 1, bias=0.5), model_params(3200, 0)]),
              flip=[0, 1], row_stream=[9, 9], seed=(9 << 32) + 2, first_sample=40, draw=7)
    inputs = b.capture_inputs(2, DEV)
    b.update(inputs, shape, **p1)
    noisy, clean, noise = (torch.empty(2, 4, c, c, device=DEV) for _ in range(3))
    used = {k: torch.empty((2, 4, c) if k == "rows" else (2, 4, c, c), device=DEV) for k in VARIATES}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.launch(inputs, fd, noisy, clean, noise, used=used)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch(inputs, fd, noisy, clean, noise, used=used)
    bufs = [noisy, clean, noise] + [used[k] for k in VARIATES]
    for prm in (p1, p2, p1):
        b.update(inputs, shape, **prm)
        for t in bufs:
            t.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        want = b(fd, **prm, return_noise=True, return_draws=True)
        assert len(want) == len(bufs) and all(torch.equal(x, y) for x, y in zip(bufs, want))
    assert float(used["counts"].abs().max()) > 0 and not torch.equal(want[0], want[1])


@pytest.mark.gpu
def test_the_public_path_trains_a_step_and_scores_against_poisson_gaussian():
    import torch.nn.functional as F
    from noisediff_amd import CameraNoiseModel, PhysicsNoiseBatchBuilder, TrainableLSID, noise_stats, physics_frames, raw, train
    from noisediff_amd.spec import lsid_param_spec
    frames = np.floor(synth.uniform(9, "physics.t.step", (2, 136, 208), 400.0, 3000.0).numpy()).astype(np.uint16)
    fd = _dev_frames(frames)
    model = CameraNoiseModel(table())
    prm = model.draw([1600, 25600], seed=5, first_sample=10, read="tukey")
    b = PhysicsNoiseBatchBuilder(64)
    call = dict(frame=[0, 1], xy=[(4, 2), (38, 3)], ratio=[250, 300], params=prm, flip=[0, 1], seed=5, first_sample=10, draw=1)
    noisy, clean, noise = b(fd, **call, return_noise=True)
    assert noisy.shape == (2, 4, 64, 64) and torch.isfinite(noisy).all() and torch.isfinite(clean).all() and float(noisy.std()) > 0
    assert torch.equal(noise, noisy - clean) and float(noisy.min()) >= 0 and float(noisy.max()) <= 1
    net = TrainableLSID(SimpleNamespace())
    net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
    net = net.to(DEV).hip()
    opt = train.Adam(net.parameters(), lr=1e-4)
    opt.zero_grad(set_to_none=True)
    loss = F.l1_loss(net(noisy), clean)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    pg_noisy, pg_clean = raw.PoissonGaussianBatchBuilder(64)(fd, [0, 1], call["xy"], call["ratio"], k=[1.53008, 24.48128], var=[40.0, 670.0], flip=[0, 1], seed=5)
    kld = noise_stats.noise_kld(noise, pg_noisy - pg_clean)
    assert all(math.isfinite(float(kld[k])) for k in ("kl_fwd", "kl_inv", "kl_sym"))
    # whole frames: physics_frames equals the entry with one window per frame
    n2, c2, z2 = physics_frames(fd, [1, 0], [300, 250], {k: v[::-1].copy() for k, v in prm.items()}, seed=5, first_sample=3, draw=2, return_noise=True)
    specs = [(1, 0, 0, 0, 300, {k: v[1] for k, v in prm.items()}), (0, 0, 0, 0, 250, {k: v[0] for k, v in prm.items()})]
    want = _run(fd, _rows(specs, 3), 68, 104, key=dict(seed=5, first_sample=3, draw=2), want=("noisy", "clean", "noise"))
    assert np.array_equal(_np(n2), want["noisy"]) and np.array_equal(_np(c2), want["clean"]) and np.array_equal(_np(z2), want["noise"])
    mosaic = raw.to_bayer(n2, [512] * 4)
    assert tuple(mosaic.shape) == (2, 136, 208)
