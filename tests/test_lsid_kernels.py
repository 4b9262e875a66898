"""LSID's backward entry points (noisediff_amd/lsid_train.py), one by one, against a bit-for-bit twin where the library has one and against float64
on the CPU everywhere: the gradient join, the 3x3 weight gradients with LeakyReLU on load (one source and the concat), conv10's weight gradient,
and the ConvTranspose2d(2, s=2) weight gradient, data gradient and forward store with the crop -- at LSID's own layers and at the odd sizes where
the crops and the partial pooling windows are.  Every output starts as NaN (an unwritten element shows) and every call runs twice (same bits).
Bounds: 2e-5 of max(1, max |ref|) for convolution weight gradients and GEMM outputs, 2e-5 * max(1, sqrt(N / 4096)) for sums over N pixels."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from noisediff_amd import _lib as L, lsid, lsid_train, synth
from noisediff_amd.lsid import _sizes
from noisediff_amd.spec import LSID_STAGES
from util import rel_err

DEV = torch.device("cuda", 0)
SLOPE = 0.2


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(17, name, shape, lo, hi)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _leaky32(x):
    """The activated fp32 copy, as the kernels form it on load: max(x, 0.2 x)."""
    return torch.maximum(x, x * SLOPE)


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _twice(fn):
    """fn() -> tuple of device tensors (fresh NaN-filled outputs); runs it twice and asserts the same bits."""
    runs = []
    for _ in range(2):
        out = fn()
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in out])
    for a, b in zip(*runs):
        assert not a.isnan().any(), "an output element was not written"
        assert torch.equal(a, b), "two runs differ"
    return runs[0]


def _sum_tol(n):
    return 2e-5 * max(1.0, (n / 4096) ** 0.5)


# ====================================================================================================== 1. the gradient join
JOIN_SHAPES = [(1, 1, 1, 4), (2, 3, 5, 8), (1, 9, 11, 32), (1, 17, 1, 64), (2, 36, 44, 32), (4, 256, 256, 32)]


def _grid_z(name, shape):
    """Multiples of 0.5 in [-2, 2] (ties in most windows), a quarter of the zeros made -0.0."""
    z = torch.round(U(name, shape, -2.0, 2.0) * 2.0) / 2.0
    neg = U(name + ".sign", shape, 0.0, 1.0) < 0.25
    return torch.where((z == 0) & neg, torch.full_like(z, -0.0), z)


def _join_ref(z, d_direct, d_pool):
    """fp32 on the CPU in the kernel's order: (d_direct + scatter) * slope, scatter = max_pool2d(ceil_mode=True)'s input gradient."""
    B, H, W, Cc = z.shape
    s = torch.zeros_like(z) if d_direct is None else d_direct.clone()
    if d_pool is not None:
        zt = z.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        F.max_pool2d(zt, 2, 2, ceil_mode=True).backward(d_pool.permute(0, 3, 1, 2).contiguous())
        s = s + zt.grad.permute(0, 2, 3, 1)
    return s * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))


def _join(z, dz, dd, ld, dp):
    B, H, W, Cc = z.shape
    L.call("nd_leaky_grad_join_f32", z.data_ptr(), dz.data_ptr(), dd, ld, None if dp is None else dp.data_ptr(), B, H, W, Cc, _st())


@pytest.mark.parametrize("shape", JOIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("call", ["direct", "direct_aliased", "pool", "both_skip_half"])
def test_the_gradient_join_is_the_cpu_scatter_times_the_slope_exactly(shape, call):
    B, H, W, Cc = shape
    tag = f"join.{call}.{'x'.join(map(str, shape))}"
    z = _grid_z(tag + ".z", shape)
    wide = U(tag + ".dd", (B, H, W, 2 * Cc))
    dp = U(tag + ".dp", (B, (H + 1) // 2, (W + 1) // 2, Cc)) if call in ("pool", "both_skip_half") else None
    direct = None if call == "pool" else (wide[..., Cc:].contiguous() if call == "both_skip_half" else wide[..., :Cc].contiguous())
    want = _join_ref(z, direct, dp)
    zd, wd = z.to(DEV), wide.to(DEV)
    pd = None if dp is None else dp.to(DEV)
    dense = None if direct is None else direct.to(DEV)

    def run():
        if call == "direct_aliased":                                    # as the network calls it: dz is the direct gradient's buffer
            dz = dense.clone()
            _join(zd, dz, dz.data_ptr(), Cc, None)
            return (dz,)
        dz = _nan(B, H, W, Cc)
        if call == "direct":
            _join(zd, dz, dense.data_ptr(), Cc, None)
        elif call == "pool":
            _join(zd, dz, None, Cc, pd)
        else:                                                           # the skip half of a 2c-wide data gradient, as _lsid_hip_backward passes it
            _join(zd, dz, wd.data_ptr() + 4 * Cc, 2 * Cc, pd)
        return (dz,)

    (got,) = _twice(run)
    assert torch.equal(got, want)


def test_the_gradient_join_routes_a_nan_as_pytorch_does():
    """A NaN in a window takes the pooled gradient (max_pool2d_with_indices: `val > maxval || isnan(val)`); its slope is 0.2."""
    B, H, W, Cc = 1, 5, 7, 8
    z = _grid_z("join.nan.z", (B, H, W, Cc))
    z[0, 0, 1, 0] = float("nan")                                         # second element of the first window
    z[0, 2, 2, 3] = float("nan")                                         # first element of a window: it stays the maximum
    z[0, 4, 6, 5] = float("nan")                                         # the corner window, clamped to one element
    z[0, 3, 2, 1] = float("nan")
    z[0, 3, 3, 1] = float("nan")                                         # two NaNs in one window: the last one wins, as on the CPU
    dd = U("join.nan.dd", (B, H, W, Cc))
    dp = U("join.nan.dp", (B, 3, 4, Cc))
    want = _join_ref(z, dd, dp)
    zd, ddd, pd = z.to(DEV), dd.to(DEV), dp.to(DEV)

    def run():
        dz = _nan(B, H, W, Cc)
        _join(zd, dz, ddd.data_ptr(), Cc, pd)
        return (dz,)

    (got,) = _twice(run)
    assert not want.isnan().any()
    assert torch.equal(got, want)


def test_the_gradient_join_refuses_bad_arguments():
    B, H, W, Cc = 1, 4, 4, 8
    z, dz, wide, dp = _nan(B, H, W, Cc), _nan(B, H, W, Cc), _nan(B, H, W, 2 * Cc), _nan(B, 2, 2, Cc)
    with pytest.raises(L.HipError):                                     # pixel stride not a multiple of 4
        _join(z, dz, wide.data_ptr(), Cc + 2, None)
    with pytest.raises(L.HipError):                                     # dz aliasing the pooled gradient
        L.call("nd_leaky_grad_join_f32", z.data_ptr(), dp.data_ptr(), None, Cc, dp.data_ptr(), B, H, W, Cc, _st())
    with pytest.raises(L.HipError):                                     # neither gradient
        _join(z, dz, None, Cc, None)
    with pytest.raises(L.HipError):                                     # dz aliasing a strided direct gradient
        L.call("nd_leaky_grad_join_f32", z.data_ptr(), wide.data_ptr(), wide.data_ptr(), 2 * Cc, None, B, H, W, Cc, _st())
    torch.cuda.synchronize()


# ====================================================================================================== 2. 3x3 weight gradient, leaky on load
FORMS = (1, 2, 3)                       # nine taps, Winograd domain on four waves, on eight waves


@pytest.fixture
def wgrad_form():
    """Pins a form of the 3x3 weight gradients for a test and restores the product's choice (by the shape) afterwards."""
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(-1)
    yield lib.nd_conv3x3_wgrad_form
    lib.nd_conv3x3_wgrad_form(was)


def _under_pin(pin, question, *shape):
    """The library's answer to one of its weight-gradient questions (nd_conv3x3_wgrad_plan / nd_conv3x3_wgrad_cat_takes) under a pin of the form; the
    pin in force before is put back."""
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(pin)
    try:
        return int(getattr(lib, question)(*shape))
    finally:
        lib.nd_conv3x3_wgrad_form(was)


def _plan(B, H, W, cin, cout, pin):
    return _under_pin(pin, "nd_conv3x3_wgrad_plan", B, H, W, cin, cout)


def _lsid_wgrad_layers():
    """conv{i}_2 (c, c) and conv{i}_1 (c / 2, c) of LSID at the stage sizes of 64x64, 36x44, 33x47, and stage 1 of 256x256."""
    cases = []
    for B, H, W in ((2, 64, 64), (1, 36, 44), (2, 33, 47)):
        for i, (h, w) in enumerate(_sizes(H, W), start=1):
            c = LSID_STAGES[i - 1]
            cases.append((B, h, w, c, c, f"{H}x{W}.conv{i}_2"))
            if i > 1:
                cases.append((B, h, w, c // 2, c, f"{H}x{W}.conv{i}_1"))
    cases.append((1, 256, 256, 32, 32, "256x256.conv1_2"))
    return cases


WGRAD_CASES = _lsid_wgrad_layers()


def _wgrad(entry, x, ldx, dy, B, H, W, cin, cout, ws):
    dw, db = _nan(cout, cin, 3, 3), _nan(cout)
    L.call(entry, x.data_ptr(), ldx, dy.data_ptr(), cout, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, H, W, cin, cout, _st())
    return dw, db


def _check_wgrad_leaky(B, H, W, cin, cout, tag, wgrad_form, x_lo=-1.5, x_hi=1.0, xpad=0):
    lib = L.load()
    ldx = cin + xpad
    xw = U(tag + ".x", (B, H, W, ldx), x_lo, x_hi).to(DEV)
    x = xw[..., xpad:]                                                   # a channel slice when xpad > 0 (16-byte aligned start)
    dy = U(tag + ".dy", (B, H, W, cout)).to(DEV)
    xa = _leaky32(x).contiguous()
    wsz = {}
    for form in (0,) + FORMS:
        wgrad_form(form)
        wsz[form] = int(lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, cin, cout))
    product = _plan(B, H, W, cin, cout, 0)
    assert wsz[0] == wsz[product], (tag, wsz)                           # the product runs the form the rule names
    ref = db64 = None
    for form in FORMS:
        wgrad_form(form)
        ws = torch.empty(wsz[form], device=DEV)
        got = _twice(lambda: _wgrad("nd_conv3x3_wgrad_leaky_nhwc_f32", x, ldx, dy, B, H, W, cin, cout, ws))
        twin = _twice(lambda: _wgrad("nd_conv3x3_wgrad_nhwc_f32", xa, cin, dy, B, H, W, cin, cout, ws))
        assert torch.equal(got[0], twin[0]) and torch.equal(got[1], twin[1]), (tag, form)
        if _plan(B, H, W, cin, cout, form) == form:       # (a pin that does not take the shape ran another form: checked there)
            if ref is None:
                ref = torch.nn.grad.conv2d_weight(F.leaky_relu(_nchw64(x), SLOPE), (cout, cin, 3, 3), _nchw64(dy), padding=1).numpy()
                db64 = _nchw64(dy).sum(dim=(0, 2, 3)).numpy()
            assert rel_err(got[0].numpy(), ref) < 2e-5, (tag, form)
            assert rel_err(got[1].numpy(), db64) < _sum_tol(B * H * W), (tag, form)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: c[-1])
def test_wgrad_leaky_is_the_plain_wgrad_of_the_activated_copy_and_float64(case, wgrad_form):
    B, H, W, cin, cout, tag = case
    _check_wgrad_leaky(B, H, W, cin, cout, "wgl." + tag, wgrad_form)


def test_wgrad_leaky_reads_a_channel_slice_and_an_all_negative_input(wgrad_form):
    _check_wgrad_leaky(2, 16, 32, 64, 64, "wgl.slice", wgrad_form, xpad=32)                        # ldx > cin, Winograd shape
    _check_wgrad_leaky(1, 9, 11, 32, 64, "wgl.slice9", wgrad_form, xpad=16)                        # ldx > cin, nine taps
    _check_wgrad_leaky(2, 16, 32, 64, 64, "wgl.neg", wgrad_form, x_lo=-2.0, x_hi=-0.01)            # every input on the 0.2 branch
    _check_wgrad_leaky(1, 9, 11, 32, 64, "wgl.neg9", wgrad_form, x_lo=-2.0, x_hi=-0.01)


def test_the_lsid_wgrad_table_reaches_every_form():
    """By the library's own answer (nd_conv3x3_wgrad_plan), the product picks the nine-tap form (1) or the
    four-wave Winograd-domain form (2) on LSID's layers -- never the eight-wave form (3), whose threshold no LSID layer here reaches.  Form 3 runs on
    this table only where the tests pin it (cout % 64 == 0: 64x64 stages 2 and 3).  The library's own evidence is the workspace it asks for: the
    Winograd-domain layout is larger than the nine-tap one on the 64x64 stages 1 to 3, so form 0 there is shown to be a Winograd form.  The
    workspace cannot tell form 2 from form 3 (the same size on these shapes); _check_wgrad_leaky asserts form 0's size equals the named form's."""
    product = {_plan(B, H, W, cin, cout, 0) for B, H, W, cin, cout, _ in WGRAD_CASES}
    pinned = {_plan(B, H, W, cin, cout, f) for B, H, W, cin, cout, _ in WGRAD_CASES for f in FORMS}
    assert product == {1, 2} and 3 not in product                    # form 3: reached by pinning only
    assert pinned == {1, 2, 3}
    assert {tag for B, H, W, cin, cout, tag in WGRAD_CASES if _plan(B, H, W, cin, cout, 3) == 3} == {
        "64x64.conv2_2", "64x64.conv2_1", "64x64.conv3_2", "64x64.conv3_1"}
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(-1)
    try:                                                                # the workspace asked for shows the Winograd domain where its layout is the larger
        shown = set()
        for B, H, W, cin, cout, tag in WGRAD_CASES:
            sizes = []
            for f in (0, 1):
                lib.nd_conv3x3_wgrad_form(f)
                sizes.append(int(lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, cin, cout)))
            if sizes[0] != sizes[1]:
                shown.add(tag)
                assert _plan(B, H, W, cin, cout, 0) != 1, tag
    finally:
        lib.nd_conv3x3_wgrad_form(was)
    assert shown >= {"64x64.conv1_2", "64x64.conv2_1", "64x64.conv2_2", "64x64.conv3_1", "64x64.conv3_2"}


# ====================================================================================================== 3. concat weight gradient, leaky on the second source
def _cat_cases():
    cases = []
    for B, H, W in ((2, 64, 64), (1, 36, 44), (2, 33, 47)):
        sizes = _sizes(H, W)
        for j in range(6, 10):
            i = 10 - j
            c = LSID_STAGES[i - 1]
            h, w = sizes[i - 1]
            cases.append((B, h, w, c, c, c, f"{H}x{W}.conv{j}_1"))
    cases += [(2, 32, 32, 16, 48, 32, "c16_48"), (1, 16, 32, 48, 16, 64, "c48_16"), (2, 9, 11, 32, 32, 32, "9x11")]
    return cases


def _cat_takes(B, H, W, c0, c1, cout, pin, ldx0=None):
    return bool(_under_pin(pin, "nd_conv3x3_wgrad_cat_takes", B, H, W, c0, c1, cout, c0 if ldx0 is None else ldx0, c1, cout))


@pytest.mark.parametrize("form", [0, 1, 3])
@pytest.mark.parametrize("case", _cat_cases(), ids=lambda c: c[-1])
def test_wgrad_cat_leaky_second_activates_the_second_source_only(case, form, wgrad_form):
    """x0 mostly negative: an activation on the wrong source moves most of dw.  Winograd branch: the same bits as nd_conv3x3_wgrad_cat_nhwc_f32 on
    (x0, leaky(x1)); nine-tap branch: per source the same bits as nd_conv3x3_wgrad_nhwc_f32 on x0 / leaky(x1), the bias gradient once."""
    B, H, W, c0, c1, cout, tag = case
    wgrad_form(form)
    lib = L.load()
    tag = f"wgc.{tag}"
    x0w = U(tag + ".x0", (B, H, W, c0 + 16), -1.5, 0.25).to(DEV)
    x0 = x0w[..., 16:]                                                   # the up-sampled half: a channel slice (ldx0 > c0)
    x1 = U(tag + ".x1", (B, H, W, c1), -1.0, 1.0).to(DEV)
    dy = U(tag + ".dy", (B, H, W, cout)).to(DEV)
    x1a = _leaky32(x1).contiguous()
    ws = torch.empty(int(lib.nd_conv3x3_wgrad_cat_workspace_floats(B, H, W, c0, c1, cout)), device=DEV)

    def run(entry, second):
        dw, db = _nan(cout, c0 + c1, 3, 3), _nan(cout)
        L.call(entry, x0.data_ptr(), c0 + 16, c0, second.data_ptr(), c1, c1, dy.data_ptr(), cout, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
               B, H, W, cout, _st())
        return dw, db

    dw, db = _twice(lambda: run("nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32", x1))
    if _cat_takes(B, H, W, c0, c1, cout, form, ldx0=c0 + 16):
        tw, tb = _twice(lambda: run("nd_conv3x3_wgrad_cat_nhwc_f32", x1a))
        assert torch.equal(dw, tw) and torch.equal(db, tb)
    else:                                                               # nine taps per source, whatever the pin asks for the single-source entry
        wgrad_form(1)
        w0 = torch.empty(int(lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, c0, cout)), device=DEV)
        w1 = torch.empty(int(lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, c1, cout)), device=DEV)
        t0 = _twice(lambda: _wgrad("nd_conv3x3_wgrad_nhwc_f32", x0, c0 + 16, dy, B, H, W, c0, cout, w0))
        t1 = _twice(lambda: _wgrad("nd_conv3x3_wgrad_nhwc_f32", x1a, c1, dy, B, H, W, c1, cout, w1))
        wgrad_form(form)
        assert torch.equal(dw[:, :c0], t0[0]) and torch.equal(dw[:, c0:], t1[0])
        assert torch.equal(db, t0[1])
    x64 = torch.cat((_nchw64(x0), F.leaky_relu(_nchw64(x1), SLOPE)), 1)
    ref = torch.nn.grad.conv2d_weight(x64, (cout, c0 + c1, 3, 3), _nchw64(dy), padding=1)
    assert rel_err(dw.numpy(), ref.numpy()) < 2e-5
    assert rel_err(db.numpy(), _nchw64(dy).sum(dim=(0, 2, 3)).numpy()) < _sum_tol(B * H * W)


def test_the_cat_table_takes_both_branches():
    cases = _cat_cases()
    assert any(_cat_takes(B, H, W, c0, c1, co, 0) for B, H, W, c0, c1, co, _ in cases)
    assert any(not _cat_takes(B, H, W, c0, c1, co, 0) for B, H, W, c0, c1, co, _ in cases)


# ====================================================================================================== 4. conv10's weight gradient
@pytest.mark.parametrize("B,H,W,xpad", [(2, 33, 47, 0), (1, 36, 44, 0), (4, 256, 256, 0), (1, 36, 44, 12)])
def test_conv10_wgrad_leaky_is_the_plain_wgrad_of_the_activated_copy_and_float64(B, H, W, xpad):
    lib = L.load()
    N, cin, cout = B * H * W, 32, 4
    tag = f"lw.{B}x{H}x{W}.{xpad}"
    xw = U(tag + ".x", (N, cin + xpad), -1.5, 1.0).to(DEV)
    x = xw[:, xpad:]
    dy = U(tag + ".dy", (N, cout)).to(DEV)
    xa = _leaky32(x).contiguous()
    ws = torch.empty(int(lib.nd_linear_wgrad_workspace_floats(N, cin, cout)), device=DEV)

    def run(entry, xx, ldx):
        dw, db = _nan(cout, cin), _nan(cout)
        L.call(entry, xx.data_ptr(), ldx, dy.data_ptr(), cout, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), N, cin, cout, _st())
        return dw, db

    dw, db = _twice(lambda: run("nd_linear_wgrad_leaky_f32", x, cin + xpad))
    tw, tb = _twice(lambda: run("nd_linear_wgrad_f32", xa, cin))
    assert torch.equal(dw, tw) and torch.equal(db, tb)
    x64, g64 = F.leaky_relu(x.double().cpu(), SLOPE), dy.double().cpu()
    assert rel_err(dw.numpy(), (g64.T @ x64).numpy()) < _sum_tol(N)
    assert rel_err(db.numpy(), g64.sum(0).numpy()) < _sum_tol(N)


# ====================================================================================================== 5./6. ConvTranspose2d(2, s=2) + crop
def _crop(h, w, kind):
    return (2 * h - (kind & 1), 2 * w - (kind >> 1))


# (cin, c, B, h, w, crop kind): kind 0 (2h, 2w), 1 (2h-1, 2w), 2 (2h, 2w-1), 3 (2h-1, 2w-1) -- every layer of LSID's up path plus a small one
CONVT_CASES = [(512, 256, 1, 3, 3, 3), (512, 256, 3, 1, 2, 1), (256, 128, 1, 5, 6, 3), (256, 128, 3, 2, 1, 2), (128, 64, 1, 9, 12, 1),
               (128, 64, 3, 4, 4, 0), (64, 32, 1, 17, 24, 3), (64, 32, 3, 5, 1, 2), (64, 32, 1, 8, 8, 0), (32, 16, 3, 1, 1, 3), (32, 16, 1, 7, 5, 1),
               (32, 16, 3, 6, 9, 2)]


def _convt_id(c):
    cin, cc, B, h, w, k = c
    return f"{cin}to{cc}.B{B}.{h}x{w}to{'x'.join(map(str, _crop(h, w, k)))}"


def test_the_convt_table_has_every_crop_and_batch():
    kinds = {k for *_, k in CONVT_CASES}
    assert kinds == {0, 1, 2, 3}
    assert {B for _, _, B, *_ in CONVT_CASES} == {1, 3}
    assert any(h == 1 for _, _, _, h, _, _ in CONVT_CASES) and any(w == 1 for _, _, _, _, w, _ in CONVT_CASES)
    assert {(cin, c) for cin, c, *_ in CONVT_CASES} == {(512, 256), (256, 128), (128, 64), (64, 32), (32, 16)}


def _convt_data(case):
    cin, c, B, h, w, kind = case
    uh, uw = _crop(h, w, kind)
    tag = "ct." + _convt_id(case)
    x = U(tag + ".x", (B, h, w, cin), -1.5, 1.0)
    wt = U(tag + ".w", (cin, c, 2, 2)) / cin ** 0.5
    dc = U(tag + ".dc", (B, uh, uw, 2 * c))                              # [d up | d skip]: d_up is the first c channels, pixel stride 2c
    return x, wt, dc, uh, uw


def _convt_ref64(x, wt, dc, uh, uw):
    """float64 autograd of conv_transpose2d(leaky(x), w, stride=2)[:, :, :up_h, :up_w] with d_up as the output gradient: (out, d leaky(x), dw)."""
    c = wt.shape[1]
    xa = F.leaky_relu(_nchw64(x), SLOPE).requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    out = F.conv_transpose2d(xa, w64, stride=2)[:, :, :uh, :uw]
    out.backward(_nchw64(dc[..., :c]))
    return out.detach(), xa.grad, w64.grad


def _pack_pw(m, cin, cout, unshuffle_c=0):
    out = torch.empty(int(L.load().nd_pack_pointwise_weight_floats(cin, cout)), device=DEV)
    L.call("nd_pack_pointwise_weight", m.data_ptr(), out.data_ptr(), cin, cout, unshuffle_c, _st())
    return out


@pytest.mark.parametrize("case", CONVT_CASES, ids=_convt_id)
def test_convt_wgrad_leaky_with_the_crop_matches_the_unshuffled_linear_wgrad_and_float64(case):
    """nd_convt2x2_wgrad_leaky_f32: bit for bit nd_linear_wgrad_leaky_f32 on the explicitly zero-padded, unshuffled d_up (the same GEMM, the same
    split), and float64 autograd."""
    lib = L.load()
    cin, c, B, h, w, kind = case
    x, wt, dc, uh, uw = _convt_data(case)
    xd, dcd = x.to(DEV), dc.to(DEV)
    N = B * h * w
    ws = torch.empty(int(lib.nd_convt2x2_wgrad_workspace_floats(B, h, w, cin, c)), device=DEV)

    def run():
        dw = _nan(cin, c, 2, 2)
        L.call("nd_convt2x2_wgrad_leaky_f32", xd.data_ptr(), cin, dcd.data_ptr(), 2 * c, dw.data_ptr(), ws.data_ptr(), B, h, w, cin, c, uh, uw, _st())
        return (dw,)

    (dw,) = _twice(run)
    pad = torch.zeros(B, 2 * h, 2 * w, c)
    pad[:, :uh, :uw] = dc[..., :c]
    dyu = pad.reshape(B, h, 2, w, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(N, 4 * c).to(DEV).contiguous()     # rows (b y x), columns (p1 p2 c)
    lw_ws = torch.empty(int(lib.nd_linear_wgrad_workspace_floats(N, cin, 4 * c)), device=DEV)

    def twin():
        t = _nan(4 * c, cin)
        L.call("nd_linear_wgrad_leaky_f32", xd.data_ptr(), cin, dyu.data_ptr(), 4 * c, t.data_ptr(), None, lw_ws.data_ptr(), N, cin, 4 * c, _st())
        return (t,)

    (t,) = _twice(twin)
    assert torch.equal(dw, t.reshape(2, 2, c, cin).permute(3, 2, 0, 1))
    _, _, dw64 = _convt_ref64(x, wt, dc, uh, uw)
    assert rel_err(dw.numpy(), dw64.numpy()) < _sum_tol(N)


@pytest.mark.parametrize("case", CONVT_CASES, ids=_convt_id)
def test_convt_dgrad_reads_the_cropped_unshuffle_as_zeros(case):
    """The data gradient as _lsid_hip_backward builds it (lsid_train.convt2x2_dgrad: the packing with unshuffle_c = c, d_up the first half of a 2c-wide
    tensor, the crop): float64 autograd (before the slope, which the join applies), and bit for bit the uncropped unshuffle GEMM over a zero-padded
    copy of d_up."""
    cin, c, B, h, w, kind = case
    x, wt, dc, uh, uw = _convt_data(case)
    dcd, wtd = dc.to(DEV), wt.to(DEV)
    pad = torch.zeros(B, 2 * h, 2 * w, 2 * c)
    pad[:, :uh, :uw] = dc
    padd = pad.to(DEV)

    def run(src, sh, sw):
        r = lsid._Launcher(DEV, False)
        t = lsid_train.convt2x2_dgrad(r, wtd, src, 2 * c, B, h, w, sh, sw)
        return (t,)

    (got,) = _twice(lambda: run(dcd, uh, uw))
    (full,) = _twice(lambda: run(padd, 2 * h, 2 * w))
    assert torch.equal(got, full)
    wp = _pack_pw(wtd.reshape(cin, 4 * c).contiguous(), 4 * c, cin, c)

    def plain():                                                        # the uncropped read through the plain entry: the same bits
        out = _nan(B, h, w, cin)
        s = L.Src()
        s.p0, s.c0, s.ld0, s.unshuffle = padd.data_ptr(), 4 * c, 2 * c, 1
        d = L.Pointwise()
        d.src, d.weight, d.out = s, wp.data_ptr(), out.data_ptr()
        d.B, d.HW, d.W, d.cin, d.cout, d.ldo = B, h * w, w, 4 * c, cin, cin
        L.call("nd_pointwise_gemm_nhwc_f32", C.byref(d), _st())
        return (out,)

    (p,) = _twice(plain)
    assert torch.equal(got, p)
    _, dx64, _ = _convt_ref64(x, wt, dc, uh, uw)
    assert rel_err(_nchw64(got).numpy(), dx64.numpy()) < 2e-5


@pytest.mark.parametrize("case", CONVT_CASES, ids=_convt_id)
def test_convt_forward_pixel_shuffle_store_crops_as_float64(case):
    """The forward LSID records (lsid.lsid_forward_hip): leaky(x) through the pointwise GEMM to 4c columns, the pixel-shuffle store cropped to
    (up_h, up_w); every element written, float64 conv_transpose2d + crop."""
    cin, c, B, h, w, kind = case
    x, wt, dc, uh, uw = _convt_data(case)
    xd = x.to(DEV)
    m = wt.permute(2, 3, 1, 0).reshape(4 * c, cin).contiguous().to(DEV)
    wp = _pack_pw(m, cin, 4 * c)

    def run():
        out = _nan(B, uh, uw, c)
        s = L.Src()
        s.p0, s.c0, s.ld0, s.mode = xd.data_ptr(), cin, cin, L.PRO_LEAKY
        d = L.Pointwise()
        d.src, d.weight, d.out = s, wp.data_ptr(), out.data_ptr()
        d.B, d.HW, d.W, d.cin, d.cout, d.ldo = B, h * w, w, cin, 4 * c, c
        d.shuffle_c, d.shuffle_h, d.shuffle_w = c, uh, uw
        L.call("nd_pointwise_gemm_nhwc_f32", C.byref(d), _st())
        return (out,)

    (got,) = _twice(run)
    out64, _, _ = _convt_ref64(x, wt, dc, uh, uw)
    assert rel_err(_nchw64(got).numpy(), out64.numpy()) < 2e-5
