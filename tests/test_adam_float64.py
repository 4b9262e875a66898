"""The weight path of a training step per element: adam.hip's three entries against float64, and the F(4x4) weight packers (conv3x3_wino4.hip).

Adam.  The references are tests/adam_ref.py: ``step64`` (torch.optim.Adam's update in float64 with the double hyper-parameters), ``step32``
(torch.optim.Adam(foreach=False) itself in fp32 on the CPU) and ``kernel32`` (adam.hip's documented arithmetic in numpy fp32).  Every comparison
is util.derived(kernel, step64, step32): 4 x the fp32 reference's own error + one ulp of the scale, no floor of 1 and no tolerance literal.
CPU: step64 is torch.optim.Adam in float64; kernel32 with the complements 1 - beta taken in double meets the bound on every case the GPU tests
run; kernel32 with 1.0f - (float)beta does not (v at beta2 = 0.999) -- the test can tell the two apart.
GPU, C ABI: ONE step from a state the test wrote, 15 items in one launch whose chunk table is in a fixed SHUFFLED order (and once more in item
order: the same bits).  Sizes 1, 7, 8191, 8192, 8193, 16384, 16389 with vec4 = 1; 8192 and 16389 with vec4 = 0 and each of p, g, m, v in turn
one float past a 16-byte boundary -- the MISALIGNED WHOLE-CHUNK case (the scalar path on hi - lo == ADAM_CHUNK).  Every p, g, m, v, every
step counter and the device learning rate sits in its own buffer between NaN fences.  Six magnitude families, each judged on its own scale.
GPU, train.Adam: three steps of the three optimizer forms, one gradient an unaligned view, one parameter skipping a step.

Packers.  nd_pack_conv3x3_wino4_weights_batch equals the single packers bit for bit; U decoded by the documented layout against G g G^T in
float64 with exact G under util.derived.
"""
import numpy as np
import pytest
import torch
from torch import nn

import adam_ref as A
import conv3x3_ref as R3
from noisediff_amd import _lib as L
from util import derived

gpu = pytest.mark.gpu
ENTRIES = ("nd_adam_step_f32", "nd_adam_step_capturable_f32", "nd_adam_step_capturable_lr_f32")
LR32 = float(np.float32(A.LR))                                        # the learning rate a capturable kernel can see (a float argument, a float in memory)
CASES = [(f, b) for b in A.BETAS for f in range(len(A.FAMILIES))]
CASE_IDS = [f"g{A.FAMILIES[f][0]:g}-p{A.FAMILIES[f][1]:g}-wd{A.FAMILIES[f][2]:g}-b{b[1]:g}" for f, b in CASES]


def lr_seen(entry):
    return A.LR if entry == "nd_adam_step_f32" else LR32


def judge(got, refs, what):
    """(p, m, v) of one item against its (step64, step32)."""
    r64, r32 = refs
    for name, g, a, b in zip(("p", "m", "v"), got, r64, r32):
        derived(g, a, b, f"{what} {name}")


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("betas", A.BETAS, ids=str)
def test_step64_is_torch_adam_in_float64(betas, weight_decay):
    """Five steps from zero state: the restatement and torch.optim.Adam on float64 CPU tensors agree to 1e-14 relative (float64 rounding of a dozen
    operations: nothing of the formula differs)."""
    rng = np.random.default_rng(5)
    n = 1000
    p = rng.uniform(-1.0, 1.0, n)
    ours = (p, np.zeros(n), np.zeros(n))
    theirs = (p, np.zeros(n), np.zeros(n))
    for t in range(1, 6):
        g = rng.uniform(-1.0, 1.0, n) * (0.5 + t)
        ours = A.step64(ours[0], g, ours[1], ours[2], t, A.LR, *betas, A.EPS, weight_decay)
        theirs = A.torch_adam(theirs[0], g, theirs[1], theirs[2], t, A.LR, *betas, A.EPS, weight_decay, torch.float64)
        for name, a, b in zip(("p", "m", "v"), ours, theirs):
            assert b.dtype == np.float64
            assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b)), (t, name)


def test_the_states_cover_what_they_claim():
    lay = A.layout()
    assert len(lay) >= 11 and [n for n, v4, off, t in lay if v4] == list(A.SIZES)
    assert sorted((n, off) for n, v4, off, t in lay if not v4) == sorted((n, k) for n in A.MISALIGNED_SIZES for k in A.TENSORS)
    assert {t for _, _, _, t in lay} == set(A.STEPS)
    for f, (gs, ps, wd) in enumerate(A.FAMILIES):
        for s in A.states(f):
            assert float(np.min(np.abs(s["g"]), initial=1.0, where=s["g"] != 0)) ** 2 > 1e-30   # (no square near the fp32 subnormal range)
            if s["t"] == 1:
                assert not s["m"].any() and not s["v"].any()
                assert (wd == 0.0) == (not s["g"][A.zero_grad_indices(s["n"])].any())
            else:
                assert float(s["v"].min()) > 1e-30


@pytest.mark.parametrize("lr", [A.LR, LR32], ids=["lr_double", "lr_float"])
@pytest.mark.parametrize("family,betas", CASES, ids=CASE_IDS)
def test_the_documented_arithmetic_meets_the_bound(family, betas, lr):
    """kernel32 with w = float(1 - beta) stays within derived's bound of step64, given step32, on every item of every case the GPU tests run
    (measured: at most 0.56 of the bound): the GPU tests do not ask for more than the arithmetic can give."""
    wd = A.FAMILIES[family][2]
    for i, (s, refs) in enumerate(zip(A.states(family), A.references(family, betas, lr))):
        got = A.kernel32(s["p"], s["g"], s["m"], s["v"], s["t"], lr, *betas, A.EPS, wd, "double")
        judge(got, refs, f"item {i} (n {s['n']}, t {s['t']})")


@pytest.mark.parametrize("family", range(len(A.FAMILIES)))
def test_complements_taken_in_fp32_miss_the_bound(family):
    """1.0f - (float)0.999 is off from 0.001 by 1.3e-5 relative: every increment of v carries it.  With the betas as floats in the ABI the kernel
    could do no better; the bound rejects that arithmetic for v at (0.9, 0.999) in every family."""
    betas, wd = (0.9, 0.999), A.FAMILIES[family][2]
    failed = 0
    for s, (r64, r32) in zip(A.states(family), A.references(family, betas, A.LR)):
        got = A.kernel32(s["p"], s["g"], s["m"], s["v"], s["t"], A.LR, *betas, A.EPS, wd, "float")
        try:
            derived(got[2], r64[2], r32[2], "v")
        except AssertionError:
            failed += 1
    assert failed > 0


# ---------------------------------------------------------------------------------------------------------------- GPU: the C ABI
@pytest.fixture(scope="module")
def ctx():
    import hiputil
    return hiputil.Ctx()


class Fenced:
    """A host array in its own flat device buffer between GUARD NaN floats (and up to 4 more behind); ``shift`` = floats past a 16-byte boundary."""

    def __init__(self, a, shift=0):
        import hiputil as hu
        a = np.asarray(a, dtype=np.float32)
        self.n, self.lo = a.size, hu.GUARD + shift
        host = torch.full((a.size + 2 * hu.GUARD + 4,), float("nan"))
        host[self.lo: self.lo + self.n] = torch.from_numpy(np.array(a))
        self.sent = host.clone()
        self.dev = hu.dev(host)
        self.ptr = self.dev.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * shift

    def read(self, what):
        """The tensor as the device holds it; the fence must be intact."""
        host = self.dev.cpu()
        R3.only_nan_outside(host, (slice(self.lo, self.lo + self.n),), what)
        return host[self.lo: self.lo + self.n].numpy()

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.sent.numpy().view(np.uint32))


def chunk_pairs(sts, order):
    pairs = np.array([(i, c) for i, s in enumerate(sts) for c in range(-(-s["n"] // A.CHUNK))], dtype=np.int32)
    if order == "shuffled":
        pairs = pairs[np.random.default_rng(7).permutation(len(pairs))]
        assert (np.diff(pairs[:, 0]) < 0).any()                       # not item-major
    return pairs


class Launch:
    """Fresh fenced buffers for every item of a family, the hand-built nd_adam_item table and the chunk table in ``order``."""

    def __init__(self, entry, family, betas, order):
        import hiputil as hu
        self.entry, self.betas, self.wd = entry, betas, A.FAMILIES[family][2]
        self.sts = sts = A.states(family)
        self.bufs = [{k: Fenced(s[k], shift=int(s["off"] == k)) for k in A.TENSORS} for s in sts]
        self.counters = [Fenced([s["t"] - 1]) for s in sts]           # capturable forms: each item's own counter, t - 1 before the call
        self.lr_dev = Fenced([A.LR])
        items = np.zeros(len(sts), dtype=np.dtype(L.AdamItem))
        for k in A.TENSORS:
            items[k] = [b[k].ptr for b in self.bufs]
        items["n"] = [s["n"] for s in sts]
        items["vec4"] = [s["vec4"] for s in sts]
        for s, b in zip(sts, self.bufs):                              # vec4 = 1 is never passed with a misaligned pointer
            assert bool(s["vec4"]) == all(b[k].ptr % 16 == 0 for k in A.TENSORS)
        ts = np.array([s["t"] for s in sts], dtype=np.float64)
        if entry == "nd_adam_step_f32":                               # in double, as the header asks of the caller
            items["step_size"] = A.LR / (1.0 - betas[0] ** ts)
            items["bias2_sqrt"] = np.sqrt(1.0 - betas[1] ** ts)
        else:                                                         # ignored by the capturable forms: NaN would show in every result
            items["step_size"] = items["bias2_sqrt"] = np.nan
            items["step"] = [c.ptr for c in self.counters]
        self.items = items
        self.table = hu.dev(torch.from_numpy(items.view(np.uint8).copy()))
        pairs = chunk_pairs(sts, order)
        self.n_chunks = len(pairs)
        self.chunks = hu.dev(torch.from_numpy(pairs.copy()))

    def args(self, table=True, n_items=None, chunks=True, n_chunks=None, lr_dev=True, beta1=None, beta2=None, eps=A.EPS, wd=None):
        head = [self.table.data_ptr() if table else None, len(self.sts) if n_items is None else n_items,
                self.chunks.data_ptr() if chunks else None, self.n_chunks if n_chunks is None else n_chunks]
        if self.entry == "nd_adam_step_capturable_f32":
            head.append(A.LR)
        elif self.entry == "nd_adam_step_capturable_lr_f32":
            head.append(self.lr_dev.ptr if lr_dev else None)
        return head + [self.betas[0] if beta1 is None else beta1, self.betas[1] if beta2 is None else beta2, eps, self.wd if wd is None else wd]

    def run(self, ctx):
        L.call(self.entry, *self.args(), ctx.stream)
        ctx.sync()

    def results(self):
        """Per item (p, m, v); every fence intact, g and the device learning rate unchanged bit for bit."""
        out = []
        for i, (s, b) in enumerate(zip(self.sts, self.bufs)):
            got = {k: b[k].read(f"{self.entry} item {i} (n {s['n']}, {s['off']} misaligned) {k}") for k in A.TENSORS}
            assert np.array_equal(got["g"].view(np.uint32), s["g"].view(np.uint32)), f"item {i}: g was written"
            out.append((got["p"], got["m"], got["v"]))
        assert self.lr_dev.untouched()
        return out

    def counts(self):
        return [float(c.read(f"{self.entry} counter {i}")[0]) for i, c in enumerate(self.counters)]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ia, ib in zip(a, b) for x, y in zip(ia, ib))


@gpu
def test_the_chunk_is_8192_elements(ctx):
    assert ctx.lib.nd_adam_chunk_elements() == A.CHUNK == 8192


@gpu
@pytest.mark.parametrize("family,betas", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_one_step_from_a_given_state(ctx, entry, family, betas):
    """One launch over all 15 items with the chunk table shuffled: every item's p, m, v within derived's bound of step64; fences intact, g
    unchanged; zero gradients at t = 1 leave p to the bit and m = v = 0.0; the same bits with the table in item order and on a repeat; the
    capturable forms count t - 1 -> t -> t + 1."""
    capturable = entry != "nd_adam_step_f32"
    first = Launch(entry, family, betas, "shuffled")
    first.run(ctx)
    got = first.results()
    refs = A.references(family, betas, lr_seen(entry))
    for i, (s, g, r) in enumerate(zip(first.sts, got, refs)):
        judge(g, r, f"item {i} (n {s['n']}, t {s['t']}, vec4 {s['vec4']}, {s['off']} misaligned)")
        if s["t"] == 1 and first.wd == 0.0:
            z = A.zero_grad_indices(s["n"])
            assert np.array_equal(g[0][z].view(np.uint32), s["p"][z].view(np.uint32)), f"item {i}: p moved under a zero gradient"
            assert not g[1][z].view(np.uint32).any() and not g[2][z].view(np.uint32).any(), f"item {i}: m, v of a zero gradient are not +0.0"
    if capturable:
        assert first.counts() == [float(s["t"]) for s in first.sts]
    else:
        assert all(c.untouched() for c in first.counters)
    for order in ("item", "shuffled"):                                # no reductions: the chunk order and a repeat change no bit
        other = Launch(entry, family, betas, order)
        other.run(ctx)
        assert same_bits(other.results(), got), f"chunk table in {order} order: other bits"
    if capturable:
        other.run(ctx)                                                # a second call counts once more (its results: fences only)
        other.results()
        assert other.counts() == [float(s["t"] + 1) for s in other.sts]


BAD = [dict(table=False), dict(chunks=False), dict(n_items=0), dict(n_items=-1), dict(n_chunks=0), dict(n_chunks=-3),
       dict(beta1=-0.1), dict(beta1=1.0), dict(beta2=-1e-3), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1e-8), dict(wd=-0.01)]


@gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_arguments_launch_nothing(ctx, entry):
    run = Launch(entry, 0, A.BETAS[0], "shuffled")
    bad = BAD + ([dict(lr_dev=False)] if entry == "nd_adam_step_capturable_lr_f32" else [])
    for kw in bad:
        assert getattr(ctx.lib, entry)(*run.args(**kw), ctx.stream) == -1, f"{entry}{kw}: not ND_E_BADARG"
        assert entry in ctx.lib.nd_last_error().decode()
    ctx.sync()
    for b in run.bufs:
        assert all(b[k].untouched() for k in A.TENSORS)
    assert all(c.untouched() for c in run.counters) and run.lr_dev.untouched()


# ---------------------------------------------------------------------------------------------------------------- GPU: train.Adam
def adam_inputs():
    """Parameters of the one-step sizes and three steps of gradients (the gradient grows with the step, as in the older Adam test)."""
    rng = np.random.default_rng(11)
    ps = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in A.SIZES]
    gs = [[(rng.uniform(-1.0, 1.0, n) * (0.5 + step)).astype(np.float32) for n in A.SIZES] for step in range(3)]
    return ps, gs


VIEW, SKIPS = len(A.SIZES) - 1, 4                                     # the 16389-element gradient is an unaligned view; the 8193-element parameter skips step 2


@gpu
@pytest.mark.parametrize("form", ["host", "capturable", "capturable_lr"])
def test_train_adam_steps_each_parameter_from_its_own_state(form):
    """train.Adam with the class default betas (0.9, 0.999), three steps.  Before each step p, m, v are read back; after it they are held to
    step64 / step32 FROM THAT STATE, so nothing compounds.  The 16389-element parameter (two whole chunks and a tail) receives its gradient as a
    contiguous view one float into a fenced buffer: the layer must pass vec4 = 0 and the fence must survive.  The 8193-element parameter has no
    gradient on the second step: its count lags and its bias correction is its own."""
    import hiputil as hu
    from noisediff_amd import train
    dev = hu.DEV
    p0, grads = adam_inputs()
    ps = [nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in p0]
    if form == "host":
        opt, lr = train.Adam(ps, lr=A.LR), A.LR
    elif form == "capturable":
        opt, lr = train.Adam(ps, lr=A.LR, capturable=True), LR32
    else:
        opt, lr = train.Adam(ps, lr=torch.tensor(A.LR, device=dev), capturable=True), LR32
    betas = opt.defaults["betas"]
    assert betas == (0.9, 0.999)
    n_view = A.SIZES[VIEW]
    assert n_view >= 2 * A.CHUNK
    fence = hu.full((n_view + 2 * hu.GUARD + 4,))
    view = fence[hu.GUARD + 1: hu.GUARD + 1 + n_view]
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    count = [0] * len(ps)
    for step in range(3):
        before = []
        for i, p in enumerate(ps):
            st = opt.state.get(p, {})
            zeros = np.zeros(p.numel(), np.float32)
            before.append((p.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy() if st else zeros,
                           st["exp_avg_sq"].cpu().numpy().copy() if st else zeros))
        stepped = [i for i in range(len(ps)) if not (step == 1 and i == SKIPS)]
        for i, p in enumerate(ps):
            p.grad = None
        for i in stepped:
            if i == VIEW:
                view.copy_(torch.from_numpy(grads[step][i]))
                ps[i].grad = view
            else:
                ps[i].grad = torch.from_numpy(grads[step][i]).to(dev)
        opt.step()
        torch.cuda.synchronize()
        table = np.frombuffer(opt._nd_keep[0].cpu().numpy().tobytes(), dtype=np.dtype(L.AdamItem))
        assert len(table) == len(stepped) and table["g"][stepped.index(VIEW)] == view.data_ptr()
        assert list(table["vec4"]) == [int(i != VIEW) for i in stepped], "vec4 must be 0 for the unaligned gradient, 1 for the others"
        R3.only_nan_outside(fence.cpu(), (slice(hu.GUARD + 1, hu.GUARD + 1 + n_view),), "gradient view")
        assert np.array_equal(view.cpu().numpy().view(np.uint32), grads[step][VIEW].view(np.uint32)), "the gradient was written"
        for i, p in enumerate(ps):
            now = (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy())
            if i not in stepped:
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(now, before[i])), "a parameter without a gradient moved"
                continue
            count[i] += 1
            assert float(opt.state[p]["step"]) == count[i]
            args = (before[i][0], grads[step][i], before[i][1], before[i][2], count[i], lr, *betas, A.EPS, 0.0)
            judge(now, (A.step64(*args), A.step32(*args)), f"{form} step {step + 1} parameter {i} (n {p.numel()}, t {count[i]})")
    assert count[SKIPS] == 2 and count[VIEW] == 3


# ---------------------------------------------------------------------------------------------------------------- GPU: the F(4x4) weight packers
# (cin, cout, transposed) of the operator that is packed.  (8, 8) leaves most of the 64 x n grid idle; (24, 8) and (72, 40) are ragged in both channel
# counts; (512, 512) has 131072 lane slots for 64 x 256 threads: the strided loop makes eight trips.
PACK_ITEMS = [(8, 8, 0), (24, 8, 0), (72, 40, 1), (16, 64, 1), (512, 512, 0)]


def pack_weight(i, cin, cout, transposed):
    """The OIHW weight item i reads: (cout, cin, 3, 3), or for a transposed item the FORWARD layer's (cin, cout, 3, 3)."""
    from noisediff_amd import synth
    return synth.uniform(31, f"w4pack.{i}.{cin}.{cout}.{transposed}", (cin, cout, 3, 3) if transposed else (cout, cin, 3, 3), -0.2, 0.2)


def pack_single(ctx, w, cin, cout, transposed):
    """nd_pack_conv3x3_wino4_weight / _dgrad into a fenced buffer -> (the Guarded output, its host copy)."""
    from hiputil import Guarded, nan_like
    src, out = Guarded(w), nan_like((ctx.lib.nd_pack_conv3x3_wino4_weight_floats(cin, cout),))
    entry = "nd_pack_conv3x3_wino4_weight_dgrad" if transposed else "nd_pack_conv3x3_wino4_weight"
    L.call(entry, src.ptr, out.ptr, cin, cout, ctx.stream)
    ctx.sync()
    buf = out.host()
    R3.only_nan_outside(buf, out.region, entry)
    return out, buf


def pack_batch(ctx, specs, ws):
    import hiputil as hu
    srcs = [hu.Guarded(w) for w in ws]
    outs = [hu.nan_like((ctx.lib.nd_pack_conv3x3_wino4_weight_floats(cin, cout),)) for cin, cout, _ in specs]
    items = (L.PackItem * len(specs))()
    for it, s, o, (cin, cout, tr) in zip(items, srcs, outs, specs):
        it.w, it.packed, it.cin, it.cout, it.transposed = s.ptr, o.ptr, cin, cout, tr
    table = hu.dev(torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8))
    L.call("nd_pack_conv3x3_wino4_weights_batch", table.data_ptr(), len(specs), ctx.stream)
    ctx.sync()
    res = []
    for o, s, w in zip(outs, srcs, ws):
        buf = o.host()
        R3.only_nan_outside(buf, o.region, "nd_pack_conv3x3_wino4_weights_batch")
        assert torch.equal(s.tensor(), w), "the packer wrote to its source"
        res.append(o.tensor(buf))
    return res, table


@gpu
def test_the_batched_wino4_packer_equals_the_single_packers_bit_for_bit(ctx):
    ws = [pack_weight(i, *spec) for i, spec in enumerate(PACK_ITEMS)]
    singles = []
    for w, (cin, cout, tr) in zip(ws, PACK_ITEMS):
        out, buf = pack_single(ctx, w, cin, cout, tr)
        singles.append(out.tensor(buf))
    batch, table = pack_batch(ctx, PACK_ITEMS, ws)
    for spec, s, b in zip(PACK_ITEMS, singles, batch):
        assert not torch.isnan(b).any(), f"{spec}: the padding was not written"
        assert torch.equal(b.view(torch.int32), s.view(torch.int32)), f"{spec}: batch != single"
    for k in (1, 2):                                                  # n_items = 1: one grid row
        one, _ = pack_batch(ctx, PACK_ITEMS[k: k + 1], ws[k: k + 1])
        assert torch.equal(one[0].view(torch.int32), singles[k].view(torch.int32))
    for bad in ((table.data_ptr(), 0), (table.data_ptr(), 65536), (None, 1)):
        assert ctx.lib.nd_pack_conv3x3_wino4_weights_batch(*bad, ctx.stream) == -1
        assert "nd_pack_conv3x3_wino4_weights_batch" in ctx.lib.nd_last_error().decode()


@gpu
@pytest.mark.parametrize("transposed", [0, 1], ids=["forward", "dgrad"])
@pytest.mark.parametrize("cin,cout", [(24, 8), (72, 40), (64, 64)])
def test_packed_U_is_G_g_Gt_in_float64(ctx, cin, cout, transposed):
    """The packed buffer decoded by the header's layout against U = G g G^T in float64 with the exact rationals of G; the fp32 reference is the same
    product in fp32 torch.  Entries of padded channels are exactly 0.0."""
    w = pack_weight(9, cin, cout, transposed)
    out, buf = pack_single(ctx, w, cin, cout, transposed)
    U, pad = R3.wino4_unpack(out.tensor(buf), cin, cout)
    assert not pad.view(torch.int32).any(), "padded channels are not +0.0"
    g = w.transpose(0, 1).flip(2, 3).contiguous() if transposed else w          # the data gradient's operator: channel roles swapped, taps flipped
    derived(U, R3.wino4_U(g, torch.float64), R3.wino4_U(g, torch.float32), f"U {cin} -> {cout} {'dgrad' if transposed else 'forward'}")
