"""train.EMA (ema.hip: the shadow-model update in one pass, decided on the device) and train.Adam with a learning rate held in device memory.

The reference is tests/ema_ref.py: ema_pytorch's rule restated in fp64 numpy (the package is compared where it is installed; it is not part of the
proof).  CPU: the surface, the plan for every step of the reference's schedule, a CPU module call by call, Adam's lr bookkeeping, the overlay.
GPU: the pass on the Adam test's awkward sizes plus the exact-chunk pair -- actions exact, weights within one fp32 ulp, skips and copies bit for bit,
lerps under util.derived -- the clamp at beta, load / deep copy, version counters and the packing caches, the tensor lr, and one whole captured
training iteration against its eager twin to the bit.

Lerps are judged on the whole shadow model as ONE vector (all tensors are O(1) and share one scale): util.derived takes its bound from the error of
the fp32 reference, and on a tensor of one or seven elements that error can be zero by luck, which would demand a correctly rounded result of a
formula that rounds four times."""
import copy
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

import ema_ref as R
from noisediff_amd import _lib as L, train
from util import derived

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
ENTRIES = ["nd_ema_chunk_elements", "nd_ema_update_f32", "nd_adam_step_capturable_lr_f32"]
REF_ARGS = dict(beta=0.995, update_after_step=500, update_every=20)           # models/trainer_diffusion.py:63-68
# the Adam test's set plus the exact-chunk pair; the 4097-element tensor is handled apart (an unaligned view on the shadow side, with guards)
SHAPES = [(1,), (7,), (3, 5, 3, 3), (8192,), (8193,), (64, 64, 3, 3), (20000,), (130, 257)]
GUARD = 3                                                                      # floats before and after the 4097 shadow elements (so: unaligned)
CALLS = 12


def one_ulp(x):
    return float(np.spacing(np.float32(abs(x))))


class Bag(nn.Module):
    """Parameters of given shapes (and one integer buffer, which no update may touch)."""

    def __init__(self, shapes, seed=3, guarded=False):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = nn.ParameterList([nn.Parameter(torch.randn(*s, generator=g)) for s in shapes])
        if guarded:
            big = torch.randn(4099, generator=g)
            self.odd = nn.Parameter(big[1:4098].clone())                       # a 4097-element clone of an unaligned view
        self.register_buffer("count", torch.tensor([5], dtype=torch.int64))


def online_values(model, call):
    """What the online tensors hold before update() number ``call``: fresh values, deterministic, made on the CPU."""
    g = torch.Generator().manual_seed(1000 + call)
    return {k: torch.randn(p.shape, generator=g) * (1.0 + 0.1 * call) for k, p in model.named_parameters()}


def set_online(model, values):
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(values[k].to(p.device))


def reference_run(model, calls, no_ema=(), **args):
    """The restatement over ``calls`` updates of ``model`` (a CPU module, not changed): per call (action, fp64 weight, {name: fp64 shadow},
    {name: torch CPU fp32 shadow, lerp_ with the restatement's weights})."""
    sh = R.Shadow({k: p.detach().numpy() for k, p in model.named_parameters()}, no_ema=no_ema, **args)
    r32 = {k: p.detach().clone() for k, p in model.named_parameters()}
    out = []
    for call in range(calls):
        vals = online_values(model, call)
        action, w = sh.update({k: v.numpy() for k, v in vals.items()})
        for k, v in vals.items():
            if action in (R.COPY, R.COPY_LERP) or (action == R.LERP and k in no_ema):
                r32[k] = v.clone()
            if action in (R.LERP, R.COPY_LERP) and k not in no_ema:
                r32[k].lerp_(v, R.weight32(w))
        out.append((action, w, {k: v.copy() for k, v in sh.t.items()}, {k: v.clone() for k, v in r32.items()}))
    return out


def flat(d, keys):
    return np.concatenate([np.asarray(torch.as_tensor(d[k]).detach().cpu().double()).reshape(-1) for k in keys])


def check_call(shadow, ref, online, what):
    """One call's shadow state (``shadow``: {name: tensor}) against the restatement's entry ``ref``."""
    action, _w, t64, t32 = ref
    keys = sorted(t64)
    if action in (R.COPY, R.COPY_LERP):
        for k in keys:
            assert torch.equal(shadow[k].cpu(), online[k]), (what, k)                  # a copy (and the no-op lerp after it): the same bits
            assert np.array_equal(shadow[k].cpu().double().numpy(), t64[k]), (what, k)
    elif action == R.LERP:
        derived(flat(shadow, keys), flat(t64, keys), flat(t32, keys), what)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_translation_unit_and_the_entry_points_exist():
    """Fails without the feature: ema.hip is built, the three entry points are declared, exported and bound, nd_ema_item's size is pinned."""
    import ctypes as C
    from noisediff_amd import build
    assert "ema" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ema.hip"))
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", header))
    lib = L.load()
    for name in ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(L.EmaItem) == 2 * 8 + 8 + 2 * 4                                 # nd_ema_item
    assert C.sizeof(L.AdamItem) == 4 * 8 + 8 + 2 * 4 + 2 * 4 + 8                    # nd_adam_item keeps its layout
    assert lib.nd_ema_chunk_elements() == 8192
    assert (train.EMA_SKIP, train.EMA_COPY, train.EMA_LERP, train.EMA_COPY_LERP) == (R.SKIP, R.COPY, R.LERP, R.COPY_LERP)


def test_the_plan_of_the_reference_schedule_follows_the_restatement():
    """beta 0.995, update_after_step 500, update_every 20, s = 0 ... 3400, through the plan function alone."""
    init_a = init_r = False
    seen = {}
    for s in range(3401):
        action, w = train.ema_plan(s, init_a, **REF_ARGS)
        ra, rw, init_r = R.plan(s, init_r, **REF_ARGS)
        init_a = init_a or action == train.EMA_COPY_LERP
        assert action == ra and init_a == init_r, s
        assert abs(w - R.weight32(rw)) <= one_ulp(rw), (s, w, rw)
        assert w == float(np.float32(w))                                             # rounded to fp32 once
        seen[s] = (action, w)
    for s in range(3401):
        if s % 20:
            assert seen[s] == (R.SKIP, 0.0), s
        elif s <= 500:
            assert seen[s] == (R.COPY, 0.0), s
        else:
            assert seen[s][0] == (R.COPY_LERP if s == 520 else R.LERP), s
    assert abs(seen[520][1] - 21.0 ** (-2.0 / 3.0)) <= one_ulp(21.0 ** (-2.0 / 3.0))      # decay 1 - 21^(-2/3): e = 20
    at_beta = float(np.float32(1.0 - 0.995))
    for s in (3340, 3360, 3380, 3400):                                                   # e = s - 500 >= 2828: the clamp, exactly
        assert seen[s][1] == at_beta, s
    assert seen[3320][1] > at_beta                                                       # e = 2820: not yet


class Three(nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = nn.Parameter(torch.randn(4, 3, generator=g))
        self.bias = nn.Parameter(torch.randn(4, generator=g))
        self.gain = nn.Parameter(torch.tensor(0.3))
        self.register_buffer("count", torch.tensor([5], dtype=torch.int64))

    def forward(self, x):
        return (x @ self.weight.t() + self.bias) * self.gain


def test_a_cpu_ema_follows_the_restatement_call_by_call():
    args = dict(beta=0.995, update_after_step=3, update_every=2)
    net = Three()
    refs = reference_run(net, CALLS, no_ema=("bias",), **args)
    assert [r[0] for r in refs] == [R.COPY, R.SKIP, R.COPY, R.SKIP, R.COPY_LERP, R.SKIP, R.LERP, R.SKIP, R.LERP, R.SKIP, R.LERP, R.SKIP]
    ema = train.EMA(net, param_or_buffer_names_no_ema=("bias",), **args)
    assert isinstance(ema, nn.Module) and ema.online_model is net and ema.ema_model is not net
    assert all(not p.requires_grad for p in ema.ema_model.parameters()) and all(p.requires_grad for p in net.parameters())
    assert ema.step.dtype == torch.int64 and ema.step.shape == (1,) and ema.initted.dtype == torch.bool and ema.initted.shape == (1,)
    assert list(ema.state_dict()) == ["initted", "step"] + [f"{m}.{k}" for m in ("online_model", "ema_model") for k in ("weight", "bias", "gain", "count")]
    initted = False
    for call, ref in enumerate(refs):
        vals = online_values(net, call)
        set_online(net, vals)
        net.count += 1                                                                 # the online integer buffer moves; the shadow's must not
        before = {k: p.clone() for k, p in ema.ema_model.named_parameters()}
        ema.update()
        action, w = ema.last_plan()
        assert action == ref[0] and abs(w - R.weight32(ref[1])) <= one_ulp(ref[1]), call
        initted = initted or action == R.COPY_LERP
        assert int(ema.step) == call + 1 and bool(ema.initted) == initted
        shadow = dict(ema.ema_model.named_parameters())
        if action == R.SKIP:
            assert all(torch.equal(shadow[k], before[k]) for k in shadow), call
        check_call(shadow, ref, vals, f"cpu call {call}")
        if action == R.LERP:
            assert torch.equal(shadow["bias"], vals["bias"])                           # named in param_or_buffer_names_no_ema: copied
            assert not torch.equal(shadow["weight"], vals["weight"])
    assert int(ema.ema_model.count) == 5 and int(net.count) == 5 + CALLS
    x = torch.ones(2, 3)
    assert torch.equal(ema(x), ema.ema_model(x))
    assert ema.get_current_decay() == pytest.approx(R.decay(CALLS - 1, **{k: v for k, v in args.items() if k != "update_every"}), rel=1e-12)
    ema.copy_params_from_model_to_ema()
    assert all(torch.equal(a, b) for a, b in zip(ema.ema_model.parameters(), net.parameters()))
    for kw in ({"use_foreach": True}, {"update_model_with_ema_every": 10}, {"allow_different_devices": False}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            train.EMA(Three(), **kw)
    half = Three()
    half.bias.data = half.bias.data.half()
    with pytest.raises(NotImplementedError):
        train.EMA(half).update()
    # deep copies and pickles carry their own counters and none of the tables
    ema._nd_tables[("stale",)] = ()
    twin = copy.deepcopy(ema)
    assert twin._nd_tables == {} and twin._nd_captured == [] and int(twin.step) == CALLS and twin.step is not ema.step
    twin.update()
    assert int(twin.step) == CALLS + 1 and int(ema.step) == CALLS


def test_against_the_package_where_it_is_installed():
    """Not part of the proof (the package computes its decay in fp32 tensor arithmetic: rel 1e-6)."""
    pkg = pytest.importorskip("ema_pytorch")
    if pkg.EMA is train.EMA:
        pytest.skip("ema_pytorch is this project's overlay")
    args = dict(beta=0.995, update_after_step=3, update_every=2)
    nets = Three(), Three()
    ours, theirs = train.EMA(nets[0], **args), pkg.EMA(nets[1], **args)
    for call in range(CALLS):
        for net in nets:
            set_online(net, online_values(net, call))
        ours.update()
        theirs.update()
        assert int(ours.step) == int(theirs.step)
        for a, b in zip(ours.ema_model.parameters(), theirs.ema_model.parameters()):
            assert a.detach().numpy() == pytest.approx(b.detach().numpy(), rel=1e-6)


def test_adam_set_lr_and_the_captured_lr_bookkeeping():
    lr = torch.tensor(2e-3)
    opt = train.Adam([nn.Parameter(torch.zeros(4))], lr=lr, capturable=True)
    group = opt.param_groups[0]
    assert group["lr"] is lr
    opt.set_lr(1e-3)
    assert group["lr"] is lr and float(lr) == float(np.float32(1e-3))                  # filled in place
    opt.check_captured_lr()                                                            # nothing captured: nothing to refuse
    opt._nd_captured_lr[id(group)] = lr                                                # what a captured step with a tensor lr records
    opt.set_lr(5e-4)
    opt.check_captured_lr()                                                            # the same tensor, whatever its value
    group["lr"] = 5e-4
    with pytest.raises(RuntimeError, match="replaced"):
        opt.check_captured_lr()
    group["lr"] = lr.clone()
    with pytest.raises(RuntimeError, match="replaced"):
        opt.check_captured_lr()
    group["lr"] = lr
    opt.check_captured_lr()
    plain = train.Adam([nn.Parameter(torch.zeros(4)), nn.Parameter(torch.ones(2))], lr=2e-3, capturable=True)
    plain.add_param_group({"params": [nn.Parameter(torch.ones(3))], "lr": 4e-3})
    plain.set_lr(1e-3)
    plain.set_lr(3e-3, group=1)
    assert [g["lr"] for g in plain.param_groups] == [1e-3, 3e-3] and all(isinstance(g["lr"], float) for g in plain.param_groups)
    plain._nd_captured_lr[id(plain.param_groups[0])] = 1e-3                            # a captured step with a float lr: the launch argument
    plain.check_captured_lr()
    plain.set_lr(2e-3)
    with pytest.raises(RuntimeError, match="recorded with lr=0.001"):
        plain.check_captured_lr()
    plain.param_groups[0]["lr"] = torch.tensor(1e-3)                                   # a tensor where the capture saw a float
    with pytest.raises(RuntimeError):
        plain.check_captured_lr()


def test_the_overlay_provides_ema_pytorch_only_where_nothing_else_does():
    from noisediff_amd import dropin
    finder = dropin.OverlayFinder()
    had = sys.modules.pop("ema_pytorch", None)
    installed = any(f is not finder and hasattr(f, "find_spec") and f.find_spec("ema_pytorch", None) is not None for f in sys.meta_path)
    sys.meta_path.insert(0, finder)
    try:
        if installed:
            assert finder.find_spec("ema_pytorch") is None                             # an installed package wins
        else:
            mod = importlib.import_module("ema_pytorch")
            assert mod.EMA is train.EMA and mod.__spec__.origin == "noisediff_amd.dropin"
            del sys.modules["ema_pytorch"]
        stub = types.ModuleType("ema_pytorch")
        stub.EMA = object
        sys.modules["ema_pytorch"] = stub
        assert importlib.import_module("ema_pytorch") is stub                          # so does whatever is already in sys.modules
        assert finder.find_spec("models.not_ours") is None
    finally:
        sys.meta_path.remove(finder)
        sys.modules.pop("ema_pytorch", None)
        if had is not None:
            sys.modules["ema_pytorch"] = had


# ---------------------------------------------------------------------------------------------------------------- GPU
ARGS32 = dict(beta=0.995, update_after_step=3, update_every=2)


@pytest.fixture(scope="module")
def bag_refs():
    return reference_run(Bag(SHAPES, guarded=True), CALLS, **ARGS32)


def gpu_bag():
    """The online Bag on the GPU and a shadow whose 4097-element tensor is an unaligned view between guard floats."""
    net = Bag(SHAPES, guarded=True).to(DEV)
    shadow = copy.deepcopy(net)
    fence = torch.full((4097 + 2 * GUARD,), 777.0, device=DEV)
    fence[GUARD:GUARD + 4097] = net.odd.detach()
    shadow.odd.data = fence[GUARD:GUARD + 4097]
    assert shadow.odd.data_ptr() % 16 != 0 and net.odd.data_ptr() % 16 == 0
    return net, shadow, fence


def run_bag(calls=range(CALLS), ema=None, net=None):
    """update() number ``call`` for each of ``calls`` on the GPU bag: per call (plan, shadow tensors on the CPU, counters)."""
    if ema is None:
        net, shadow, fence = gpu_bag()
        ema = train.EMA(net, ema_model=shadow, **ARGS32).to(DEV)
        ema.fence = fence
    out = []
    for call in calls:
        set_online(net, online_values(net, call))
        versions = [p._version for p in ema.ema_model.parameters()]
        ema.update()
        assert all(p._version > v for p, v in zip(ema.ema_model.parameters(), versions)), call       # every update() tells the packing caches
        out.append((ema.last_plan(), {k: p.detach().cpu() for k, p in ema.ema_model.named_parameters()}, int(ema.step), bool(ema.initted)))
    return ema, out


@pytest.mark.gpu
def test_twelve_updates_on_the_gpu_follow_the_restatement(bag_refs):
    ema, got = run_bag()
    cpu_model = Bag(SHAPES, guarded=True)
    prev = {k: p.detach().clone() for k, p in cpu_model.named_parameters()}
    initted = False
    for call, (ref, ((action, w), shadow, step, flag)) in enumerate(zip(bag_refs, got)):
        assert action == ref[0], call                                                   # the device's decision: exactly the restatement's
        assert abs(w - R.weight32(ref[1])) <= one_ulp(ref[1]), (call, w, ref[1])         # fp64 pow on the device against numpy's: one fp32 ulp
        initted = initted or action == R.COPY_LERP
        assert step == call + 1 and flag == initted
        if action == R.SKIP:
            assert all(torch.equal(shadow[k], prev[k]) for k in shadow), call            # a skipped call leaves every bit
        check_call(shadow, ref, online_values(cpu_model, call), f"gpu call {call}")
        prev = shadow
    assert [g[0][0] for g in got].count(R.LERP) == 3
    assert int(ema.ema_model.count) == 5                                                # integer buffers are not the pass's
    fence = ema.fence.cpu()
    assert bool((fence[:GUARD] == 777.0).all()) and bool((fence[GUARD + 4097:] == 777.0).all())
    assert torch.equal(fence[GUARD:GUARD + 4097], got[-1][1]["odd"])
    _, again = run_bag()
    for a, b in zip(got, again):                                                        # no reductions, no atomics: the same bits
        assert a[0] == b[0] and a[2:] == b[2:] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.gpu
def test_the_decay_is_clamped_at_beta():
    net = Bag(SHAPES[:5]).to(DEV)
    ema = train.EMA(net, **REF_ARGS).to(DEV)
    ema.step.fill_(3340)
    ema.initted.fill_(True)
    before = {k: p.detach().cpu() for k, p in ema.ema_model.named_parameters()}
    vals = online_values(net, 0)
    set_online(net, vals)
    ema.update()
    w = float(np.float32(1.0 - 0.995))
    assert ema.last_plan() == (R.LERP, w) and int(ema.step) == 3341
    assert ema.get_current_decay() == 0.995
    keys = sorted(before)
    t64 = {k: R.lerp(before[k].numpy(), vals[k].numpy(), w) for k in keys}
    t32 = {k: before[k].clone().lerp_(vals[k], w) for k in keys}
    derived(flat(dict(ema.ema_model.named_parameters()), keys), flat(t64, keys), flat(t32, keys), "lerp at the clamp")


@pytest.mark.gpu
def test_a_loaded_state_and_a_deep_copy_continue_to_the_bit():
    _, whole = run_bag()
    half = CALLS // 2
    ema, _ = run_bag(range(half))
    assert bool(ema.initted)                                                            # (the flag is part of what must travel)
    state = copy.deepcopy(ema.state_dict())
    net2 = Bag(SHAPES, seed=99, guarded=True).to(DEV)
    loaded = train.EMA(net2, **ARGS32).to(DEV)
    loaded.load_state_dict(state)
    twin = copy.deepcopy(ema)
    assert twin._nd_tables == {} and twin.step is not ema.step
    for other, model in ((loaded, net2), (twin, twin.online_model)):
        _, rest = run_bag(range(half, CALLS), ema=other, net=model)
        for a, b in zip(whole[half:], rest):
            assert a[0] == b[0] and a[2:] == b[2:] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert int(ema.step) == half                                                        # the copy counted for itself


@pytest.mark.gpu
def test_a_forward_of_the_shadow_model_sees_every_update():
    """The packing caches compare version counters: update() bumps the shadow's, so no invalidate_packs() is needed."""
    from noisediff_amd._host import conv3x3_kind
    assert conv3x3_kind(2, 32, 32, 32, 64, 32, 0, 32) == "wino4"                        # wide enough for F(4x4): its weights are packed and cached

    def make():
        torch.manual_seed(1)
        net = nn.Sequential(nn.Conv2d(32, 64, 3, padding=1), nn.Conv2d(64, 8, 1)).to(DEV)
        train.accelerate(net)
        return net
    net = make()
    ema = train.EMA(net, beta=0.9, update_after_step=0, update_every=1).to(DEV)
    x = torch.randn(2, 32, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        y0 = ema(x).clone()                                                             # the shadow's weights are packed and cached now
        for call in range(3):                                                           # copy, copy + lerp, lerp
            versions = [p._version for p in ema.ema_model.parameters()]
            for p in net.parameters():
                p.mul_(1.25).add_(0.01)
            ema.update()
            assert all(p._version > v for p, v in zip(ema.ema_model.parameters(), versions)), call
            y = ema(x)
            fresh = make()
            fresh.load_state_dict(ema.ema_model.state_dict())
            assert torch.equal(y, fresh(x)), call
            assert not torch.equal(y, y0)
    assert [ema.last_plan()[0], int(ema.step), bool(ema.initted)] == [R.LERP, 3, True]


def adam_params():
    torch.manual_seed(3)
    ps = [nn.Parameter(torch.randn(*s, device=DEV)) for s in SHAPES]
    big = torch.randn(4099, device=DEV)
    ps.append(nn.Parameter(big[1:4098].clone()))
    return ps


def adam_grads(ps, step):
    g = torch.Generator(device="cpu").manual_seed(100 + step)
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * (0.5 + step)).to(DEV)


@pytest.mark.gpu
def test_adam_reads_a_tensor_lr_on_the_device():
    runs = {}
    for kind in ("float", "tensor"):
        ps = adam_params()
        lr = 3e-3 if kind == "float" else torch.tensor(3e-3, device=DEV)
        opt = train.Adam(ps, lr=lr, betas=(0.9, 0.99), weight_decay=0.01, capturable=True)
        snaps = []
        for step in range(6):
            if step == 4:
                opt.set_lr(1e-3)
                assert (opt.param_groups[0]["lr"] is lr) == (kind == "tensor")
            adam_grads(ps, step)
            opt.step()
            snaps.append([p.detach().cpu() for p in ps] + [opt.state[p][k].cpu() for p in ps for k in ("exp_avg", "exp_avg_sq", "step")])
        runs[kind] = snaps
    for step, (a, b) in enumerate(zip(runs["float"], runs["tensor"])):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), step                       # the same bits, before and after set_lr
    assert not torch.equal(runs["tensor"][3][0], runs["tensor"][5][0])
    # capturable=False: a tensor lr is read on the host, as torch does
    ps = adam_params()
    host = train.Adam(ps, lr=torch.tensor(3e-3), betas=(0.9, 0.99), weight_decay=0.01)
    ref = train.Adam(adam_params(), lr=float(np.float32(3e-3)), betas=(0.9, 0.99), weight_decay=0.01)     # (the value the tensor holds)
    for opt in (host, ref):
        adam_grads(opt.param_groups[0]["params"], 0)
        opt.step()
    assert all(torch.equal(a, b) for a, b in zip(host.param_groups[0]["params"], ref.param_groups[0]["params"]))
    with pytest.raises(NotImplementedError):                                            # capturable: the kernel reads it, so it must be there
        bad = train.Adam(ps, lr=torch.tensor(3e-3), capturable=True)
        bad.step()


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load()
    ps = [torch.zeros(16, device=DEV) for _ in range(4)]
    items = np.zeros(1, dtype=np.dtype(L.EmaItem))
    items["ema"], items["src"], items["n"], items["vec4"] = ps[0].data_ptr(), ps[1].data_ptr(), 16, 1
    table = torch.from_numpy(items.view(np.uint8)).to(DEV)
    chunks = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    step = torch.tensor([4], dtype=torch.int64, device=DEV)
    flag = torch.tensor([False], device=DEV)
    plan = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    st = None
    good = [table.data_ptr(), 1, chunks.data_ptr(), 1, step.data_ptr(), flag.data_ptr(), plan.data_ptr(), 0.995, 3, 2, 1.0, 2.0 / 3.0, 0.0, st]
    bad = {0: None, 1: 0, 2: None, 3: 0, 4: None, 5: None, 6: None}
    cases = [(i, v) for i, v in bad.items()] + [(1, -1), (3, -2), (7, -0.01), (7, 1.01), (7, float("nan")), (9, 0), (9, -3), (10, 0.0), (10, -1.0)]
    for i, v in cases:
        args = list(good)
        args[i] = v
        assert lib.nd_ema_update_f32(*args) == -1, (i, v)                               # ND_E_BADARG
        with pytest.raises(L.HipError):
            L.call("nd_ema_update_f32", *args)
    torch.cuda.synchronize()
    assert int(step) == 4 and not bool(flag) and plan.tolist() == [-7, -7] and float(ps[0].sum()) == 0.0      # nothing ran
    # the learning rate of the device-lr Adam step
    adam = np.zeros(1, dtype=np.dtype(L.AdamItem))
    cnt = torch.zeros((), device=DEV)
    adam["p"], adam["g"], adam["m"], adam["v"], adam["n"], adam["step"] = (*[p.data_ptr() for p in ps], 16, cnt.data_ptr())
    atable = torch.from_numpy(adam.view(np.uint8)).to(DEV)
    assert lib.nd_adam_step_capturable_lr_f32(atable.data_ptr(), 1, chunks.data_ptr(), 1, None, 0.9, 0.99, 1e-8, 0.0, st) == -1
    with pytest.raises(L.HipError):
        L.call("nd_adam_step_capturable_lr_f32", atable.data_ptr(), 1, chunks.data_ptr(), 1, None, 0.9, 0.99, 1e-8, 0.0, st)
    torch.cuda.synchronize()
    assert float(cnt) == 0.0                                                            # the counter launch did not run either


T = 1000


class PlugNet(nn.Module):
    """One 1x1 convolution with the reference's plug-in surface: three parameters (weight, bias, a gain on the timestep)."""
    channels = out_dim = 4
    self_condition = False
    random_or_learned_sinusoidal_cond = False

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.weight = nn.Parameter(torch.randn(4, 4, 1, 1, generator=g) * 0.5)
        self.bias = nn.Parameter(torch.randn(4, generator=g) * 0.1)
        self.tgain = nn.Parameter(torch.tensor(0.3))

    def forward(self, x, time, condition):
        # the 1x1 convolution as a broadcast product and a sum: its backward is ATen's tree reductions, which repeat to the bit.  (F.conv2d's weight
        # gradient on MIOpen does not: measured here, three identical eager runs differ by 3e-8 in it, so no bitwise comparison can go through it.)
        y = (x[:, None] * self.weight[None, :, :, 0, 0, None, None]).sum(2) + self.bias[None, :, None, None]
        return y * (1 + self.tgain * (time.to(x.dtype) / T))[:, None, None, None]


def iteration_setup(img):
    from noisediff_amd import GaussianDiffusion
    net = PlugNet()
    gd = GaussianDiffusion(net, image_size=16, timesteps=T, beta_schedule="sigmoid2", objective="pred_v").to(DEV).use_device_rng(7)
    opt = train.Adam(net.parameters(), lr=torch.tensor(1e-2, device=DEV), capturable=True)
    ema = train.EMA(net, **ARGS32).to(DEV)

    def one():
        opt.zero_grad(set_to_none=True)
        loss = gd(img, None)
        loss.backward()
        opt.step()
        ema.update()

    def state():
        torch.cuda.synchronize()
        out = [p.detach().cpu().clone() for p in net.parameters()] + [p.detach().cpu().clone() for p in ema.ema_model.parameters()]
        out += [ema.step.cpu().clone(), ema.initted.cpu().clone()]
        return out + [opt.state[p][k].cpu().clone() for p in net.parameters() for k in ("exp_avg", "exp_avg_sq", "step")]
    return net, gd, opt, ema, one, state


@pytest.mark.gpu
def test_one_whole_training_iteration_replays_as_a_captured_graph():
    """{gd(img), backward, opt.step(), ema.update()} captured once after one eager step and replayed six times, the learning rate changed between
    replays 3 and 4 through set_lr: the online and the shadow parameters, the counters and the Adam state equal the eager run of the same seven
    steps, to the bit.  Without the feature the lr of a captured step cannot move and the shadow update cannot be captured."""
    from noisediff_amd import synth
    img = synth.uniform(8, "ema.cap.img", (2, 4, 16, 16), -1.0, 1.0).to(DEV)
    side = torch.cuda.Stream()
    *_, opt, ema, one, state = iteration_setup(img)
    eager = []
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for step in range(7):
            if step == 4:
                opt.set_lr(3e-3)
            one()
            eager.append(state())
    torch.cuda.current_stream().wait_stream(side)
    assert int(ema.step) == 7 and bool(ema.initted) and ema.last_plan()[0] == R.LERP     # 3 / 2: copy, skip, copy, skip, copy + lerp, skip, lerp
    assert not all(torch.equal(a, b) for a, b in zip(eager[6][:3], eager[6][3:6]))       # the shadow lags the online model

    _net, _gd, opt, ema, one, state = iteration_setup(img)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(state(), eager[0]))
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss = _gd(img, None)
        loss.backward()
        opt.step()
        ema.update()
    assert all(torch.equal(a, b) for a, b in zip(state(), eager[0]))                     # capturing ran nothing
    lr = opt.param_groups[0]["lr"]
    for replay in range(1, 7):
        if replay == 4:
            opt.set_lr(3e-3)
        opt.check_captured_lr()
        graph.replay()
        got = state()
        assert len(got) == len(eager[replay]) and all(torch.equal(a, b) for a, b in zip(got, eager[replay])), replay
    assert opt.param_groups[0]["lr"] is lr and float(lr) == float(np.float32(3e-3))
    opt.param_groups[0]["lr"] = 1e-3
    with pytest.raises(RuntimeError):
        opt.check_captured_lr()
