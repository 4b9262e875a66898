#!/usr/bin/env python3
"""The folded AttnBlock tails and the fast Downsample layers stand-alone against the launches they replace, run back to back (DESIGN 8.9's protocol: same box,
same process, alternating):

    python tools/attn_fold_bench.py [--dim 64] [--size 256] [--batch 16] [--reps 12]

Records the headline plan twice -- as shipped, and with engine.FOLD_ATTN / engine.DOWN_FAST off -- runs one whole step of each so that every buffer holds real
activations, then times the launches of each layer between two HIP events on the library stream (3 warm-up rounds, then --reps alternating rounds)."""
import argparse
import ctypes as C
import os
import statistics
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from noisediff_amd import NoiseDiffNet, synth  # noqa: E402
from noisediff_amd import _lib as L  # noqa: E402
from noisediff_amd import engine as E  # noqa: E402
from noisediff_amd.spec import noisediff_param_spec  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    net = NoiseDiffNet(SimpleNamespace(dim=a.dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
    net.load_state_dict(synth.make_state_dict(noisediff_param_spec(a.dim), 0), strict=True)
    net = net.to(dev).eval()
    eng = net.hip_engine(dev)
    B, H = a.batch, a.size
    cond = {k: (v if k == "iso_ratio_idx" else v.to(dev)) for k, v in synth.make_condition(B, H, seed=1).items()}
    x, t = torch.randn(B, 4, H, H, generator=torch.Generator().manual_seed(0)).to(dev), torch.full((B,), 500, dtype=torch.long)
    E.FOLD_ATTN = E.DOWN_FAST = True
    fast = eng.plan(B, H, H)
    E.FOLD_ATTN = E.DOWN_FAST = False
    plain = eng.plan(B, H, H, tag=1)
    for p in (fast, plain):
        p.set_condition(cond)
        p.forward(x, t)
    layer = lambda op: op[3].get("layer", "") if op[3] else ""
    # layer of the new launch -> layers of the launches it replaces
    pairs = {layer(op): (layer(op)[:-len(".tail_fold")] + ".ff.net.2", layer(op)[:-len(".tail_fold")] + ".proj_out")
             for op in fast.step_ops if layer(op).endswith(".tail_fold")}
    pairs.update({layer(op): (layer(op),) for op in fast.step_ops if op[2] == "nd_pointwise_downsample_nhwc_f32"})
    if not pairs:
        raise SystemExit("the plan records neither a folded AttnBlock tail nor a fast Downsample at these widths")
    st = eng.stream
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.call("nd_event_create", C.byref(e))

    def ops_of(plan, layers):
        got = [op for op in plan.step_ops if layer(op) in layers]
        if len(got) != len(layers):
            raise SystemExit(f"plan records {[layer(op) for op in got]} of {layers}")
        return got

    def timed(ops):
        L.call("nd_event_record", ev[0], st)
        for fn, args, name, _ in ops:
            L.check(fn(*args), name)
        L.call("nd_event_record", ev[1], st)
        L.call("nd_stream_sync", st)
        ms = C.c_float()
        L.call("nd_event_elapsed_ms", ev[0], ev[1], C.byref(ms))
        return ms.value * 1e3

    print(f"d={a.dim}, {B} x {H} x {H}; microseconds between two events around the launches, {a.reps} alternating rounds after 3 warm-up rounds")
    saved = 0.0
    for new, old in pairs.items():
        f_ops, u_ops = ops_of(fast, (new,)), ops_of(plain, old)
        for _ in range(3):
            timed(f_ops), timed(u_ops)
        tf, tu = [], []
        for _ in range(a.reps):
            tu.append(timed(u_ops))
            tf.append(timed(f_ops))
        m = f_ops[0][3]
        line = lambda v: f"median {statistics.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}"
        saved += statistics.median(tu) - statistics.median(tf)
        print(f"{new} ({m['cin']} -> {m['cout']}, {m['HW']} pixels):\n  before ({' + '.join(old)}): {line(tu)}\n  after: {line(tf)}\n"
              f"  faster in every round: {max(tf) < min(tu)}; median saving {statistics.median(tu) - statistics.median(tf):.1f} us")
    print(f"sum of the median savings: {saved:.1f} us per step")
    for e in ev:
        L.call("nd_event_destroy", e)


if __name__ == "__main__":
    main()
