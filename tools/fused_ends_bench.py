#!/usr/bin/env python3
"""Each fused end of the step stand-alone against the two launches it replaces, run back to back (DESIGN 8.9's protocol: same box, same process, alternating):

    python tools/fused_ends_bench.py [--dim 64] [--size 256] [--batch 16] [--reps 12]

Records the headline plan twice -- as shipped, and with engine.FOLD_FINAL / engine.SHOT_TAIL off -- runs one whole step of each so that every buffer holds
real activations, then times the launches of each end between two HIP events on the library stream (3 warm-up rounds, then --reps alternating rounds)."""
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

ENDS = {   # end -> (layer of the fused launch, layers of the launches it replaces)
    "shot-noise end": ("shot_time.tail+shot_mlp3", ("shot_time.tail", "shot_mlp3")),
    "trunk end": ("final_res_block.res_conv+final_conv", ("final_res_block.res_conv", "final_conv")),
}


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
    fused = eng.plan(B, H, H)
    E.FOLD_FINAL = E.SHOT_TAIL = False
    plain = eng.plan(B, H, H, tag=1)
    for p in (fused, plain):
        p.set_condition(cond)
        p.forward(x, t)
    st = eng.stream
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.call("nd_event_create", C.byref(e))

    def ops_of(plan, layers):
        got = [op for op in plan.step_ops if op[3] and op[3].get("layer") in layers]
        if len(got) != len(layers):
            raise SystemExit(f"plan records {[op[3]['layer'] for op in got]} of {layers}: this end is not fused at these widths")
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
    for end, (f_layer, u_layers) in ENDS.items():
        f_ops, u_ops = ops_of(fused, (f_layer,)), ops_of(plain, u_layers)
        for _ in range(3):
            timed(f_ops), timed(u_ops)
        tf, tu = [], []
        for _ in range(a.reps):
            tu.append(timed(u_ops))
            tf.append(timed(f_ops))
        line = lambda v: f"median {statistics.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}"
        print(f"{end}:\n  two launches ({' + '.join(u_layers)}): {line(tu)}\n  fused ({f_layer}): {line(tf)}\n"
              f"  fused faster in every round: {max(tf) < min(tu)}; median saving {statistics.median(tu) - statistics.median(tf):.1f} us")
    for e in ev:
        L.call("nd_event_destroy", e)


if __name__ == "__main__":
    main()
