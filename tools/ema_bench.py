#!/usr/bin/env python3
"""train.EMA.update() (ema.hip: one pass over all tensors, decided on the device) on the parameters of TrainableNoiseDiffNet(dim=64): a lerp call and a
skipped call against the per-tensor ``lerp_`` loop of ema_pytorch's rule (and torch._foreach_lerp_, the package's use_foreach form).  Device time of
each call between one event pair (an eager call includes what the device waits for the host; the captured rows are the pass alone); median and
p10-p90 of ROUNDS (100) calls after WARMUP (10).  The pass moves 12 bytes per element (read ema, read src, write ema): the achieved rate is printed
next to the rows that move them.  env DIM=64."""
import os, sys
sys.path.insert(0, os.environ.get("ND_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from types import SimpleNamespace
from noisediff_amd import TrainableNoiseDiffNet
from noisediff_amd.train import EMA

dev = torch.device("cuda", 0)
ROUNDS, WARMUP = int(os.environ.get("ROUNDS", "100")), int(os.environ.get("WARMUP", "10"))
net = TrainableNoiseDiffNet(SimpleNamespace(dim=int(os.environ.get("DIM", "64")))).to(dev)


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.percentile(ms, [50, 10, 90])


lerp = EMA(net, beta=0.995, update_after_step=0, update_every=1).to(dev)          # from the third call on every call is a lerp
skip = EMA(net, beta=0.995, update_after_step=0, update_every=10 ** 9).to(dev)    # after the first call every call is skipped
pairs = [(e, s) for _, e, s in lerp._nd_pairs()]
n = sum(e.numel() for e, _ in pairs)
w = float(np.float32(1.0 - 0.995))
emas, srcs = [e for e, _ in pairs], [s for _, s in pairs]


def loop():
    for e, s in pairs:
        e.data.lerp_(s.data, w)


def captured(ema):
    """update() as a one-node-pair graph: the device time of the pass without the host side of the call."""
    ema.update()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ema.update()
    return g


g_lerp, g_skip = captured(lerp), captured(skip)
rows = [("train.EMA.update(), lerp", timed(lerp.update)), ("train.EMA.update(), skipped", timed(skip.update)),
        ("captured update, lerp", timed(g_lerp.replay)), ("captured update, skipped", timed(g_skip.replay)),
        ("per-tensor lerp_ loop", timed(loop)), ("torch._foreach_lerp_", timed(lambda: torch._foreach_lerp_(emas, srcs, w)))]
assert lerp.last_plan()[0] == 2 and skip.last_plan()[0] == 0
print(f"{len(pairs)} tensors, {n} elements, {12 * n / 1e6:.1f} MB per pass; device ms per call: median (p10 - p90) of {ROUNDS}", flush=True)
for name, (p50, p10, p90) in rows:
    rate = "" if "skipped" in name else f"   {12 * n / (p50 * 1e-3) / 1e12:6.2f} TB/s of 12 B/element"
    print(f"{name:30s} {p50:8.4f} ({p10:.4f} - {p90:.4f}) ms{rate}", flush=True)
