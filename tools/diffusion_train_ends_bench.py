#!/usr/bin/env python3
"""The two ends of a diffusion training step -- everything of ``GaussianDiffusion.forward`` / ``p_losses`` but the network -- as the PyTorch
expressions and as the HIP launches behind ``use_device_rng`` (nd_diffusion_noising_f32, nd_diffusion_loss_f32, nd_diffusion_loss_backward_f32,
nd_diffusion_train_advance), forward and backward, on an identity stand-in for the model.

    python tools/diffusion_train_ends_bench.py [--reps 100] [--out out/diffusion_train_ends_bench.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/diffusion_train_ends_bench.py --count torch|hip
    python tools/diffusion_train_ends_bench.py --summarise torch=STATS.csv hip=STATS.csv [--out ...]       (appends the launch counts)

Timing: B = 4 at 256 x 256 and B = 8 at 128 x 128, pred_v; the two forms alternate, 100 rounds after 5 warm-up rounds, one pair of HIP events per
call; median and the 10th-90th percentile.  Two clocks per form: the eager call (host side included: the stream waits for the launches) and the same
call captured as one graph and replayed (the device side alone, what a captured training step pays).
--count FORM: ten calls of one form and nothing else, for a kernel trace: launches per call = kernel dispatches / 10."""
import argparse
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ND_PKG_ROOT") or REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=os.path.join(REPO, "out", "diffusion_train_ends_bench.txt"))
ap.add_argument("--count", choices=["torch", "hip"])
ap.add_argument("--summarise", nargs="+", metavar="FORM=CSV")
a = ap.parse_args()
COUNT_CALLS = 10

if a.summarise:
    lines = [f"kernels launched per call (rocprofv3 --kernel-trace --stats, {COUNT_CALLS} calls of one form per run, B=4 256x256, no counters):"]
    for item in a.summarise:
        form, path = item.split("=", 1)
        with open(path) as f:
            rows = sorted(((int(r["Calls"]), r["Name"]) for r in csv.DictReader(f)), reverse=True)
        total = sum(c for c, _ in rows)
        lines.append(f"  {form}: {total} dispatches in {COUNT_CALLS} calls = {total / COUNT_CALLS:.1f} per call")
        lines += [f"    {c / COUNT_CALLS:5.1f}  {name[:150]}" for c, name in rows]
    print("\n".join(lines), flush=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

import numpy as np
import torch
from torch import nn

from noisediff_amd import GaussianDiffusion, synth

dev = torch.device("cuda", 0)


class Identity(nn.Module):
    """The model's stand-in: hands x_t back as a leaf that wants a gradient, so backward() runs the loss's backward and nothing else."""
    channels = out_dim = 4
    self_condition = False
    random_or_learned_sinusoidal_cond = False

    def forward(self, x, time, condition):
        return x.requires_grad_()


def forms(B, S):
    img = synth.uniform(7, "img", (B, 4, S, S), -1.0, 1.0).to(dev)
    out = []
    for name, seed in (("PyTorch", None), ("HIP", 1)):
        gd = GaussianDiffusion(Identity(), image_size=S, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(dev).use_device_rng(seed)

        def call(gd=gd):
            loss = gd(img, None)
            loss.backward()
            return loss
        out.append((name, call))
    return out


if a.count:
    fn = dict(forms(4, 256))[{"torch": "PyTorch", "hip": "HIP"}[a.count]]
    for _ in range(COUNT_CALLS):
        fn()
    torch.cuda.synchronize(dev)
    sys.exit(0)


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms alternating, one pair of "
         f"HIP events per call; times in us; the ends alone (forward + backward of everything but the network, identity stand-in), pred_v"]
for B, S in ((4, 256), (8, 128)):
    eager = forms(B, S)
    for clock, fs in (("eager call", eager), ("one graph, replayed", [(n, graphed(f)) for n, f in eager])):
        for _ in range(5):
            for _, fn in fs:
                fn()
        torch.cuda.synchronize(dev)
        times = {n: [] for n, _ in fs}
        for _ in range(a.reps):
            for n, fn in fs:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[n].append(t0.elapsed_time(t1) * 1e3)
        lines.append(f"B={B} {S}x{S}, {clock}:")
        med = {}
        for n, _ in fs:
            t = np.array(times[n])
            med[n] = float(np.median(t))
            lines.append(f"  {n:>8}: median {med[n]:9.1f}   p10 {np.percentile(t, 10):9.1f}   p90 {np.percentile(t, 90):9.1f}")
        lines.append(f"  PyTorch - HIP = {med['PyTorch'] - med['HIP']:.1f} us ({med['PyTorch'] / med['HIP']:.1f}x)")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
