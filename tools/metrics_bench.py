#!/usr/bin/env python3
"""Scoring kernels (csrc/quality.hip) on the SID frame and on a batch of training patches: µs per call from HIP events, GB/s against the
8 TB/s spec and the 6.3 TB/s achievable, and the float64 numpy restatement (tests/metrics_ref.py) on the same frame for contrast.

    python tools/metrics_bench.py [--reps 50] [--out out/metrics_bench.txt]

Bytes are the algorithmic floor: est and target read once (2 x 4 B per element); the halo re-reads (L2) and the few-KB partials are not
counted.  The timed call is nd_image_quality_f32 (tile kernel + finalize); 'fused' adds the illumination scale (two more launches and one
more read of est and source) and reads k inside the tile kernel."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from noisediff_amd import io, metrics, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(REPO, "out", "metrics_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
SPEC, ACHIEVABLE = 8.0e12, 6.3e12
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} timed calls after 5 warm-up calls"]


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / a.reps


for shape in ((1, 4, io.PACKED_H, io.PACKED_W), (16, 4, 256, 256)):
    x = synth.uniform(1, "bench.x", shape, -0.1, 1.1).to(dev)
    y = synth.uniform(1, "bench.y", shape, 0.0, 1.0).to(dev)
    nbytes = 2 * 4 * x.numel()
    for name, fn in (("quality", lambda: metrics.quality(x, y)), ("quality fused", lambda: metrics.quality(x, y, illum_source=y)),
                     ("IlluminanceCorrect", lambda: metrics.IlluminanceCorrect()(x, y))):
        us = timed(fn)
        gbs = nbytes / (us * 1e-6) / 1e9
        lines.append(f"{str(shape):>24} {name:>18}: {us:9.1f} us  {gbs:7.0f} GB/s  ({100 * gbs * 1e9 / SPEC:4.1f} % of 8 TB/s spec, "
                     f"{100 * gbs * 1e9 / ACHIEVABLE:4.1f} % of 6.3 TB/s achievable; floor {nbytes / ACHIEVABLE * 1e6:.1f} us)")
        print(lines[-1], flush=True)

import metrics_ref as R  # noqa: E402
shape = (1, 4, io.PACKED_H, io.PACKED_W)
x = synth.uniform(1, "bench.x", shape, -0.1, 1.1)
y = synth.uniform(1, "bench.y", shape, 0.0, 1.0)
t = time.perf_counter()
ref_s, ref_p = R.ssim(x[0].numpy(), y[0].numpy()), R.psnr(x[0].numpy(), y[0].numpy())
dt = time.perf_counter() - t
r = metrics.quality(x.to(dev), y.to(dev))
got_s, got_p = float(r["SSIM"][0]), float(r["PSNR"][0])
lines.append(f"float64 numpy restatement on {shape}: {dt * 1e3:.0f} ms on the host (one thread for the box filters); "
             f"|dSSIM| {abs(got_s - ref_s):.1e}, |dPSNR| {abs(got_p - ref_p):.1e} dB")
print(lines[-1], flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
