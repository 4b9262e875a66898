#!/usr/bin/env python3
"""The physics-based noise launch (nd_raw_physics_noise_f32, noisediff_amd/physics_noise.py) next to the Poisson-Gaussian launch it extends.

    python tools/physics_noise_bench.py [--reps 200] [--out out/physics_noise_bench.txt]

B = 4 crops of 256 x 256 from a SID-size frame (1424 x 2128 packed), ISO 1600 and 25600 rows of the calibration fixture, ratio 250 and 300:
``PhysicsNoiseBatchBuilder.launch`` with Gaussian and with Tukey-lambda read noise and ``PoissonGaussianBatchBuilder.launch`` at the same gains
into persistent outputs, the three alternating, one pair of HIP events per launch; median and 10th-90th percentile over the rounds."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from noisediff_amd import io, physics_noise as pn, raw, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=os.path.join(REPO, "out", "physics_noise_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
H, W, C, B = io.PACKED_H, io.PACKED_W, 256, 4

with open(os.path.join(REPO, "tests", "golden", "physics_params.json")) as f:
    table = {int(k): v for k, v in json.load(f)["rows"].items()}
frames = raw.frames_on_device(np.floor(synth.uniform(2, "bench.physics.long", (1, 2 * H, 2 * W), 400.0, 16384.0).numpy()).astype(np.uint16), dev)
shape = tuple(frames.shape)
isos, ratio = [1600, 25600, 1600, 25600], [250, 300, 250, 300]
xy = [(0, 0), (1001, 513), (640, 1100), (1872, 1168)]
model = pn.CameraNoiseModel(table)
pb, gb = pn.PhysicsNoiseBatchBuilder(C), raw.PoissonGaussianBatchBuilder(C)
K = [table[i]["Kmax"] for i in isos]
blocks = {kind: pb.update(pb.capture_inputs(B, dev), shape, [0] * B, xy, ratio, model.draw(isos, seed=3, read=kind), seed=7) for kind in ("gaussian", "tukey")}
pg_block = gb.update(gb.capture_inputs(B, dev), shape, [0] * B, xy, ratio, K, [table[i]["sigGs"] ** 2 for i in isos], seed=7)
noisy, clean = (torch.empty(B, 4, C, C, device=dev) for _ in range(2))
forms = {"physics, Gaussian read": lambda: pb.launch(blocks["gaussian"], frames, noisy, clean),
         "physics, Tukey-lambda read": lambda: pb.launch(blocks["tukey"], frames, noisy, clean),
         "Poisson-Gaussian": lambda: gb.launch(pg_block, frames, noisy, clean)}
for fn in forms.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize(dev)
times = {name: [] for name in forms}
for _ in range(a.reps):
    for name, fn in forms.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3)
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; packed frame {H} x {W}, B = {B} crops of {C}, ISO {isos}, ratio {ratio}",
         f"{a.reps} rounds after 5 warm-up launches, the forms alternating, one pair of HIP events per launch; times in us"]
for name, t in times.items():
    t = np.array(t)
    lines.append(f"  {name:>28}: median {float(np.median(t)):8.1f}   p10 {np.percentile(t, 10):8.1f}   p90 {np.percentile(t, 90):8.1f}")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
