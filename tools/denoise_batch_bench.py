#!/usr/bin/env python3
"""The denoiser's training batch (csrc/denoise_batch.hip) at the shipped training command's shape -- B = 4, 256 x 256 crops of 512 x 512 patches,
dark shading and shot-noise augmentation on -- against the same work as plain PyTorch operations on the same device: the reference's per-sample
loop (compose, remove_darkshading on the whole patch, crop, flip, SNA with torch.poisson), every tensor already on the GPU.

    python tools/denoise_batch_bench.py [--reps 50] [--out out/denoise_batch_bench.txt]

Each round times, one after the other, the bare launch (BatchBuilder.launch: what a captured training step replays), the whole call
(BatchBuilder.__call__: host checks, one parameter copy, allocations, launch) and the PyTorch-ops form, each between its own pair of HIP events;
reported: median and the 10th-90th percentile spread over the rounds.  The byte floor is the algorithmic one: the crop windows of noise and clean
and of two shading planes read, two outputs written (6 x 4 B per output element)."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from noisediff_amd import denoise_data as dd, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(REPO, "out", "denoise_batch_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
TRAIN_STEP_MS = 4.39          # TrainableLSID().hip() at B = 4, 256 x 256 (the training step this batch feeds)
B, P, C, HM, WM = 4, 512, 256, 1424, 2128

bayer = {k: synth.uniform(2, f"bench.ds.{k}", (2 * HM, 2 * WM), lo, hi).numpy()
         for k, (lo, hi) in {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}.items()}
blc = {800: 0.25, 1600: -0.5, 3200: 1.0, 25600: 1.75}
shading = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], blc, dev)
noise = (0.2 * synth.normal(2, "bench.noise", (B, 4, P, P))).to(dev)
clean = synth.uniform(2, "bench.clean", (B, 4, P, P), -0.05, 1.1).to(dev)
prm = dict(xy=[(0, 0), (384, 384), (768, 2), (WM - P, HM - P)], iso=[800, 3200, 1600, 25600], ratio=[100, 250, 300, 100],
           crop_xy=[(256, 0), (0, 256), (34, 118), (128, 6)], flip=[1, 1, 1, 1],
           wb=np.array([[0.31, 0.12, 0.55, 0.12], [0.2, 0.1, 0.3, 0.1], [1.0, 0.4, 0.0, 0.4], [0.02, 0.9, 0.7, 0.9]], np.float32),
           K=[dd.sna_gain(i, 0.0) for i in (800, 3200, 1600, 25600)])
build = dd.BatchBuilder(crop=C, patch=P, shading=shading)
inputs = build.update(build.capture_inputs(B, dev), **prm, seed=1)
out_n, out_c = (torch.empty(B, 4, C, C, device=dev) for _ in range(2))


def hip_launch():
    build.launch(inputs, noise, clean, out_n, out_c)


def hip_call():
    return build(noise, clean, **prm, seed=1)


def torch_form():
    """The reference's operations, sample by sample, as torch calls on the device."""
    ns, cs = [], []
    for b in range(B):
        (x0, y0), (cx, cy), iso, ratio = prm["xy"][b], prm["crop_xy"][b], prm["iso"][b], prm["ratio"][b]
        g = clean[b].clamp(0.0, 1.0)
        v = (noise[b].clamp(-1.0, 1.0) + clean[b]).clamp(0.0, 1.0)
        k, o = (shading.k_high, shading.b_high) if iso > 1600 else (shading.k_low, shading.b_low)
        im = (v / ratio * 15871 + 512).clamp(0, 16383)
        im = im - (k[:, y0:y0 + P, x0:x0 + P] * iso + o[:, y0:y0 + P, x0:x0 + P] + blc[iso])
        v = ((im - 512).clamp_min(0) / 15871 * ratio).clamp(0.0, 1.0)
        v, g = v[:, cy:cy + C, cx:cx + C], g[:, cy:cy + C, cx:cx + C]
        if prm["flip"][b]:
            v, g = torch.flip(v, dims=[1]), torch.flip(g, dims=[1])
        wb = prm["wb"][b]
        if np.abs(wb).max() != 0:
            K = prm["K"][b]
            gt = g * 15871 / ratio
            dy = gt * torch.from_numpy(wb).to(dev).reshape(-1, 1, 1)
            dn = torch.poisson(dy / K) * K
            v, g = v + dn / 15871 * ratio, g + dy * ratio / 15871
        ns.append(v)
        cs.append(g)
    return torch.stack(ns), torch.stack(cs)


forms = (("HIP launch", hip_launch), ("HIP call", hip_call), ("PyTorch ops", torch_form))
for _ in range(5):
    for _, fn in forms:
        fn()
torch.cuda.synchronize(dev)
# the two forms compute the same thing: same clean_out up to fp32 rounding, same noisy without the (differently drawn) shot noise
got, want = hip_call(), torch_form()
err_c = float((got[1] - want[1]).abs().max())
times = {name: [] for name, _ in forms}
for _ in range(a.reps):
    for name, fn in forms:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3)

nbytes = 6 * 4 * B * 4 * C * C
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; B={B}, {C}x{C} from {P}x{P}, dark shading + SNA; "
         f"{a.reps} rounds after 5 warm-up rounds, the three forms alternating, one pair of HIP events per call",
         f"byte floor: {nbytes / 2 ** 20:.0f} MiB -> {nbytes / ACHIEVABLE * 1e6:.1f} us at 6.3 TB/s; clean_out of the two forms differs by at most {err_c:.1e}"]
med = {}
for name, _ in forms:
    t = np.array(times[name])
    med[name] = float(np.median(t))
    lines.append(f"{name:>12}: median {med[name]:9.1f} us   p10 {np.percentile(t, 10):9.1f}   p90 {np.percentile(t, 90):9.1f}   min {t.min():9.1f}   max {t.max():9.1f}")
spread = max(np.percentile(times[n], 90) - np.percentile(times[n], 10) for n, _ in forms)
lines.append(f"PyTorch ops / HIP call: {med['PyTorch ops'] / med['HIP call']:.1f}x; PyTorch ops - HIP call = {med['PyTorch ops'] - med['HIP call']:.1f} us "
             f"against a p10-p90 spread of {spread:.1f} us")
lines.append(f"next to the {TRAIN_STEP_MS} ms training step it feeds: HIP launch {100 * med['HIP launch'] / (TRAIN_STEP_MS * 1e3):.2f} %, HIP call "
             f"{100 * med['HIP call'] / (TRAIN_STEP_MS * 1e3):.2f} %, PyTorch ops {100 * med['PyTorch ops'] / (TRAIN_STEP_MS * 1e3):.1f} % of a step")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
