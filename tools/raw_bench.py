#!/usr/bin/env python3
"""Raw Bayer frames (csrc/raw.hip) against the same work as plain PyTorch operations on the same device, and against the reference's route.

    python tools/raw_bench.py [--reps 100] [--out out/raw_bench.txt]

(a) ``raw.load_pair`` on a resident 2848 x 4256 pair with dark shading, against load_image's chain as torch calls on the device and against
    the numpy restatement plus the 2 x 48 MB host-to-device copy on the host clock (the reference's route, a few rounds only).
(b) ``RealBatchBuilder`` and ``PoissonGaussianBatchBuilder`` at B = 4, 256 x 256 crops: the bare launch, the whole call, and the dataset's
    operations as torch calls on the device.

Each round times the forms one after the other, each between its own pair of HIP events; reported: median and the 10th-90th percentile over the
rounds.  Byte floors are the algorithmic ones at 6.3 TB/s: codes read once (2 B each), two planes read where shaded, outputs written once."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from noisediff_amd import denoise_data as dd, raw, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "out", "raw_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
TRAIN_STEP_MS = 4.39          # TrainableLSID().hip() at B = 4, 256 x 256
H, W, B, C = 1424, 2128, 4, 256
ISO, RATIO = 25600, 250

bayer = {k: synth.uniform(2, f"bench.ds.{k}", (2 * H, 2 * W), lo, hi).numpy()
         for k, (lo, hi) in {"k_high": (0.5e-4, 1.5e-4), "b_high": (-2.0, 2.0), "k_low": (0.5e-4, 1.5e-4), "b_low": (-2.0, 2.0)}.items()}
blc = {800: 0.25, 1600: -0.5, 3200: 1.0, 25600: 1.75}
shading = dd.DarkShading(bayer["k_high"], bayer["b_high"], bayer["k_low"], bayer["b_low"], blc, dev)
long_np = np.floor(synth.uniform(2, "bench.raw.long", (2 * H, 2 * W), 400.0, 16384.0).numpy()).astype(np.uint16)
short_np = np.floor(synth.uniform(2, "bench.raw.short", (2 * H, 2 * W), 480.0, 700.0).numpy()).astype(np.uint16)
frames = raw.frames_on_device(np.stack([short_np, long_np]), dev)
short, long = frames[0], frames[1]
WB = 15871.0


def codes(f):
    """uint16 stored as int16 -> float codes, packed (4, H, W): what a torch user has to do without the library."""
    x = (f.to(torch.int32) & 0xFFFF).to(torch.float32)
    return torch.stack((x[0::2, 0::2], x[0::2, 1::2], x[1::2, 1::2], x[1::2, 0::2]))


def planes(iso):
    return (shading.k_high, shading.b_high) if iso > 1600 else (shading.k_low, shading.b_low)


def hip_load_pair():
    return raw.load_pair(short, long, ISO, RATIO, shading)


def torch_load_pair():
    k, o = planes(ISO)
    v = ((codes(short) - 512) / WB * RATIO).clamp(0, 1) / RATIO * WB + 512
    v = v.clamp(0, 16383) - (k * ISO + o + blc[ISO])
    v = ((v - 512).clamp_min(0) / WB * RATIO).clamp(0, 1)
    g = ((codes(long) - 512).clamp_min(0) / WB).clamp(0, 1)
    return v[None], g[None]


def host_load_pair():
    import raw_ref as R
    pl = {n: R.pack_planes(bayer[n]) for n in ("k_high", "b_high")}
    d = R.dark(pl["k_high"], pl["b_high"], ISO, blc[ISO])
    v = R.pack_shaded(R.codes(short_np), d, RATIO)
    g = R.pack(R.codes(long_np), True, 1)
    out = torch.from_numpy(v[None]).to(dev), torch.from_numpy(g[None]).to(dev)
    torch.cuda.synchronize(dev)
    return out


rp = dict(short=[0, 0, 0, 0], long=[1, 1, 1, 1], xy=[(0, 0), (W - C, H - C), (513, 77), (1000, 600)], iso=[800, 3200, 1600, 25600],
          ratio=[100, 250, 300, 100], flip=[1, 1, 1, 1])
pp = dict(frame=[1, 1, 1, 1], xy=rp["xy"], ratio=rp["ratio"], k=[0.76504, 3.06016, 1.53008, 24.48128], var=[2.5, 20.0, 6.0, 900.0], flip=rp["flip"], seed=1)
rb, pb = raw.RealBatchBuilder(C, shading), raw.PoissonGaussianBatchBuilder(C)
ri = rb.update(rb.capture_inputs(B, dev), tuple(frames.shape), **rp)
pi = pb.update(pb.capture_inputs(B, dev), tuple(frames.shape), **pp)
o = [torch.empty(B, 4, C, C, device=dev) for _ in range(4)]


def torch_real():
    ns, cs = [], []
    for b in range(B):
        (x0, y0), iso, ratio = rp["xy"][b], rp["iso"][b], rp["ratio"][b]
        k, off = planes(iso)
        win = (slice(None), slice(y0, y0 + C), slice(x0, x0 + C))
        n = (codes(short[2 * y0:2 * y0 + 2 * C, 2 * x0:2 * x0 + 2 * C]) - 512).clamp_min(0) - (k[win] * iso + off[win] + blc[iso])
        n = (n * ratio).clamp(0, WB) / WB
        g = (codes(long[2 * y0:2 * y0 + 2 * C, 2 * x0:2 * x0 + 2 * C]) - 512).clamp_min(0) / WB
        ns.append(torch.flip(n, dims=[1]))
        cs.append(torch.flip(g, dims=[1]))
    return torch.stack(ns), torch.stack(cs)


def torch_pg():
    ns, cs = [], []
    for b in range(B):
        (x0, y0), ratio, k, var = pp["xy"][b], pp["ratio"][b], pp["k"][b], pp["var"][b]
        c = (codes(long[2 * y0:2 * y0 + 2 * C, 2 * x0:2 * x0 + 2 * C]) - 512).clamp_min(0)
        lam = (c / ratio).double() / k
        n = ((k * torch.poisson(lam) + var ** 0.5 * torch.randn(lam.shape, dtype=torch.float64, device=dev)) * ratio).clamp(0, WB) / WB
        ns.append(torch.flip(n.float(), dims=[1]))
        cs.append(torch.flip(c / WB, dims=[1]))
    return torch.stack(ns), torch.stack(cs)


groups = {
    "load_pair 2848x4256 shaded": (("HIP load_pair", hip_load_pair), ("PyTorch ops", torch_load_pair)),
    f"RealBatchBuilder B={B} {C}x{C} shaded": (("HIP launch", lambda: rb.launch(ri, frames, o[0], o[1])), ("HIP call", lambda: rb(frames, **rp)),
                                              ("PyTorch ops", torch_real)),
    f"PoissonGaussianBatchBuilder B={B} {C}x{C}": (("HIP launch", lambda: pb.launch(pi, frames, o[2], o[3])), ("HIP call", lambda: pb(frames, **pp)),
                                                   ("PyTorch ops", torch_pg)),
}
floors = {
    "load_pair 2848x4256 shaded": (2 * 2 * 4 + 2 * 4 * 4 + 2 * 4 * 4) * H * W,                  # two frames' codes, two planes, two outputs
    f"RealBatchBuilder B={B} {C}x{C} shaded": (2 * 2 * 4 + 2 * 4 * 4 + 2 * 4 * 4) * B * C * C,
    f"PoissonGaussianBatchBuilder B={B} {C}x{C}": (2 * 4 + 2 * 4 * 4) * B * C * C,
}
got, want = hip_load_pair(), torch_load_pair()
err = float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max())
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms of a group alternating, "
         f"one pair of HIP events per call; times in us", f"load_pair: HIP and PyTorch forms differ by at most {err[0]:.1e} (noisy) and {err[1]:.1e} (clean)"]
for title, forms in groups.items():
    for _ in range(5):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in forms}
    for _ in range(a.reps):
        for name, fn in forms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3)
    floor = floors[title] / ACHIEVABLE * 1e6
    lines.append(f"{title}: byte floor {floors[title] / 2 ** 20:.1f} MiB -> {floor:.1f} us at 6.3 TB/s")
    med, spread = {}, 0.0
    for name, _ in forms:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        spread = max(spread, float(np.percentile(t, 90) - np.percentile(t, 10)))
        lines.append(f"  {name:>14}: median {med[name]:10.1f}   p10 {np.percentile(t, 10):10.1f}   p90 {np.percentile(t, 90):10.1f}   "
                     f"{med[name] / floor:7.1f} x floor")
    lib = "HIP call" if "HIP call" in med else "HIP load_pair"
    lines.append(f"  PyTorch ops - {lib} = {med['PyTorch ops'] - med[lib]:.1f} us ({med['PyTorch ops'] / med[lib]:.1f}x) against a larger p10-p90 spread of "
                 f"{spread:.1f} us")
    if "HIP launch" in med:
        lines.append(f"  next to the {TRAIN_STEP_MS} ms training step: HIP launch {100 * med['HIP launch'] / (TRAIN_STEP_MS * 1e3):.2f} %, HIP call "
                     f"{100 * med['HIP call'] / (TRAIN_STEP_MS * 1e3):.2f} %, PyTorch ops {100 * med['PyTorch ops'] / (TRAIN_STEP_MS * 1e3):.1f} % of a step")
host = []
for _ in range(a.host_reps):
    t0 = time.perf_counter()
    host_load_pair()
    host.append((time.perf_counter() - t0) * 1e3)
lines.append(f"load_pair by the reference's route (numpy restatement on the host + 2 x {4 * 4 * H * W / 2 ** 20:.0f} MiB copy), host clock, "
             f"{a.host_reps} rounds: median {np.median(host):.0f} ms, min {min(host):.0f} ms")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
