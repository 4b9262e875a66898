#!/usr/bin/env python3
"""The diffusion sets' batches (nd_raw_diffusion_batch_f32, noisediff_amd/diffusion_data.py) against the same arithmetic as plain PyTorch
operations on the same device, and against the reference's host route.

    python tools/diffusion_data_bench.py [--reps 100] [--out out/diffusion_data_bench.txt]

(a) ``DiffusionBatchBuilder`` at B = 4, 256 x 256 crops of a resident 2848 x 4256 pair, outputs noise + clean_img + coord: the bare launch, the
    whole call, and SonyTrainDataset.__getitem__'s operations on the windows as torch calls on the device.
(b) ``GenerationBatchBuilder`` at B = 4, 512 x 512 patches (the shipped script.sh shape): the same three forms.
(c) Once: the reference's route for ONE training sample, the numpy restatement over the whole frames (two packs, the multiply, clip and
    subtraction, the whole coordinate grid, then the crop) plus the copy of the crops, on the host clock.

Each round times the forms of a group one after the other, each between its own pair of HIP events; reported: median and the 10th-90th
percentile over the rounds.  Byte floors are the algorithmic ones at 6.3 TB/s: the windows' codes read once (2 B each), outputs written once."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from noisediff_amd import diffusion_data as dd, io, raw, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=os.path.join(REPO, "out", "diffusion_data_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
TRAIN_STEP_MS = 25.0          # TrainableNoiseDiffNet(dim=64).hip() at B = 4, 256 x 256, one graph
H, W, B = io.PACKED_H, io.PACKED_W, 4
WB = 15871.0

long_np = np.floor(synth.uniform(2, "bench.raw.long", (2 * H, 2 * W), 400.0, 16384.0).numpy()).astype(np.uint16)
short_np = np.floor(synth.uniform(2, "bench.raw.short", (2 * H, 2 * W), 480.0, 700.0).numpy()).astype(np.uint16)
frames = raw.frames_on_device(np.stack([short_np, long_np]), dev)
short, long = frames[0], frames[1]
shape = tuple(frames.shape)


def codes(f, x0, y0, c):
    """uint16 stored as int16 -> float codes of one window, packed (4, c, c): what a torch user has to do without the library."""
    x = (f[2 * y0:2 * y0 + 2 * c, 2 * x0:2 * x0 + 2 * c].to(torch.int32) & 0xFFFF).to(torch.float32)
    return torch.stack((x[0::2, 0::2], x[0::2, 1::2], x[1::2, 1::2], x[1::2, 0::2]))


def coord(x0, y0, c):
    rows = torch.arange(y0, y0 + c, device=dev).float() / (H - 1)
    cols = torch.arange(x0, x0 + c, device=dev).float() / (W - 1)
    return torch.stack(torch.meshgrid([rows, cols], indexing="ij"))


# ---- (a) training batches
CT = 256
tp = dict(short=[0, 0, 0, 0], long=[1, 1, 1, 1], xy=[(0, 0), (W - CT, H - CT - 1), (513, 77), (1001, 600)], ratio=[100, 250, 300, 100])
tb = dd.DiffusionBatchBuilder(CT)
ti = tb.update(tb.capture_inputs(B, dev), shape, **tp)
WANT = ("noise", "clean_img", "coord")
tout = {k: torch.empty(B, 2 if k == "coord" else 4, CT, CT, device=dev) for k in WANT}


def torch_train():
    ns, cs, ps = [], [], []
    for b in range(B):
        (x0, y0), ratio = tp["xy"][b], tp["ratio"][b]
        noisy = ((codes(short, x0, y0, CT) - 512).clamp_min(0) / WB * ratio).clamp(0, 1)
        clean = (codes(long, x0, y0, CT) - 512).clamp_min(0) / WB
        ns.append(noisy - clean)
        cs.append(clean)
        ps.append(coord(x0, y0, CT))
    return {"noise": torch.stack(ns), "clean_img": torch.stack(cs), "coord": torch.stack(ps)}


# ---- (b) generation batches
CG = 512
gb = dd.GenerationBatchBuilder(CG)
gframe, gxy = next(gb.frame_batches(1, B))
gi = gb.update(gb.capture_inputs(B, dev), shape, gframe, gxy)
gout = {"clean_img": torch.empty(B, 4, CG, CG, device=dev), "position": torch.empty(B, 2, CG, CG, device=dev)}


def torch_gen():
    cs, ps = [], []
    for x0, y0 in gxy:
        cs.append((codes(long, x0, y0, CG) - 512).clamp_min(0) / WB)
        ps.append(coord(x0, y0, CG))
    return {"clean_img": torch.stack(cs), "position": torch.stack(ps)}


# ---- (c) the reference's host route for one training sample
def host_sample():
    import diffusion_data_ref as D
    import raw_ref as R
    (x0, y0), ratio = tp["xy"][2], tp["ratio"][2]
    noisy = D.noisy(R.codes(short_np), ratio)                 # pack_raw(raw) * ratio, clipped: the whole frame
    clean = D.clean(R.codes(long_np))                         # pack_raw(gt_raw): the whole frame
    noise = noisy - clean
    grid = D.coord(H, W, 0, 0, H, W)                          # make_coord(H, W): the whole grid
    crops = [np.ascontiguousarray(t[:, y0:y0 + CT, x0:x0 + CT]) for t in (noise, noisy, clean, grid)]
    out = [torch.from_numpy(t).to(dev) for t in crops]
    torch.cuda.synchronize(dev)
    return out


groups = {
    f"DiffusionBatchBuilder B={B} {CT}x{CT} noise+clean_img+coord": (("HIP launch", lambda: tb.launch(ti, frames, tout, want=WANT)),
                                                                     ("HIP call", lambda: tb(frames, **tp, want=WANT)), ("PyTorch ops", torch_train)),
    f"GenerationBatchBuilder B={B} {CG}x{CG}": (("HIP launch", lambda: gb.launch(gi, frames, gout)), ("HIP call", lambda: gb(frames, gframe, gxy, 0)),
                                                ("PyTorch ops", torch_gen)),
}
floors = {
    f"DiffusionBatchBuilder B={B} {CT}x{CT} noise+clean_img+coord": (2 * 2 * 4 + (4 + 4 + 2) * 4) * B * CT * CT,        # two frames' codes, ten planes
    f"GenerationBatchBuilder B={B} {CG}x{CG}": (2 * 4 + (4 + 2) * 4) * B * CG * CG,
}
got, want = tb(frames, **tp, want=WANT), torch_train()
err = {k: float((got[k] - want[k]).abs().max()) for k in WANT}
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms of a group alternating, "
         f"one pair of HIP events per call; times in us",
         "training batch: HIP and PyTorch forms differ by at most " + ", ".join(f"{v:.1e} ({k})" for k, v in err.items())]
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
    lines.append(f"  PyTorch ops - HIP call = {med['PyTorch ops'] - med['HIP call']:.1f} us ({med['PyTorch ops'] / med['HIP call']:.1f}x) against a larger "
                 f"p10-p90 spread of {spread:.1f} us")
    lines.append(f"  next to the {TRAIN_STEP_MS} ms training step: HIP launch {100 * med['HIP launch'] / (TRAIN_STEP_MS * 1e3):.3f} %, HIP call "
                 f"{100 * med['HIP call'] / (TRAIN_STEP_MS * 1e3):.2f} %, PyTorch ops {100 * med['PyTorch ops'] / (TRAIN_STEP_MS * 1e3):.1f} % of a step")
t0 = time.perf_counter()
host_sample()
host_ms = (time.perf_counter() - t0) * 1e3
lines.append(f"one training sample by the reference's route (numpy restatement over the whole 2848 x 4256 pair, crop, copy of the four {CT} x {CT} "
             f"crops), host clock, once: {host_ms:.0f} ms; a batch of {B} is {B} of these")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
