#!/usr/bin/env python3
"""Whole synthetic frames (nd_frame_assemble, noisediff_amd/frame.py) at the SID geometry: the assembly launch against its byte floor, and one
whole-frame FrameSynthesizer call next to the sampling it wraps.

    python tools/frame_bench.py [--reps 200] [--dim 64] [--sampling-timesteps 50] [--calls 2] [--out out/frame_bench.txt]

(a) ``FrameAssembler.launch`` for the first 16 patches (crop 256) of a 1424 x 2128 packed frame into persistent outputs, with all three outputs
    and with noisy alone: one pair of HIP events per launch, the two forms alternating; median and 10th-90th percentile over the rounds.  Bytes:
    the patches' owned pixels read once (16 B a packed pixel), the long exposure's codes under them (8 B), each output written once (noise 16 B,
    noisy 16 B, short 8 B), against the 5.6 TB/s the project's own streaming passes reach.  Beside them the same grid with every rectangle
    empty (the fixed cost of one launch between two events) and all 88 patches of the frame in one launch.
(b) One ``FrameSynthesizer`` call for one frame: 88 patches in 6 batches of 16 (the last padded with 8 empty rows), host clock around the call and a
    device synchronise, next to the same six ``sample()`` calls alone on the conditions of those batches."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from noisediff_amd import GaussianDiffusion, NoiseDiffNet, frame as FR, io, raw, synth
from noisediff_amd.diffusion_data import GenerationBatchBuilder
from noisediff_amd.spec import noisediff_param_spec

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--sampling-timesteps", type=int, default=50)
ap.add_argument("--calls", type=int, default=2)
ap.add_argument("--out", default=os.path.join(REPO, "out", "frame_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
STREAMING = 5.6e12
H, W, C, B = io.PACKED_H, io.PACKED_W, 256, 16
KEYS = FR.WANT

long_np = np.floor(synth.uniform(2, "bench.frame.long", (1, 2 * H, 2 * W), 400.0, 16384.0).numpy()).astype(np.uint16)
frames = raw.frames_on_device(long_np, dev)
shape = tuple(frames.shape)
lay = FR.FrameLayout(C, (H, W))
lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; packed frame {H} x {W}, crop {C}, {len(lay)} patches a frame"]

# ---- (a) the launch
asm = FR.FrameAssembler(C)
patches = synth.uniform(3, "bench.frame.patches", (B, 4, C, C), -1.2, 1.2).to(dev)
inputs = asm.update(asm.capture_inputs(B, dev), shape, 1, [0] * B, [0] * B, lay.patches[:B], lay.rects[:B], 100.0, KEYS)
out = {"noise": torch.empty(1, 4, H, W, device=dev), "noisy": torch.empty(1, 4, H, W, device=dev),
       "short": torch.empty(1, 2 * H, 2 * W, dtype=raw._U16[-1], device=dev)}
owned = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in lay.rects[:B])
# two more launches say where the time of so small a launch goes: the same grid with every rectangle empty (each thread reads its row and leaves:
# the fixed cost of a launch between two events), and the whole frame's 88 patches in one launch (5.5 times the bytes behind the same fixed cost)
empty = asm.update(asm.capture_inputs(B, dev), shape, 1, [0] * B, [0] * B, lay.patches[:B], [(x0, y0, x0, y0) for x0, y0, _, _ in lay.rects[:B]], 100.0, KEYS)
P = len(lay)
every = asm.update(asm.capture_inputs(P, dev), shape, 1, [0] * P, [0] * P, lay.patches, lay.rects, 100.0, KEYS)
patches_every = synth.uniform(3, "bench.frame.patches.every", (P, 4, C, C), -1.2, 1.2).to(dev)
ALL = 16 + 8 + 16 + 16 + 8
forms = {"noise + noisy + short": (inputs, patches, KEYS, owned * ALL), "noisy alone": (inputs, patches, ("noisy",), owned * (16 + 8 + 16)),
         "all three, empty rows": (empty, patches, KEYS, 0), f"all three, {P} patches": (every, patches_every, KEYS, H * W * ALL)}
for block, src, want, _ in forms.values():
    for _ in range(5):
        asm.launch(block, src, frames, out=out, want=want)
torch.cuda.synchronize(dev)
times = {name: [] for name in forms}
for _ in range(a.reps):
    for name, (block, src, want, _) in forms.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        asm.launch(block, src, frames, out=out, want=want)
        t1.record()
        t1.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3)
lines.append(f"(a) FrameAssembler.launch, {B} patches owning {owned} packed pixels ({100 * owned / (B * C * C):.0f} % of their area); {a.reps} rounds after 5 "
             "warm-up launches, the forms alternating, one pair of HIP events per launch; times in us")
for name, (_, _, _, nbytes) in forms.items():
    t = np.array(times[name])
    med = float(np.median(t))
    lines.append(f"  {name:>22}: median {med:8.1f}   p10 {np.percentile(t, 10):8.1f}   p90 {np.percentile(t, 90):8.1f}   {nbytes / 2 ** 20:6.1f} MiB moved -> "
                 f"{nbytes / (med * 1e-6) / 1e12:.2f} TB/s, {100 * nbytes / (med * 1e-6) / STREAMING:.0f} % of the 5.6 TB/s of the streaming passes")

# ---- (b) one whole frame
net = NoiseDiffNet(SimpleNamespace(dim=a.dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
net.load_state_dict(synth.make_state_dict(noisediff_param_spec(a.dim), 0), strict=True)
net = net.to(dev).eval()
gs = GaussianDiffusion(net, image_size=C, timesteps=1000, sampling_timesteps=a.sampling_timesteps, beta_schedule="sigmoid2").to(dev)
synthesize = FR.FrameSynthesizer(C)
res = {k: out[k] for k in KEYS}


def whole():
    synthesize(gs, frames, [0], 31, 100.0, batch_size=B, seed=5, want=KEYS, out=res)
    torch.cuda.synchronize(dev)


gb = GenerationBatchBuilder(C)
conds = [gb(frames, [0] * B, xy, 31) for _, _, xy, _ in synthesize.batches(lay, 1, B)]


def sampling():
    for k, cond in enumerate(conds):
        gs.sample_offset = k * B
        gs.sample(batch_size=B, condition=cond, seed=5)
    gs.sample_offset = 0
    torch.cuda.synchronize(dev)


whole()                                                          # the plan, the captured step graph, the code objects
sampling()
clock = {"FrameSynthesizer call": [], "the six sample() calls alone": []}
for _ in range(a.calls):
    for name, fn in zip(clock, (whole, sampling)):
        t0 = time.perf_counter()
        fn()
        clock[name].append((time.perf_counter() - t0) * 1e3)
lines.append(f"(b) one frame, {len(lay)} patches in {len(conds)} batches of {B}; NoiseDiffNet dim {a.dim}, {a.sampling_timesteps}-step DDIM of 1000; host clock to a device "
             f"synchronise, {a.calls} calls each after one warm-up call, alternating; times in ms")
for name, t in clock.items():
    lines.append(f"  {name:>30}: " + ", ".join(f"{v:.1f}" for v in t) + f"   (median {float(np.median(t)):.1f})")
extra = float(np.median(clock["FrameSynthesizer call"]) - np.median(clock["the six sample() calls alone"]))
lines.append(f"  conditions, table uploads and assembly of the whole frame: {extra:.1f} ms of the call "
             f"({100 * extra / float(np.median(clock['FrameSynthesizer call'])):.1f} %)")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
