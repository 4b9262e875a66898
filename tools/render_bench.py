#!/usr/bin/env python3
"""Developing a packed frame to sRGB (csrc/develop.hip) against its byte floor, against the other placement of the tone curve, and against the
route without it.

    python tools/render_bench.py [--reps 100] [--out profiles/render_bench.txt] [--variant global=PATH]

One SID frame, 4 x 1424 x 2128 fp32 -> 1424 x 2128 x 3 (half size) and -> 2848 x 4256 x 3 (full resolution, bilinear), uint8.  Each round times
the forms of a group one after the other, each between its own pair of HIP events; reported: median and the 10th-90th percentile over the rounds.
Byte floors at 6.3 TB/s: the source read once, the output written once.  ``--variant global=PATH`` names a build of csrc/develop.hip with
-DND_DEVELOP_CURVE_LDS=0 (``python -m noisediff_amd.build --variant develop ND_DEVELOP_CURVE_LDS=0 PATH``): the curve read from global memory
through L2, a thread item or tile per thread or workgroup; in the shipped build one workgroup per CU holds the curve in LDS.  The route without the kernel: ``raw.to_bayer``, the 24 MB copy to the host and the
numpy restatement (tests/render_ref.py) there, on the host clock, a few rounds (rawpy is not a dependency, so LibRaw itself is not timed)."""
import argparse
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from noisediff_amd import _lib as L, raw, render, synth
from noisediff_amd._host import _stream

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_bench.txt"))
ap.add_argument("--variant", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
H, W = 1424, 2128
BLACK, CAM = (512, 512, 512, 512), (2.3, 1, 1.6, 0)
MATRIX = [[1.9, -0.7, -0.2], [-0.25, 1.6, -0.35], [0.03, -0.55, 1.52]]

variants = {}
for item in filter(None, a.variant.split(",")):
    name, path = item.split("=")
    lib = C.CDLL(os.path.abspath(path))
    lib.nd_raw_develop.restype, lib.nd_raw_develop.argtypes = L.SIGNATURES["nd_raw_develop"]
    variants[name] = lib

# a smooth picture with noise on it, as a denoised frame is: neighbouring pixels read neighbouring entries of the curve
yy, xx = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
base = (0.5 + 0.5 * np.sin(6.0 * xx + 3.0 * yy) * np.cos(4.0 * yy)) ** 2
img = np.clip(base[None] * np.array([0.35, 0.8, 0.5, 0.8], np.float32)[:, None, None] + synth.uniform(2, "bench.render", (4, H, W), -0.02, 0.02).numpy(), 0, 1)
x = torch.from_numpy(img.astype(np.float32)[None]).to(dev)
flat = torch.from_numpy(synth.uniform(2, "bench.render.flat", (1, 4, H, W), 0.0, 1.0).numpy()).to(dev)      # no locality at all in the curve reads
modes = {"half size": render.Develop(BLACK, cam_mul=CAM, rgb_cam=MATRIX), "full resolution": render.Develop(BLACK, cam_mul=CAM, rgb_cam=MATRIX, half_size=False)}
floors = {"half size": (16 + 3) * H * W, "full resolution": (16 + 12) * H * W}


def launcher(lib, d, src, out):
    p = d.params()
    args = (src.data_ptr(), None, 1, H, W, C.byref(p), d.device_curve(dev).data_ptr(), out.data_ptr(), H, W)
    return lambda: lib.nd_raw_develop(*args, _stream(dev))


def host_route(d):
    import render_ref as RR
    mosaic = raw.to_bayer(x, d.black)
    codes = (mosaic if mosaic.dtype == torch.int16 else mosaic.view(torch.int16)).cpu().numpy().view(np.uint16)
    return RR.develop(codes[0], d.black, d.white, d.scale_mul, d.rgb_cam, d.curve, 8, not d.half_size)


lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms of a group alternating, "
         f"one pair of HIP events per call; times in us; one frame 4 x {H} x {W} fp32, uint8 out"]
for title, d in modes.items():
    k = 1 if d.half_size else 2
    for picture, src in (("smooth picture", x), ("uniform random values", flat)):
        outs = {"HIP call": None}
        forms = [("HIP call", lambda src=src: d(src))]
        outs["HIP launch"] = torch.empty(1, k * H, k * W, 3, dtype=torch.uint8, device=dev)
        forms.append(("HIP launch", launcher(L.load(), d, src, outs["HIP launch"])))
        for name, lib in variants.items():
            outs[name] = torch.zeros(1, k * H, k * W, 3, dtype=torch.uint8, device=dev)
            forms.append((f"curve in {name}", launcher(lib, d, src, outs[name])))
        for _ in range(5):
            for _, fn in forms:
                fn()
        torch.cuda.synchronize(dev)
        same = {name: bool(torch.equal(outs[name], outs["HIP launch"])) for name in variants}
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
        lines.append(f"{title}, {picture}: byte floor {floors[title] / 2 ** 20:.1f} MiB -> {floor:.1f} us at 6.3 TB/s")
        med, spread = {}, 0.0
        for name, _ in forms:
            t = np.array(times[name])
            med[name] = float(np.median(t))
            spread = max(spread, float(np.percentile(t, 90) - np.percentile(t, 10)))
            lines.append(f"  {name:>14}: median {med[name]:9.1f}   p10 {np.percentile(t, 10):9.1f}   p90 {np.percentile(t, 90):9.1f}   {med[name] / floor:6.1f} x floor")
        for name in variants:
            lines.append(f"  curve in {name} memory - curve in LDS (HIP launch) = {med[f'curve in {name}'] - med['HIP launch']:+.1f} us against a larger p10-p90 spread of "
                         f"{spread:.1f} us; the two write the same bytes: {same[name]}")
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        want = host_route(d)
        host.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  {title} without the kernel (to_bayer, {2 * 4 * H * W / 2 ** 20:.0f} MiB to the host, numpy restatement there), host clock, {a.host_reps} rounds: "
                 f"median {np.median(host):.0f} ms, min {min(host):.0f} ms; the kernel's picture equals it: {bool(np.array_equal(d(x)[0].cpu().numpy(), want))}")
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
