#!/usr/bin/env python3
"""The value histogram of the KLD metric (nd_histogram_f32, noisediff_amd/noise_stats.py) against the same counts as plain PyTorch operations on
the same device and against numpy on the host.

    python tools/noise_stats_bench.py [--reps 100] [--out profiles/noise_stats_bench.txt] [--variants per-wave=PATH,fold=PATH]

Shapes: (a) one generated SID frame, 24 patches of 4 x 512 x 512, as one set; (b) the same as 24 sets; (c) B = 4 at 256 x 256 as one set.  Each on
three value distributions: Gaussian at sigma 0.02, all values equal (every sample in one bin: the worst case of the LDS atomics) and uniform
over the 64 interior bins.  The edges are kld_edges().

Forms: ``HIP call`` is noise_stats.histogram_counts (allocations included); ``HIP launches`` the two launches of nd_histogram_f32 on buffers made
beforehand; ``PyTorch ops`` torch.bucketize on the float64 edges + bincount with the same end and NaN handling; ``--variants`` names other
builds of csrc/noise_stats.hip (-DND_HIST_VARIANT=1 one histogram per wave, 2 a lane folds its run of equal bins; the shipped 0 is plain) whose
nd_histogram_f32 is timed in the same rounds.  numpy on the host (device-to-host copy + np.histogram) is timed three times on the host clock.

Each round times the forms one after the other, each between its own pair of HIP events; reported: median and the 10th-90th percentile over
the rounds.  The byte floor is the input read once at 6.3 TB/s."""
import argparse
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from noisediff_amd import _lib as L, noise_stats as ns
from noisediff_amd._host import _stream

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_stats_bench.txt"))
ap.add_argument("--variants", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
edges = ns.kld_edges()
ed = ns.device_edges(edges, dev)
NB = edges.size - 1
variants = {}
for item in filter(None, a.variants.split(",")):
    name, path = item.split("=")
    lib = C.CDLL(os.path.abspath(path))
    lib.nd_histogram_f32.restype, lib.nd_histogram_f32.argtypes = L.SIGNATURES["nd_histogram_f32"]
    variants[name] = lib

SHAPES = [("24 patches of 4x512x512, S=1", 1, 24 * 4 * 512 * 512), ("24 patches of 4x512x512, S=24", 24, 4 * 512 * 512), ("B=4 of 4x256x256, S=1", 1, 4 * 4 * 256 * 256)]


def data(kind, S, n):
    g = torch.Generator(device=dev).manual_seed(7)
    if kind == "gaussian 0.02":
        return torch.randn(S, n, device=dev, generator=g) * 0.02
    if kind == "all equal":
        return torch.full((S, n), 0.01, device=dev)
    return torch.rand(S, n, device=dev, generator=g) * 0.2 - 0.1


def torch_counts(x):
    S = x.shape[0]
    v = x.double()
    idx = torch.bucketize(v, ed, right=True) - 1
    idx = torch.where(v == ed[-1], NB - 1, idx)
    idx = torch.where((v >= ed[0]) & (v <= ed[-1]), idx, NB)                       # NaN and out-of-range values go to a bin that is dropped
    idx = idx + torch.arange(S, device=dev).view(S, 1) * (NB + 1)
    return torch.bincount(idx.view(-1), minlength=S * (NB + 1)).view(S, NB + 1)[:, :NB]


lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; numpy {np.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms "
         f"alternating, one pair of HIP events per call; times in us; {NB} bins (kld_edges)"]
for title, S, n in SHAPES:
    ws = torch.empty(int(L.call("nd_histogram_workspace_bytes", S, n, NB)), dtype=torch.uint8, device=dev)
    out = torch.empty(S, NB, dtype=torch.int64, device=dev)
    floor = 4.0 * S * n / ACHIEVABLE * 1e6
    for kind in ("gaussian 0.02", "all equal", "uniform interior"):
        x = data(kind, S, n)
        args = (x.data_ptr(), S, n, ed.data_ptr(), NB + 1, out.data_ptr(), ws.data_ptr(), _stream(dev))
        forms = [("HIP call", lambda: ns.histogram_counts(x, ed, per_sample=True)), ("HIP launches", lambda: L.call("nd_histogram_f32", *args))]
        forms += [(f"variant {k}", (lambda lib: lambda: lib.nd_histogram_f32(*args))(lib)) for k, lib in variants.items()]
        forms += [("PyTorch ops", lambda: torch_counts(x))]
        want = torch_counts(x)
        assert torch.equal(ns.histogram_counts(x, ed, per_sample=True), want)
        for k, lib in variants.items():
            out.fill_(-1)
            assert lib.nd_histogram_f32(*args) == 0
            assert torch.equal(out, want), k
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
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            got = np.stack([np.histogram(xh[s], edges)[0] for s in range(S)])
            host.append((time.perf_counter() - t0) * 1e6)
        assert np.array_equal(got, want.cpu().numpy())
        lines.append(f"{title}, {kind}: {4.0 * S * n / 2 ** 20:.0f} MiB read once -> byte floor {floor:.1f} us at 6.3 TB/s; largest bin holds "
                     f"{100.0 * float(want.max()) / n:.1f} % of a set")
        for name, _ in forms:
            t = np.array(times[name])
            lines.append(f"  {name:>18}: median {np.median(t):10.1f}   p10 {np.percentile(t, 10):10.1f}   p90 {np.percentile(t, 90):10.1f}   "
                         f"{np.median(t) / floor:7.1f} x floor")
        lines.append(f"  {'numpy on the host':>18}: median {np.median(host):10.0f}   of 3, host clock, device-to-host copy included")
        print("\n".join(lines[-(len(forms) + 2):]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
