#!/usr/bin/env python3
"""The noise level function (noisediff_amd/noise_level.py): the moments pass against the same statistics as plain PyTorch operations on the same
device, and the all-pairs Theil-Sen fit per call and per step.

    python tools/noise_level_bench.py [--reps 100] [--out profiles/noise_level_bench.txt]

Moments.  Shapes: B = 4 at 4 x 256 x 256 and one SID frame (4 x 1424 x 2128).  Level distributions: ``natural`` (a smooth ramp over 0 .. 3000
levels with a jitter of 30 levels: neighbours sit on near but different levels), ``one level`` (a dark or clipped frame: every element on one
cache line of the table) and ``uniform`` (independent draws over all 15872 levels).  Forms: ``HIP add`` is LevelMoments.add on a table made
beforehand (the launch of nd_level_moments_f32 and the conversions of the Python layer); ``HIP add + stats`` adds nd_level_stats_f64; the table
is reset before every timed call, outside the pair of events, so it stays within its element limit.  ``PyTorch sort`` forms count, mean and
unbiased std per level from a sort by level, unique_consecutive and differences of float64 prefix sums: no atomics, so its time does not
depend on how many elements share a level.  ``PyTorch scatter`` is bincount + index_add_ in float64, the form with floating-point atomics;
it is timed on the B = 4 shape for the natural and the uniform distribution only (DESIGN.md section 15 says why).  The byte floor is the two
tensors read once at 6.3 TB/s.

Fit.  M = 141, 2000 and 7936 points of a synthetic curve.  ``per step``: the difference of two calls with tol = 0 (no step stops) at 12 and 4
steps, over 8.  ``call, 300``: theil_sen with the defaults (max_iter 300, tol 1e-3), which stops after a few steps on these curves: its device
time holds the launches that exit at their first instruction, and ``host`` is the time the call keeps the host thread (602 launches).  At
M = 141 sklearn's TheilSenRegressor on the host is timed three times where sklearn is installed.

Protocol: ``--reps`` rounds (100) after 5 warm-up rounds, each round times the forms one after the other, each between its own pair of HIP
events; reported: median and the 10th-90th percentile.  Lines are appended to the output file as they are measured."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from noisediff_amd import noise_level as nl

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_level_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
NL, SCALE = nl.N_LEVELS, nl.SCALE


def frame(kind, shape):
    g = torch.Generator(device=dev).manual_seed(7)
    n = int(np.prod(shape))
    if kind == "natural":
        ramp = torch.linspace(0.0, 3000.0, n, device=dev)
        lv = (ramp + 30.0 * torch.randn(n, device=dev, generator=g)).round().clamp(0, NL - 1)
    elif kind == "one level":
        lv = torch.full((n,), 100.0, device=dev)
    else:
        lv = torch.randint(0, NL, (n,), device=dev, generator=g).float()
    clean = (lv / torch.tensor(SCALE, dtype=torch.float32, device=dev)).view(shape)
    noisy = clean + torch.sqrt(2e-4 * clean + 1e-6) * torch.randn(shape, device=dev, generator=g)
    return clean, noisy


def torch_sort_stats(clean, noisy):
    lv, order = torch.sort(torch.round(clean.view(-1) * SCALE).long())
    v = noisy.view(-1).double()[order]
    levels, counts = torch.unique_consecutive(lv, return_counts=True)
    ends = counts.cumsum(0)
    starts = ends - counts
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    c1 = torch.cat([zero, v.cumsum(0)])
    mean = (c1[ends] - c1[starts]) / counts
    d = v - torch.repeat_interleave(mean, counts)
    c2 = torch.cat([zero, (d * d).cumsum(0)])
    std = torch.sqrt((c2[ends] - c2[starts]) / (counts - 1))
    count = torch.zeros(NL, dtype=torch.int64, device=dev)
    count[levels] = counts
    nan = torch.full((NL,), float("nan"), dtype=torch.float64, device=dev)
    return count, nan.clone().index_copy_(0, levels, mean), nan.index_copy_(0, levels, std)


def torch_scatter_stats(clean, noisy):
    lv = torch.round(clean.view(-1) * SCALE).long()
    v = noisy.view(-1).double()
    count = torch.bincount(lv, minlength=NL)
    s1 = torch.zeros(NL, dtype=torch.float64, device=dev).index_add_(0, lv, v)
    mean = s1 / count
    s2 = torch.zeros(NL, dtype=torch.float64, device=dev).index_add_(0, lv, (v - mean[lv]) ** 2)
    return count, mean, torch.sqrt(s2 / (count - 1))


def once(fn, before=None):
    if before is not None:
        before()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3


def timed(forms, before=None):
    """{name: times in us}.  The first call of every form is printed at once, so that a log shows how far a run came."""
    torch.cuda.synchronize(dev)
    for name, fn in forms:
        print(f"    first call of {name}: {once(fn, before):.1f} us", flush=True)
    for _ in range(4):
        for _, fn in forms:
            if before is not None:
                before()
            fn()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in forms}
    for _ in range(a.reps):
        for name, fn in forms:
            times[name].append(once(fn, before))
    return {k: np.array(v) for k, v in times.items()}


def row(name, t, floor=None):
    s = f"  {name:>18}: median {np.median(t):10.1f}   p10 {np.percentile(t, 10):10.1f}   p90 {np.percentile(t, 90):10.1f}"
    return s + (f"   {np.median(t) / floor:7.1f} x floor" if floor else "")


os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").close()
written = 0


def flush_lines():
    global written
    with open(a.out, "a") as f:
        f.write("".join(l + "\n" for l in lines[written:]))
    print("\n".join(lines[written:]), flush=True)
    written = len(lines)


lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; numpy {np.__version__}; {a.reps} rounds after 5 warm-up rounds, the forms "
         f"alternating, one pair of HIP events per call; times in us; {NL} levels"]
flush_lines()
for title, shape in (("B=4 of 4x256x256", (4, 4, 256, 256)), ("one SID frame 4x1424x2128", (4, 1424, 2128))):
    n = int(np.prod(shape))
    floor = 8.0 * n / ACHIEVABLE * 1e6
    mom = nl.LevelMoments(device=dev)
    for kind in ("natural", "one level", "uniform"):
        clean, noisy = frame(kind, shape)
        mom.reset()
        print(f"{title}, {kind}", flush=True)
        count, mean, std = mom.add(clean, noisy).stats()
        torch.cuda.synchronize(dev)
        print("    the table is in", flush=True)
        tc, tm, ts = torch_sort_stats(clean, noisy)
        ok = count >= 2
        assert torch.equal(count, tc) and int(count.sum()) == n and int(mom.counters().sum()) == 0
        assert float((std[ok] - ts[ok]).abs().max()) < 1e-8 and float((mean[ok] - tm[ok]).abs().max()) < 1e-8
        forms = [("HIP add", lambda: mom.add(clean, noisy)), ("HIP add + stats", lambda: mom.add(clean, noisy).stats()),
                 ("PyTorch sort", lambda: torch_sort_stats(clean, noisy))]
        scatter = n <= 1 << 20 and kind != "one level"
        if scatter:
            forms.append(("PyTorch scatter", lambda: torch_scatter_stats(clean, noisy)))
        t = timed(forms, before=mom.reset)
        lines.append(f"{title}, {kind}: 2 x {4.0 * n / 2 ** 20:.0f} MiB read once -> byte floor {floor:.1f} us at 6.3 TB/s; {int((count > 0).sum())} "
                     f"levels in use, the largest holds {100.0 * float(count.max()) / n:.2f} %")
        lines += [row(k, v, floor) for k, v in t.items()]
        if not scatter:
            lines.append(f"  {'PyTorch scatter':>18}: not measured")
        flush_lines()

import noise_level_ref as R  # noqa: E402  (the synthetic curve of the tests)

for M in (141, 2000, 7936):
    xh, yh = R.synthetic_curve(M, 40 + M)
    x, y = torch.from_numpy(xh).to(dev), torch.from_numpy(yh).to(dev)
    slope, icpt, steps = nl.theil_sen(x, y)
    forms = [("steps 4, tol 0", lambda: nl.theil_sen(x, y, max_iter=4, tol=0.0)), ("steps 12, tol 0", lambda: nl.theil_sen(x, y, max_iter=12, tol=0.0)),
             ("call, 300", lambda: nl.theil_sen(x, y))]
    print(f"fit, M = {M}", flush=True)
    t = timed(forms)
    host = []
    for _ in range(a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        nl.theil_sen(x, y)
        host.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize(dev)
    per_step = (np.median(t["steps 12, tol 0"]) - np.median(t["steps 4, tol 0"])) / 8.0
    lines.append(f"fit, M = {M}: {M * (M - 1) // 2} pairs; the default call stops after {int(steps)} steps: slope {float(slope):.6g} intercept {float(icpt):.6g}")
    lines += [row(k, v) for k, v in t.items()]
    lines.append(f"  {'per step':>18}: {per_step:10.1f}   ({M * (M - 1) / 2 / max(per_step, 1e-9) / 1e3:.2f} G pairs/s)")
    lines.append(row("call, 300: host", np.array(host)) + "   host clock, the call alone, no synchronisation inside")
    if M == 141:
        try:
            from sklearn.linear_model import TheilSenRegressor
            sk = []
            for _ in range(3):
                t0 = time.perf_counter()
                reg = TheilSenRegressor().fit(xh.reshape(-1, 1), yh)
                sk.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"  {'sklearn on the host':>18}: median {np.median(sk):10.0f}   of 3, host clock; slope {reg.coef_[0]:.6g} intercept {reg.intercept_:.6g}")
        except ImportError:
            lines.append("  sklearn on the host: not measured (sklearn is not installed)")
    flush_lines()
