#!/usr/bin/env python3
"""Calibration from dark frames (noisediff_amd/calibrate.py) at the SID geometry: 2848 x 4256 codes, n = 12.1 M values per frame, N = 1 and 4.

    python tools/calibrate_bench.py [--reps 20] [--out profiles/calibrate_bench.txt] [--scipy-side 1424x2128]

Timed, each between its own pair of HIP events: the row pass (nd_calib_row_sums_i64), the residual pass (nd_calib_residual_f64), torch.sort of
the residual, one objective evaluation (nd_probplot_f64: the partial launch over all elements and the one-workgroup finalize) with the
Tukey-lambda and with the normal quantile, the search alone (ppcc_max: init + max_eval evaluate / step pairs, the ones after the stop leaving
at their first instruction) and one whole calibrate_dark_frames.  The evaluation reads 8 bytes per element: its achieved bytes/s stands next
to the 6.3 TB/s the HBM-bound passes of DESIGN.md section 8 reach, which says whether the fp64 transcendentals (log, log1p and two expm1 per
element; one normcdfinv) or the bytes bound it.  The frames are synthetic dark frames: rint(512 + 3.2 Q(u, -0.044) + g[c, Y]).

Protocol: ``--reps`` rounds after 3 warm-up rounds, the forms one after the other in every round; reported: median and the 10th-90th
percentile, in us.  scipy on the host (ppcc_max with the same bracket and probplot twice, after numpy's sort) is timed ONCE on one frame of
``--scipy-side`` codes, a size at which it finishes in about a minute at the most; the GPU's whole call on that frame stands next to it."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from noisediff_amd import calibrate as K

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "calibrate_bench.txt"))
ap.add_argument("--scipy-side", default="1424x2128")
a = ap.parse_args()
dev = torch.device("cuda", 0)
ACHIEVABLE = 6.3e12
LAM, STL, SR = -0.044, 3.2, 1.0


def dark_frames(N, H2, W2, seed):
    """uint16 (N, H2, W2) as int16 storage on the device, drawn there (a bench input: its bits are not pinned)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(N, H2, W2, dtype=torch.float64, device=dev, generator=g).clamp_(1e-12, 1 - 1e-12)
    q = (torch.expm1(LAM * torch.log(u)) - torch.expm1(LAM * torch.log1p(-u))) / LAM
    rows = torch.randn(N, H2, 1, dtype=torch.float64, device=dev, generator=g)
    return torch.round(512 + STL * q + SR * rows).clamp_(0, 65535).to(torch.int32).to(torch.int16)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3


def timed(forms):
    torch.cuda.synchronize(dev)
    for _ in range(3):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize(dev)
    times = {name: [] for name, _ in forms}
    for _ in range(a.reps):
        for name, fn in forms:
            times[name].append(once(fn))
    return {k: np.array(v) for k, v in times.items()}


def row(name, t, extra=""):
    return f"  {name:>28}: median {np.median(t):11.1f}   p10 {np.percentile(t, 10):11.1f}   p90 {np.percentile(t, 90):11.1f}{extra}"


lines = [f"device {torch.cuda.get_device_name(dev)}; torch {torch.__version__}; {a.reps} rounds after 3 warm-up rounds, one pair of HIP events per call; times in us"]
for N in (1, 4):
    f = dark_frames(N, 2848, 4256, 5 + N)
    n = 4 * 1424 * 2128
    R = K.row_sums(f)
    x = K.residuals(f, R)
    xs = torch.sort(x, dim=1).values
    lam = torch.full((N,), LAM, dtype=torch.float64, device=dev)
    found, r, n_eval = K.ppcc_max(xs)
    forms = [("row pass", lambda: K.row_sums(f, out=R)), ("residual pass", lambda: K.residuals(f, R, out=x)), ("torch.sort", lambda: torch.sort(x, dim=1)),
             ("evaluation, Tukey-lambda", lambda: K.probplot(xs, lam)), ("evaluation, normal", lambda: K.probplot(xs)),
             ("ppcc_max, 32 pairs enqueued", lambda: K.ppcc_max(xs)), ("calibrate_dark_frames", lambda: K.calibrate_dark_frames(f))]
    t = timed(forms)
    lines.append(f"N = {N} of 2848 x 4256 codes, n = {n}: the search took {n_eval.tolist()} evaluations, lam {[round(v, 6) for v in found.tolist()]}, "
                 f"r {[round(v, 8) for v in r.tolist()]}")
    for name, v in t.items():
        extra = ""
        if name.startswith("evaluation"):
            extra = f"   {8.0 * n * N / (np.median(v) * 1e-6) / 1e12:6.3f} TB/s of the 8 B per element it reads ({ACHIEVABLE / 1e12:.1f} TB/s: section 8's streaming rate)"
        elif name == "row pass":
            extra = f"   {2.0 * n * N / (np.median(v) * 1e-6) / 1e12:6.3f} TB/s of the codes"
        elif name == "residual pass":
            extra = f"   {10.0 * n * N / (np.median(v) * 1e-6) / 1e12:6.3f} TB/s of codes read and fp64 written"
        lines.append(row(name, v, extra))
    per_eval = np.median(t["ppcc_max, 32 pairs enqueued"]) / max(int(n_eval.max()), 1)
    lines.append(f"  {'search / evaluations taken':>28}: {per_eval:11.1f}")
    del f, R, x, xs
    torch.cuda.empty_cache()

try:
    from scipy import stats
    H2, W2 = (int(v) for v in a.scipy_side.split("x"))
    f = dark_frames(1, H2, W2, 3)
    res = K.calibrate_dark_frames(f).cpu()
    gpu = np.median([once(lambda: K.calibrate_dark_frames(f)) for _ in range(5)])
    codes = f.cpu().numpy().view(np.uint16).astype(np.int64)
    t0 = time.perf_counter()
    packed = np.stack([codes[0, r::2, c::2] for r, c in ((0, 0), (0, 1), (1, 1), (1, 0))]) - 512.0
    xh = np.sort((packed - packed.mean(axis=2, keepdims=True)).reshape(-1))
    lam_s = stats.ppcc_max(xh, brack=(K.LO, K.HI), dist="tukeylambda")
    tl = stats.probplot(xh, sparams=(lam_s,), dist="tukeylambda")[1]
    gs = stats.probplot(xh)[1]
    host = time.perf_counter() - t0
    lines.append(f"one frame of {H2} x {W2} codes (n = {xh.size}): scipy on the host (sort, ppcc_max with brack = ({K.LO}, {K.HI}), probplot twice) {host:.1f} s, "
                 f"once; calibrate_dark_frames {gpu / 1e3:.2f} ms (median of 5).  lam scipy {lam_s:.6f} GPU {res['lam'][0]:.6f}; sigTL scipy {tl[0]:.5f} GPU "
                 f"{res['sigTL'][0]:.5f}; sigGs scipy {gs[0]:.5f} GPU {res['sigGs'][0]:.5f}")
except ImportError:
    lines.append("scipy on the host: not measured (scipy is not installed)")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines))
