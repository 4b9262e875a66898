#!/usr/bin/env python3
"""Golden vectors for noisediff_amd.noise_stats: the reference's own KLD and patch-statistics code on the CPU, run on small seeded inputs.

    python tests/golden/capture_noise_stats.py      # writes tests/golden/noise_stats.npz

As in capture_diffusion_data.py the functions are taken out of the reference's files with ``ast`` and executed with numpy, torch and sklearn in
scope: ``get_histogram`` and the four ``kl_div_*`` (utils/util.py:188-227), ``sliding_window`` and ``compute_poisson_lambda_by_patch``
(utils/raw_util.py:161-189).  The 67 edges are formed by the two lines of ``kldiv_patch_set`` (:245-246), which is not callable on its own.

Stored: the inputs; the counts (hist * n, exact) and the hists on the KLD edges and on get_histogram's default 1001 edges, per set and for
the whole tensor; the three divergences of real against generated; the fp32 std / mean maps and the fitted slopes and intercepts."""
import ast
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F
from sklearn.linear_model import LinearRegression

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
from capture_golden import REF as REF_TREE  # noqa: E402  (where the reference checkout is)
from noise_stats_ref import ramp_image  # noqa: E402  (the fit's seeded input)

SEED = 61
FIT_SHAPES = [(1, 1, 1, 7), (1, 2, 3, 3), (2, 4, 24, 40), (1, 1, 33, 257)]
MAP_SHAPES = [(1, 2, 3, 3), (2, 4, 24, 40)]


def load(path, names, scope):
    tree = ast.parse(open(path).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert set(found) == set(names), (path, set(names) - set(found))
    exec(compile(ast.Module(body=list(found.values()), type_ignores=[]), path, "exec"), scope)
    return scope


U = load(os.path.join(REF_TREE, "utils", "util.py"), {"get_histogram", "kl_div_forward", "kl_div_inverse", "kl_div_sym", "kl_div_3"}, {"np": np})
R = load(os.path.join(REF_TREE, "utils", "raw_util.py"), {"sliding_window", "compute_poisson_lambda_by_patch"},
         {"np": np, "torch": torch, "F": F, "LinearRegression": LinearRegression})

bw = 0.2 / 64                                                                                  # utils/util.py:245-246
bin_edges = np.concatenate(([-1000.0], np.arange(-0.1, 0.1 + 1e-9, bw), [1000.0]), axis=0)
assert bin_edges.shape == (67,) and bin_edges[33] == 8.326672684688674e-17 and bin_edges[65] == 0.10000000000000017

rs = np.random.RandomState(SEED)
S, SHAPE = 3, (4, 16, 16)
generated = (rs.standard_normal((S,) + SHAPE) * np.array([0.02, 0.03, 0.005]).reshape(S, 1, 1, 1)).astype(np.float32)
real = (rs.standard_normal((S,) + SHAPE) * 0.025).astype(np.float32)
real[0, 0, 0, :6] = [0.5, -0.7, 1000.0, -1000.0, 1000.5, -1001.0]                             # the two outer bins and beyond them
unit = rs.uniform(-0.05, 1.05, (2, 1500)).astype(np.float32)                                   # for the default layout: some values outside [0, 1]
unit[0, :3] = [0.0, 1.0, 0.5]
special = np.array([np.nan, 1000, -1000, 1000.5, -1001, np.inf, -np.inf, 0.0, -0.0], np.float32)

out = {"meta.seed": np.int64(SEED), "kld_edges": bin_edges, "generated": generated, "real": real, "unit": unit, "special": special}


def hist(data, **kw):
    h, centers = U["get_histogram"](data, **kw)
    c = np.rint(h * np.prod(data.shape)).astype(np.int64)
    assert np.array_equal(c / np.prod(data.shape), h)
    return c, h, centers


c, h, _ = hist(special, bin_edges=bin_edges)
assert c.sum() == 4 and c[0] == 1 and c[32] == 2 and c[65] == 1
out["special.counts"] = c
for name, data in (("generated", generated), ("real", real)):
    c, h, centers = hist(data, bin_edges=bin_edges)
    out[f"{name}.counts"], out[f"{name}.hist"] = c, h
    per = [hist(data[s], bin_edges=bin_edges) for s in range(S)]
    out[f"{name}.counts.per_sample"], out[f"{name}.hist.per_sample"] = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
out["kld_centers"] = centers
c, h, centers = hist(unit)
out["unit.counts"], out["unit.hist"], out["unit.centers"] = c, h, centers
assert h.shape == (1000,)
per = [hist(unit[s]) for s in range(2)]
out["unit.counts.per_sample"], out["unit.hist.per_sample"] = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])

# kldiv_patch_set's order: kl_div_forward(hist_real, hist_generated)
kl3 = lambda p, q: np.array(U["kl_div_3"](p, q), np.float64)  # noqa: E731
out["kl3"] = kl3(out["real.hist"], out["generated.hist"])
out["kl3.per_sample"] = np.stack([kl3(out["real.hist.per_sample"][s], out["generated.hist.per_sample"][s]) for s in range(S)])
assert out["kl3"][0] == U["kl_div_forward"](out["real.hist"], out["generated.hist"]) and out["kl3"][1] == U["kl_div_inverse"](out["real.hist"], out["generated.hist"])
assert out["kl3"][2] == U["kl_div_sym"](out["real.hist"], out["generated.hist"])
out["kl3.unit"] = kl3(out["unit.hist.per_sample"][0], out["unit.hist.per_sample"][1])

for shape in FIT_SHAPES:
    key = "x".join(map(str, shape))
    x = ramp_image(SEED + sum(shape), shape)
    lam, icpt = R["compute_poisson_lambda_by_patch"](x)
    out[f"fit.{key}.x"], out[f"fit.{key}.lambda"], out[f"fit.{key}.intercept"] = x.numpy(), np.asarray(lam, np.float64), np.asarray(icpt, np.float64).reshape(shape[:2])
    if shape in MAP_SHAPES:
        std, mean = torch.std_mean(R["sliding_window"](x), dim=2)
        out[f"fit.{key}.std"], out[f"fit.{key}.mean"] = std.view(shape).numpy(), mean.view(shape).numpy()

path = os.path.join(HERE, "noise_stats.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:      # np.savez_compressed at the highest level
    for k, v in out.items():
        with zf.open(k + ".npy", "w") as f:
            np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
print({k: getattr(v, "shape", ()) for k, v in out.items()})
print("kl3", out["kl3"], "lambda", out["fit.2x4x24x40.lambda"][0])
print("bytes", os.path.getsize(path))
assert os.path.getsize(path) < 512 * 1024
