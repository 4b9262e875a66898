#!/usr/bin/env python3
"""Golden vectors for noisediff_amd.metrics.IlluminanceCorrect: the reference's own class (test_denoising.py:232-263) on CPU fp32.

    python tests/golden/capture_metrics.py      # writes tests/golden/metrics.npz

test_denoising.py cannot be imported without its dependencies (rawpy, exifread, skimage, and cv2 / tensorboardX through its trainer), so
the class is taken out of the file with ``ast`` and executed with only torch in scope.  Inputs are synthetic (noisediff_amd.synth); stored: inputs and the
reference's outputs.
  case "b":  pred (2, 4, 32, 48) in [-0.2, 1.2], source of batch 2 with ~10 % of its values exactly 1 (excluded from the dot products)
  case "b1": the same pred against a batch-1 source (the reference's broadcast branch)
  case "z":  den == 0: every pred value at a pixel whose source is not 1 is <= 0, so num = den = 0 and the output is NaN"""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from capture_golden import REF as REF_TREE  # noqa: E402  (where the reference checkout is)
from noisediff_amd import synth  # noqa: E402

REF = os.path.join(REF_TREE, "test_denoising.py")

tree = ast.parse(open(REF).read())
cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "IlluminanceCorrect")
scope = {"torch": torch, "nn": nn}
exec(compile(ast.Module(body=[cls], type_ignores=[]), REF, "exec"), scope)
corrector = scope["IlluminanceCorrect"]()

shape = (2, 4, 32, 48)
pred = synth.uniform(21, "metrics.pred", shape, -0.2, 1.2)
source = synth.uniform(21, "metrics.source", shape, 0.0, 1.0)
sat = synth.uniform(21, "metrics.sat", shape, 0.0, 1.0) < 0.1
source[sat] = 1.0
source1 = source[1:2].clone()
pred_z = pred.clone()
pred_z[source != 1.0] = -0.5 * pred_z[source != 1.0].abs()          # clamp -> 0 wherever the mask is on

out = {"pred": pred.numpy(), "source": source.numpy(), "source1": source1.numpy(), "pred_z": pred_z.numpy()}
with torch.no_grad():
    out["out.b"] = corrector(pred, source).numpy()
    out["out.b1"] = corrector(pred, source1).numpy()
    out["out.z"] = corrector(pred_z, source).numpy()
assert int(sat.sum()) > 0 and np.isnan(out["out.z"]).all() and np.isfinite(out["out.b"]).all()
np.savez_compressed(os.path.join(HERE, "metrics.npz"), **out)
print({k: v.shape for k, v in out.items()})
