#!/usr/bin/env python3
"""Golden vectors for LSID training (train_denoising.py, script.sh:17): loss and parameter gradients of the REAL reference
LSID in train mode (build container only).  Writes tests/golden/lsid_train.npz; weights, inputs and targets come from
noisediff_amd.synth, results only are stored."""
import os, sys
from types import SimpleNamespace
import numpy as np
import torch
from torch import nn
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")
from noisediff_amd import synth
from noisediff_amd.spec import lsid_param_spec
import models.archs.SID_arch as sid

sys.path.insert(0, os.path.join(REPO, "tests"))
from util import sub

CASES = ((2, 64, 64), (1, 36, 44))      # the second size exercises ceil-mode pooling (18x22, 9x11, 5x6, 3x3) and the crop
LOSSES = {"l1": nn.L1Loss, "mse": nn.MSELoss}
torch.set_num_threads(4)
out = {}
for (B, H, W) in CASES:
    x = synth.uniform(11, f"lsid_train.x.{H}x{W}", (B, 4, H, W), 0.0, 1.0)
    y = synth.uniform(11, f"lsid_train.y.{H}x{W}", (B, 4, H, W), 0.0, 1.0)
    for lname, lcls in LOSSES.items():
        net = sid.LSID(SimpleNamespace()).train()
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(p.name, p.shape) for p in lsid_param_spec()]
        net.load_state_dict(synth.make_state_dict(lsid_param_spec(), 0), strict=True)
        loss = lcls()(net(x), y)
        loss.backward()
        key = f"{lname}.{H}x{W}"
        grads = {k: p.grad for k, p in net.named_parameters()}
        out[f"{key}.loss"] = np.array(float(loss.detach()))
        out[f"{key}.grad_sq_norm"] = np.array(sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None))
        out[f"{key}.n_params_with_grad"] = np.array(sum(1 for g in grads.values() if g is not None))
        for k, g in grads.items():
            out[f"{key}.grad.{k}"] = sub(g, 2048)
np.savez_compressed(os.path.join(HERE, "lsid_train.npz"), **out)
print(len(out), {k: float(v) for k, v in out.items() if v.ndim == 0})
