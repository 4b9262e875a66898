#!/usr/bin/env python3
"""Generate tests/golden/arch_meta.json from the REAL reference (build container only).

    python tests/golden/capture_arch_meta.py      # writes tests/golden/arch_meta.json

For each network the reference's registry hands to this package (NoiseDiffNet, UNet_PosEmbV2*) at d=16: the reference
class's state-dict (name, shape) list and every 3x3 nn.Conv2d it holds with the attributes that decide whether the training
path takes it (name, in / out channels, stride, padding, dilation, groups, padding mode), plus how many of them
noisediff_amd.train.accelerate took on the reference class itself.  Names and numbers only; nothing of the reference's code."""
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from capture_golden import import_reference  # noqa: E402
from noisediff_amd import train  # noqa: E402
from noisediff_amd.spec import ARCHS  # noqa: E402

_, arch_mod = import_reference()
import models.archs.others_arch as others  # noqa: E402

DIM = 16
out = {"torch": torch.__version__, "dim": DIM}
for name in ARCHS:
    cls = getattr(arch_mod if name == "NoiseDiffNet" else others, name)
    net = cls(SimpleNamespace(dim=DIM, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
    convs = [[n, m.in_channels, m.out_channels, list(m.stride), list(m.padding), list(m.dilation), m.groups, m.padding_mode]
             for n, m in net.named_modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    out[name] = {"state_dict": [[k, list(v.shape)] for k, v in net.state_dict().items()], "conv3x3": convs,
                 "conv3x3_accelerated": train.accelerate(net)}
with open(os.path.join(HERE, "arch_meta.json"), "w") as f:
    json.dump(out, f)
print({k: (len(v["state_dict"]), len(v["conv3x3"]), v["conv3x3_accelerated"]) for k, v in out.items() if isinstance(v, dict)})
