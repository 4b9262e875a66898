"""The zero-edit overlay (noisediff_amd/dropin.py): the reference's import names resolve to this package's classes.

Two checks:
  * in a fresh interpreter (the overlay patches the import system), a miniature tree with the reference's LAYOUT
    (models/modules.py-style registry scanning archs/*_arch.py by suffix, a script importing
    `from models.denoising_diffusion_pytorch import GaussianDiffusion`) written by this test;
  * the classes the overlay rebinds, against the recorded shape of the reference's own classes (tests/golden/arch_meta.json).
"""
import json
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import torch

from noisediff_amd import dropin, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(code, cwd, *args):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_overlay_on_a_tree_with_the_reference_layout(tmp_path):
    root = tmp_path / "tree"
    (root / "models" / "archs").mkdir(parents=True)
    (root / "models" / "__init__.py").write_text("")
    (root / "models" / "archs" / "__init__.py").write_text("")
    (root / "models" / "archs" / "Diffusion_arch.py").write_text(
        "import torch.nn as nn\nclass NoiseDiffNet(nn.Module):\n    def __init__(self, args):\n        super().__init__()\n        self.tag = 'tree'\n"
        "class Unrelated(nn.Module):\n    pass\n")
    (root / "models" / "denoising_diffusion_pytorch.py").write_text("raise ImportError('the overlay must answer this name')\n")
    (root / "models" / "modules.py").write_text(textwrap.dedent("""
        import importlib, os
        folder = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'archs')
        mods = [importlib.import_module('models.archs.' + f[:-3]) for f in sorted(os.listdir(folder)) if f.endswith('_arch.py')]
        def define_network(args):
            for m in mods:
                c = getattr(m, args.net_name, None)
                if c is not None:
                    return c(args)
            raise ValueError(args.net_name)
    """))
    (root / "run_me.py").write_text(textwrap.dedent("""
        import sys
        from types import SimpleNamespace
        from models.modules import define_network
        from models.denoising_diffusion_pytorch import GaussianDiffusion
        a = SimpleNamespace(net_name='NoiseDiffNet', dim=16, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False, phase=sys.argv[1])
        net = define_network(a)
        gd = GaussianDiffusion(net, image_size=32, timesteps=10, beta_schedule='sigmoid2') if sys.argv[1] == 'test' else None
        print('RESULT', type(net).__module__, type(net).__name__, GaussianDiffusion.__module__, sys.argv[1:], gd is not None and gd.num_timesteps)
    """))
    out = _run("from noisediff_amd import dropin; dropin.main()", str(tmp_path), str(root / "run_me.py"), "test", "--flag")
    assert "RESULT noisediff_amd.net NoiseDiffNet noisediff_amd.diffusion ['test', '--flag'] 10" in out
    out = _run("from noisediff_amd import dropin; dropin.main()", str(tmp_path), str(root / "run_me.py"), "train")
    assert "RESULT models.archs.Diffusion_arch NoiseDiffNet noisediff_amd.diffusion ['train'] False" in out



def test_overlay_classes_match_the_reference_classes_they_replace():
    """Against the reference classes as tests/golden/capture_arch_meta.py recorded them at d=16, for every class the overlay rebinds: the HIP
    network the registry hands out for inference has the reference class's state dict, name for name and shape for shape (a checkpoint trained
    on the reference class loads unchanged), and the training path takes every 3x3 convolution the reference class holds."""
    import noisediff_amd
    with open(os.path.join(REPO, "tests", "golden", "arch_meta.json")) as f:
        meta = json.load(f)
    for name in dropin.HIP_CLASSES:
        ref = meta[name]
        net = getattr(noisediff_amd, name)(SimpleNamespace(dim=meta["dim"], cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
        assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == ref["state_dict"], name
        shapes = dict((k, v) for k, v in ref["state_dict"])
        convs = torch.nn.ModuleList()
        for conv, cin, cout, stride, padding, dilation, groups, mode in ref["conv3x3"]:
            assert shapes[conv + ".weight"] == [cout, cin // groups, 3, 3], (name, conv)
            convs.append(torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=padding, dilation=dilation, groups=groups, padding_mode=mode))
        assert len(convs) > 20 and train.accelerate(convs) == len(convs), name
