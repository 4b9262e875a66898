#!/usr/bin/env python3
"""The calibration rows tests/test_physics_noise.py feeds noisediff_amd.physics_noise.CameraNoiseModel: four ISO rows of the SID camera.

    python tests/golden/capture_physics_params.py      # writes tests/golden/physics_params.json

The rows are read out of the dict literal of ``get_camera_noisy_params_max`` (utils/raw_util.py) with ``ast``: the reference is parsed, not
imported, as capture_raw.py does (its module imports ``rawpy``).  The fixture holds settings only: per ISO the numbers ``Kmax, lam, sigGs,
sigGssig, sigTL, sigTLsig, sigR, sigRsig, bias, biassig, q, wp, bl``."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from capture_golden import REF as REF_TREE  # noqa: E402  (where the reference checkout is)

CAMERA, ISOS = "SonyA7S2", (100, 1600, 3200, 25600)


def rows():
    tree = ast.parse(open(os.path.join(REF_TREE, "utils", "raw_util.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_camera_noisy_params_max")
    literal = next(n.value for n in fn.body if isinstance(n, ast.Assign) and isinstance(n.value, ast.Dict))
    table = ast.literal_eval(literal)
    return {str(iso): {k: float(v) for k, v in table[f"{CAMERA}_{iso}"].items()} for iso in ISOS}


if __name__ == "__main__":
    out = os.path.join(HERE, "physics_params.json")
    with open(out, "w") as f:
        json.dump({"camera": CAMERA, "rows": rows()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)
