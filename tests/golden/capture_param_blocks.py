#!/usr/bin/env python3
"""The parameter blocks of the five GPU batch builders, as ``check`` returns them: the bytes a launch reads from the device.

    python tests/golden/capture_param_blocks.py      # writes tests/golden/param_blocks.npz

Host only: no GPU, no built library and no reference checkout are needed.  ``cases()`` lists the parameter sets; tests/test_param_blocks.py runs the
same list against the code under test and compares every block bit for bit, so a field that moves shows.  Capture from a commit whose blocks are
known to be right (the GPU golden tests of the three modules pass on it).

The sets: B = 1 and B = 3; ratio, k and var as one value and per sample; flip as None, one int and (B,); a seed above 2**63 (the uint64 -> int64
view); first_sample and draw nonzero; the generation builder with and without dark_frame; the denoise builder with and without wb / K (its
``use_sna`` flag is stored as ``<name>.use_sna``).  No dark-shading rows: a ``DarkShading`` lives on a GPU, and the GPU golden tests cover them."""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 64, 96)                                               # the frames' (N, H2, W2): packed 32 x 48
SEED = (1 << 63) + (5 << 32) + 7
XY = {1: [(3, 5)], 3: [(0, 0), (31, 15), (32, 16)]}               # crop 16: an odd origin and the far corner
CROP_XY = {1: [(64, 0)], 3: [(0, 0), (2, 62), (64, 64)]}          # crop 64 in patch 128
ISO = {1: [800], 3: [800, 1600, 3200]}                            # at, below and above the high-ISO threshold
RATIO = {1: [100.0], 3: [100.0, 250.0, 300.0]}
WB = {1: [[0.1, 0.2, 0.3, 0.2]], 3: [[0.1, 0.2, 0.3, 0.2], [0, 0, 0, 0], [1.0, 0.5, 0.25, 0.5]]}


def cases():
    """[(name, builder, args, kwargs)]: ``builder.check(*args, **kwargs)`` is the block stored as ``name``."""
    from noisediff_amd import denoise_data as dd, diffusion_data as df, raw
    out = []
    for B in (1, 3):
        frame, other = [b % 2 for b in range(B)], [(b + 1) % 2 for b in range(B)]
        flips = {"none": None, "one": 1, "each": [b % 2 for b in range(B)][::-1]}
        key = dict(seed=SEED, first_sample=3, draw=2)
        for fname, flip in flips.items():
            out.append((f"real.B{B}.flip_{fname}", raw.RealBatchBuilder(crop=16), (B, SHAPE),
                        dict(short=frame, long=other, xy=XY[B], iso=ISO[B], ratio=RATIO[B], flip=flip)))
            out.append((f"pg.B{B}.flip_{fname}", raw.PoissonGaussianBatchBuilder(crop=16), (B, SHAPE),
                        dict(frame=frame, xy=XY[B], ratio=RATIO[B], k=[0.76, 24.5, 3.0][:B], var=[2.5, 0.0, 7.0][:B], flip=flip, **key)))
            out.append((f"denoise.B{B}.flip_{fname}", dd.BatchBuilder(crop=64, patch=128), (B,),
                        dict(xy=XY[B], iso=ISO[B], ratio=RATIO[B], crop_xy=CROP_XY[B], flip=flip, wb=WB[B], K=[0.7, 3.0, 1.5][:B], **key)))
        out.append((f"real.B{B}.scalar", raw.RealBatchBuilder(crop=16, black=500, white=16000), (B, SHAPE),
                    dict(short=frame, long=other, xy=XY[B], iso=ISO[B], ratio=250)))
        out.append((f"pg.B{B}.scalar", raw.PoissonGaussianBatchBuilder(crop=16), (B, SHAPE), dict(frame=frame, xy=XY[B], ratio=100, k=0.76, var=2.5)))
        out.append((f"denoise.B{B}.no_sna", dd.BatchBuilder(crop=64, patch=128), (B,),
                    dict(xy=XY[B], iso=ISO[B], ratio=RATIO[B], crop_xy=CROP_XY[B], seed=9, draw=1)))
        out.append((f"denoise.B{B}.scalar_K", dd.BatchBuilder(crop=64, patch=128), (B,),
                    dict(xy=XY[B], iso=ISO[B], ratio=RATIO[B], crop_xy=CROP_XY[B], wb=np.float32(WB[B]), K=0.7, first_sample=1 << 40)))
        out.append((f"diffusion.B{B}", df.DiffusionBatchBuilder(crop=16), (B, SHAPE), dict(short=frame, long=other, xy=XY[B], ratio=RATIO[B])))
        out.append((f"diffusion.B{B}.scalar", df.DiffusionBatchBuilder(crop=16), (B, SHAPE), dict(short=frame, long=other, xy=XY[B], ratio=300)))
        out.append((f"generation.B{B}", df.GenerationBatchBuilder(crop=16), (B, SHAPE), dict(frame=frame, xy=XY[B])))
        out.append((f"generation.B{B}.dark", df.GenerationBatchBuilder(crop=16, dark_frame=True), (B, (32, 48)), dict(frame=None, xy=XY[B])))
    return out


def blocks():
    """{name: block} of every case, and {name.use_sna: flag} for the denoise builder."""
    out = {}
    for name, builder, args, kwargs in cases():
        got = builder.check(*args, **kwargs)
        if isinstance(got, tuple):
            got, out[name + ".use_sna"] = got[0], np.bool_(got[1])
        out[name] = got
    return out


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = blocks()
    path = os.path.join(HERE, "param_blocks.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:      # np.savez_compressed at the highest level
        for k, v in out.items():
            with zf.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    print({k: (v.dtype, v.shape) for k, v in out.items()})
    print("bytes", os.path.getsize(path))
