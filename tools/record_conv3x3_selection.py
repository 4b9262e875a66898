"""Record what the conv3x3 kernel rules decide into tests/golden/conv3x3_selection.json (CPU; needs the built library, no GPU).

    python tools/record_conv3x3_selection.py            # rewrite the table from THIS tree's rules
    python tools/record_conv3x3_selection.py --check    # exit status 1 where this tree decides otherwise (no file written)

The table pins three rules: engine.conv3x3_form (inputs -> form, splits, rows per launch; "raise" where it raises), _host.conv3x3_kind (inputs -> kind) and
train.cat_sources_ok.  It was recorded from the tree in which the engine's decision had just been moved into conv3x3_form with every kernel limit still
spelled out in Python; tests/test_host.py holds later trees to it, and evaluates itself the one difference that is allowed (the recorded choice raises, or
the library's nd_conv3x3_takes says the recorded kernel refuses the descriptor).  Re-record only when a rule is meant to change.
"""
from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "conv3x3_selection.json")

BATCHES = (1, 2, 4, 16, 31, 32, 33, 63, 64, 65, 128)
NONE, AFFINE, MAP, GENMAP = 0, 1, 2, 7                       # the prologues the engine puts in front of a 3x3 convolution (enum nd_prologue)
NET_SIZES = ((256, 256), (128, 128), (64, 64), (32, 32), (16, 16))      # the stages of a 256 x 256 and a 128 x 128 patch
SIZES = ((8, 8), (15, 17), (16, 32), (17, 31), (31, 32), (32, 40), (36, 44), (40, 48), (48, 48), (64, 95), (95, 96), (96, 96), (64, 112), (112, 112), (256, 512),
         (512, 512), (16, 2048), (32, 2064), (2048, 16), (2048, 2048), (2064, 2064))
CHANNELS = (8, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128, 256, 512, 1536, 2048, 2052, 4096)
W16 = ("narrow", "all", "0")                                 # ND_WINO4_16; a row holds the index
KNOBS = tuple((sk, w16) for sk in (0, 1) for w16 in (0, 1, 2))
DEFAULT = (0, 0)
# (H, W, cin, cout, c0, c1) whose batches are taken on both sides of every limit: d = 64 and d = 128 at 256 x 256 (plain, concat, the upsampling conv), LSID's 512 x 512
EDGE_LAYERS = ((256, 256, 64, 64, 64, 0), (256, 256, 128, 128, 128, 0), (256, 256, 128, 64, 64, 64), (256, 256, 256, 128, 128, 128), (512, 512, 32, 32, 32, 0),
               (512, 512, 64, 32, 32, 32), (32, 32, 512, 512, 512, 0))


def straddles(H, W, cin, cout, ld):
    """The two batches that straddle each byte / pixel limit of the family at this layer: 2^24 pixels, sources of 1 GiB and 2 GiB, a scale / shift map of
    1 GiB, an output of 4 GiB, 2 GiB written by one launch, split-K partial sums of 2 GiB (2, 4, 8 ranges)."""
    out = set()
    for per_sample, limit in ((H * W, 1 << 24), (H * W * 4 * ld, 1 << 30), (H * W * 4 * ld, 1 << 31), (H * W * 8 * cin, 1 << 30), (H * W * 4 * cout, 1 << 32),
                              (H * W * 4 * cout, 1 << 31), (H * W * 4 * cout * 2, 1 << 31), (H * W * 4 * cout * 4, 1 << 31), (H * W * 4 * cout * 8, 1 << 31)):
        b = limit // per_sample
        out |= {x for x in (b - 1, b, b + 1) if 1 <= x <= 4096}
    return sorted(out)


def form_inputs():
    """(B, H, W, cin, cout, c0, c1, ld0, ld1, mode, upsample, packed4, split_k, wino4_16) rows, in a fixed order without repeats."""
    rows = {}

    def add(B, H, W, cin, cout, c0, c1, ld0=None, ld1=None, mode=NONE, up=0, packed=1, knobs=DEFAULT):
        packed = int(packed and cin > 16 and cin % 4 == 0 and cout % 4 == 0)         # the layers that get the F(4x4) packing (engine._wino4_layer)
        rows[(B, H, W, cin, cout, c0, c1, c0 if ld0 is None else ld0, (c1 if ld1 is None else ld1) if c1 else 0, mode, up, packed, *knobs)] = None

    # the nets at d = 48 / 64 / 128: a stage's block, concat and widening layers; every batch at d = 64, every knob setting at 16 patches
    for d in (48, 64, 128):
        for i, (H, W) in enumerate(NET_SIZES):
            c = d * (1 << min(i, 3))
            for cin, cout, c0, c1 in ((c, c, c, 0), (2 * c, c, c, c), (c + c // 2, c, c, c // 2), (c, 2 * c, c, 0)):
                for B in BATCHES if d == 64 else (1, 16, 33):
                    add(B, H, W, cin, cout, c0, c1, mode=AFFINE if c1 == 0 else NONE)
                for knobs in KNOBS if d == 64 else ((1, 1),):
                    add(16, H, W, cin, cout, c0, c1, knobs=knobs)
                if d == 64:
                    add(16, H, W, cin, cout, c0, c1, packed=0)
                if c1 == 0 and cin == cout:
                    add(16, H, W, cin, cout, c0, 0, mode=AFFINE, up=1)
            for B in (1, 16, 32):                                 # pos_block*.block2.proj: the map prologues at d -> d
                for mode in (MAP, GENMAP):
                    add(B, H, W, d, d, d, 0, mode=mode)
            add(16, H, W, d, d, d, 0, mode=GENMAP, knobs=(1, 1))
            add(16, H, W, d, d, d, 0, mode=MAP, up=1)
    # geometry x channels, thinned: every size with a few widths, every width at one size
    for H, W in SIZES:
        for cin, cout in ((8, 64), (24, 24), (64, 64), (512, 512)):
            for B, knobs in ((16, DEFAULT), (1, (1, 1)), (65, (0, 2))):
                add(B, H, W, cin, cout, cin, 0, mode=AFFINE, knobs=knobs)
        for mode in (NONE, MAP, GENMAP):
            add(2, H, W, 64, 64, 64, 0, mode=mode)
        add(2, H, W, 72, 64, 72, 0, mode=GENMAP)                 # a ragged last chunk: no map formed in the kernel
    for cin in CHANNELS:
        for cout in CHANNELS:
            if cin == cout or cin in (64, 20) or cout in (64, 20):
                add(4, 32, 32, cin, cout, cin, 0)
    # two sources: c0 on and off the 16- and 32-channel boundaries, strides equal to and wider than the channels, with and without upsample
    for c0, c1 in ((8, 24), (16, 16), (16, 32), (24, 40), (32, 32), (48, 16), (64, 64), (512, 256), (20, 12)):
        for H, W in ((32, 32), (36, 44), (256, 256), (16, 16)):
            for knobs in (DEFAULT, (1, 0), (0, 1)):
                add(16, H, W, c0 + c1, 64, c0, c1, knobs=knobs)
            add(1, H, W, c0 + c1, 64, c0, c1, ld0=c0 + 8, ld1=c1 + 16, mode=AFFINE)
            add(64, H, W, c0 + c1, 64, c0, c1, up=1)
            add(16, H, W, c0 + c1, 64, c0, c1, mode=MAP)
    for cin in (32, 64, 128):
        for H, W in ((64, 64), (256, 256), (512, 512)):
            for B in (16, 63, 64):
                add(B, H, W, cin, cin, cin, 0, ld0=2 * cin)
                add(B, H, W, cin, cin, cin, 0, ld0=cin + 4, mode=AFFINE, up=1)
    # both sides of every byte and pixel limit
    for H, W, cin, cout, c0, c1 in EDGE_LAYERS:
        for B in straddles(H, W, cin, cout, max(c0, c1)):
            for mode, knobs in ((NONE, DEFAULT), (AFFINE, (1, 0))) + (((MAP, DEFAULT),) if c1 == 0 and cin == cout else ()):
                add(B, H, W, cin, cout, c0, c1, mode=mode, knobs=knobs)
            if c1 == 0 and cin > 32:
                add(B, H, W, cin, cout, c0, 0, up=1)
    return list(rows)


def kind_inputs():
    """(B, H, W, cin, cout, c0, c1, ld, wino4) rows of _host.conv3x3_kind: train passes ld = c0 + c1, LSID the widest stride."""
    rows = {}
    for H, W in SIZES + NET_SIZES + ((18, 22), (9, 11), (72, 88)):
        for cin, cout in ((8, 32), (64, 64), (512, 256)):
            for B, w4 in ((1, 1), (65, 1), (16, 0)):
                rows[(B, H, W, cin, cout, cin, 0, cin, w4)] = None
        for c0, c1 in ((32, 32), (8, 32), (16, 32), (24, 40)):
            for ld in (c0 + c1, max(c0, c1)):
                rows[(4, H, W, c0 + c1, 32, c0, c1, ld, 1)] = None
            rows[(16, H, W, c0 + c1, 32, c0, c1, c0 + c1, 0)] = None
    for cin in CHANNELS:
        for cout in CHANNELS:
            if cin == cout or cin in (64, 20) or cout in (64, 20):
                rows[(4, 64, 64, cin, cout, cin, 0, cin, 1)] = None
    for H, W, cin, cout, c0, c1 in EDGE_LAYERS:
        for ld in {c0 + c1, max(c0, c1)}:
            for B in straddles(H, W, cin, cout, ld):
                rows[(B, H, W, cin, cout, c0, c1, ld, 1)] = None
    return list(rows)


def cat_inputs():
    """(B, c0, c1, H, W, cout or None) rows of train.cat_sources_ok."""
    rows = {}
    for H, W in ((16, 16), (32, 32), (36, 44), (64, 40), (256, 256), (512, 512), (32, 2064)):
        for c0, c1 in ((32, 32), (16, 16), (8, 32), (32, 8), (16, 48), (256, 256), (24, 40)):
            for B, cout in ((1, None), (16, 32), (16, 20), (16, 2048), (2, 2052)):
                rows[(B, c0, c1, H, W, cout)] = None
    return list(rows)


def decide_form(row):
    from noisediff_amd import _lib as L, engine
    *layer, split_k, w16 = row
    try:
        return list(engine.conv3x3_form(*layer[:10], bool(layer[10]), bool(layer[11]), split_k=bool(split_k), wino4_16=W16[w16]))
    except L.HipError:
        return ["raise", 0, 0]


def decide_kind(row):
    from noisediff_amd._host import conv3x3_kind
    return conv3x3_kind(*row[:8], wino4=bool(row[8]))


def decide_cat(row):
    import torch
    from noisediff_amd import train
    B, c0, c1, H, W, cout = row
    like = lambda c: SimpleNamespace(shape=torch.Size((B, c, H, W)), is_cuda=True, dim=lambda: 4)       # what cat_sources_ok reads of a CUDA tensor
    return bool(train.cat_sources_ok(like(c0), like(c1), cout))


def table():
    return {"form": [[*r, *decide_form(r)] for r in form_inputs()],       # a row: the inputs, then what was decided
            "kind": [[*r, decide_kind(r)] for r in kind_inputs()],
            "cat": [[*r, decide_cat(r)] for r in cat_inputs()]}


def main(argv) -> int:
    new = table()
    print({k: len(v) for k, v in new.items()})
    if "--check" in argv:
        old = json.load(open(PATH))
        diff = [(k, a, b) for k in new for a, b in zip(new[k], old[k]) if a != b]
        for d in diff[:40]:
            print(d)
        print(f"{len(diff)} rows differ")
        return 1 if diff else 0
    with open(PATH, "w") as f:
        per = 8                                              # rows per line of the file
        f.write("{" + ",\n".join(f'"{k}": [\n' + ",\n".join(",".join(json.dumps(r, separators=(",", ":")) for r in v[i:i + per]) for i in range(0, len(v), per)) + "\n]"
                                  for k, v in new.items()) + "}\n")
    print(PATH, os.path.getsize(PATH), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
