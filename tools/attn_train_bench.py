#!/usr/bin/env python3
"""Times of training the attention modules on the HIP library against the PyTorch expressions they replace.

    python tools/attn_train_bench.py core                    # (a) forward + backward of the two cores, library and PyTorch alternating in one run
    python tools/attn_train_bench.py step                    # (b) one training step, eager and as a captured graph, of the package ND_PKG_ROOT names (default: this tree)
    python tools/attn_train_bench.py ab /path/to/parent      # (b) `step` of this tree and of a copy of the parent commit's package, alternating, each in a fresh process

HIP events, every shape warmed, the median of REPEATS (>= 30) timed repeats; `ab` runs each side ROUNDS times so that the spread of a repeated run shows."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ND_PKG_ROOT") or REPO)      # ND_PKG_ROOT: another copy of the package (A/B against a saved state)
REPEATS, ROUNDS = 30, 2


def _median_ms(fn, repeats=REPEATS, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _torch_full(qkv, heads):
    """The parent's expression (trainable._Ops.attention before the library path)."""
    import torch.nn.functional as F
    b, _, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, -1, h * w).transpose(-1, -2) for t in qkv.chunk(3, dim=1))
    return F.scaled_dot_product_attention(q, k, v).transpose(-1, -2).reshape(b, -1, h, w)


def _torch_linear(qkv, heads):
    """The parent's expression (trainable._Ops.linear_attention before the library path)."""
    import torch
    b, _, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, -1, h * w) for t in qkv.chunk(3, dim=1))
    q = q.softmax(dim=-2) * (q.shape[2] ** -0.5)
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(b, -1, h, w)


def core():
    import torch
    from noisediff_amd import synth, train
    dev = torch.device("cuda", 0)
    heads, B = 4, 4
    cases = [("full", 32, 32, train.attention_core, _torch_full)] + [("linear", s, s, train.linear_attention_core, _torch_linear) for s in (256, 128, 64)]
    for kind, H, W, lib_fn, torch_fn in cases:
        qkv = synth.normal(3, f"bench.qkv.{kind}.{H}", (B, 3 * heads * 32, H, W)).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        dout = synth.normal(3, f"bench.dout.{kind}.{H}", (B, heads * 32, H, W)).to(dev).contiguous(memory_format=torch.channels_last)

        def run(fn):
            def one():
                out = fn(qkv, heads)
                torch.autograd.grad(out, qkv, dout)
            return one
        res = {"library": [], "pytorch": []}
        for _ in range(ROUNDS):                                          # the two versions alternate
            res["library"].append(_median_ms(run(lib_fn)))
            res["pytorch"].append(_median_ms(run(torch_fn)))
        print(json.dumps({"bench": "core", "kind": kind, "B": B, "N": H * W, "heads": heads, "repeats": REPEATS,
                          **{f"{k}_median_min_max_ms": [[round(x, 4) for x in r] for r in v] for k, v in res.items()}}), flush=True)


def step():
    import torch
    from types import SimpleNamespace
    from noisediff_amd import GaussianDiffusion, TrainableNoiseDiffNet, synth
    from noisediff_amd.train import Adam as HipAdam
    dev = torch.device("cuda", 0)
    B, S = 4, 256
    for kw in (dict(dim=64, stage_attn=True), dict(dim=128, mid_attn=True)):
        cond = {k: v.to(dev) for k, v in synth.make_condition(B, S, seed=1).items()}
        img = synth.uniform(7, "img", (B, 4, S, S), -1.0, 1.0).to(dev)
        net = TrainableNoiseDiffNet(SimpleNamespace(**kw)).to(dev).hip(True)
        gd = GaussianDiffusion(net, image_size=S, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(dev)
        opt = HipAdam(net.parameters(), lr=1e-4, capturable=True)

        def one():
            opt.zero_grad(set_to_none=True)
            loss = gd(img, cond)
            loss.backward()
            opt.step()

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                one()
        torch.cuda.current_stream().wait_stream(s)
        eager = _median_ms(one)
        g = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g):
            loss = gd(img, cond)
            loss.backward()
            opt.step()
        graphed = _median_ms(g.replay)
        print(json.dumps({"bench": "step", "package": "ND_PKG_ROOT copy" if os.environ.get("ND_PKG_ROOT") else "this tree", "net": kw, "B": B, "size": S, "repeats": REPEATS,
                          "eager_median_min_max_ms": [round(x, 3) for x in eager], "graph_median_min_max_ms": [round(x, 3) for x in graphed]}), flush=True)
        del g, opt, gd, net
        torch.cuda.empty_cache()


def ab(parent_root):
    for _ in range(ROUNDS):
        for root in (None, parent_root):                                 # this tree, the parent's copy, this tree, ...: each in a fresh process
            env = dict(os.environ)
            env.pop("ND_PKG_ROOT", None)
            if root:
                env["ND_PKG_ROOT"] = os.path.abspath(root)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "step"], env=env, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"step failed for {root or 'this tree'} with status {r.returncode}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "core"
    if mode == "core":
        core()
    elif mode == "step":
        step()
    elif mode == "ab" and len(sys.argv) > 2:
        ab(sys.argv[2])
    else:
        raise SystemExit(__doc__)
