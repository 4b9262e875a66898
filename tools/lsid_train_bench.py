#!/usr/bin/env python3
"""LSID training step on one MI355X (train_denoising.py, script.sh:17: B = 4, 256 x 256 crops, L1 loss, Adam): prints ONE JSON line with

    hip_eager_ms      TrainableLSID(...).hip(), forward + L1 + backward + train.Adam, launched eagerly
    hip_graph_ms      the same step captured once into a torch.cuda.graph (train.Adam(capturable=True)) and replayed
    hip_graph_loss_ms the captured step with net.loss(noisy, clean) -- network and L1 loss as one Function -- in place of F.l1_loss(net(noisy), clean)
    torch_ms          TrainableLSID without .hip() (PyTorch's own ROCm kernels) + torch.optim.Adam on the same GPU
    hip_vs_torch      torch_ms / hip_graph_ms (> 1: the library path is faster)

    timeout -k 10 900 python tools/lsid_train_bench.py [--steps 20] [--warmup 5] [--batch 4] [--size 256]

Times are CUDA-event spans over `steps` steps after `warmup` steps, divided by `steps`.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("ND_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # ND_PKG_ROOT: another copy of the package (A/B against a saved state)
from noisediff_amd import TrainableLSID, synth, train  # noqa: E402


def _time(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--wino4-forward", type=int, choices=(0, 1), default=None, help="A/B: F(4x4) kernels for the forward convolutions (default: the module's)")
    args = ap.parse_args()
    if args.wino4_forward is not None:
        from noisediff_amd import lsid_train
        lsid_train.WINO4_FORWARD = bool(args.wino4_forward)
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    x = synth.uniform(21, "bench.x", (B, 4, S, S), 0.0, 1.0).to(dev)
    y = synth.uniform(21, "bench.y", (B, 4, S, S), 0.0, 1.0).to(dev)

    def stepper(net, opt, fused=False):
        def step():
            opt.zero_grad(set_to_none=True)
            loss = net.loss(x, y) if fused else F.l1_loss(net(x), y)
            loss.backward()
            opt.step()
            return loss
        return step

    def captured_ms(fused: bool) -> float:
        """The step captured by torch's recipe (warm-up steps on a side stream, then the capture), replayed."""
        net = TrainableLSID().to(dev).hip()
        opt = train.Adam(net.parameters(), lr=1e-4, capturable=True)
        step = stepper(net, opt, fused)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g, capture_error_mode="relaxed"):    # (train.Adam stages its pointer table through pinned host memory)
            (net.loss(x, y) if fused else F.l1_loss(net(x), y)).backward()
            opt.step()
        return _time(g.replay, args.steps, args.warmup)

    from noisediff_amd import lsid_train
    out = {"workload": f"LSID train step, B={B}, {S}x{S}, L1, Adam", "steps": args.steps, "warmup": args.warmup, "wino4_forward": lsid_train.WINO4_FORWARD}
    out["hip_graph_ms"] = captured_ms(False)
    out["hip_graph_loss_ms"] = captured_ms(True)

    net = TrainableLSID().to(dev).hip()
    out["hip_eager_ms"] = _time(stepper(net, train.Adam(net.parameters(), lr=1e-4)), args.steps, args.warmup)

    net = TrainableLSID().to(dev)
    out["torch_ms"] = _time(stepper(net, torch.optim.Adam(net.parameters(), lr=1e-4)), args.steps, args.warmup)
    out["hip_vs_torch"] = out["torch_ms"] / out["hip_graph_ms"]
    out["gflop_per_step_estimate"] = 290
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
