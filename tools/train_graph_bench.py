#!/usr/bin/env python3
"""Training step of TrainableNoiseDiffNet(...).hip() as ONE captured graph (torch.cuda.CUDAGraph): forward + backward + Adam(capturable=True) --
noisediff_amd.train.Adam (one launch + a counter launch; env ADAM=torch: torch.optim.Adam).
The library's launches are queued on torch's current stream, so they are captured like any ATen kernel; replaying the graph removes the host side of the
~300 autograd-function calls of a step (which bounds the small configurations in eager mode).
env ENDS=hip: gd.use_device_rng(1) -- timestep, noising, target, loss and loss gradient on the library too (diffusion_train.hip); REPLAYS=n: timed replays (8).
env EMA=1: train.EMA(net, beta=0.995, update_after_step=500, update_every=20).update() is part of the step (the reference's arguments; EMA_EVERY=1: a
lerp on every step, the upper bound of its cost); LR=tensor: the learning rate is a device tensor (nd_adam_step_capturable_lr_f32), moved with set_lr
between replays."""
import os, sys, time
sys.path.insert(0, os.environ.get("ND_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # ND_PKG_ROOT: another copy of the package (A/B against a saved state)
import torch
from types import SimpleNamespace
from noisediff_amd import GaussianDiffusion, TrainableNoiseDiffNet, synth
from noisediff_amd.train import Adam as HipAdam
dev = torch.device("cuda", 0)
for (B, S) in [(4, 256), (8, 128)]:
    cond = {k: v.to(dev) for k, v in synth.make_condition(B, S, seed=1).items()}
    img = synth.uniform(7, "img", (B, 4, S, S), -1.0, 1.0).to(dev)
    net = TrainableNoiseDiffNet(SimpleNamespace(dim=64)).to(dev).hip(True)
    gd = GaussianDiffusion(net, image_size=S, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(dev)
    if os.environ.get("ENDS") == "hip":
        gd.use_device_rng(1)
    lr = torch.tensor(1e-4, device=dev) if os.environ.get("LR") == "tensor" else 1e-4
    opt = (torch.optim.Adam if os.environ.get("ADAM") == "torch" else HipAdam)(net.parameters(), lr=lr, capturable=True)
    ema = None
    if os.environ.get("EMA") == "1":
        from noisediff_amd.train import EMA
        every = int(os.environ.get("EMA_EVERY", "20"))
        ema = EMA(net, beta=0.995, update_after_step=500 if every > 1 else 0, update_every=every).to(dev)
    def one():
        opt.zero_grad(set_to_none=True)
        loss = gd(img, cond)
        loss.backward()
        opt.step()
        if ema is not None:
            ema.update()
        return loss.detach()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3): one()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5): l = one()
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / 5
    g = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        loss = gd(img, cond)
        loss.backward()
        opt.step()
        if ema is not None:
            ema.update()
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_rep = int(os.environ.get("REPLAYS", "8"))
    for i in range(n_rep):
        if isinstance(lr, torch.Tensor):
            opt.set_lr(1e-4 * (1.0 - 0.01 * i))      # a schedule's fill_ between replays: no new capture
            opt.check_captured_lr()
        g.replay()
    torch.cuda.synchronize()
    graphed = (time.perf_counter() - t0) / n_rep
    print(f"B={B} {S}x{S}: eager {eager * 1e3:.2f} ms/step, one captured graph per step {graphed * 1e3:.2f} ms/step, loss {float(loss.detach()):.6f}", flush=True)
