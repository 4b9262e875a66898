#!/usr/bin/env python3
"""bench.py -- sampled RAW patches / second on the NoiseDiff sampling hot path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W]          # N=1: one process; N>1: starts N rank processes itself
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` (no WORLD_SIZE in the environment) starts N fresh child processes -- one per GPU, RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1 -- BEFORE this process touches the GPU, relays rank 0's
JSON line and exits non-zero if any rank fails: one command starts all GPUs, as the reference's nn.DataParallel entry
does (models/modules.py:73-83).  Under torch.distributed.run the ranks already exist and nothing is spawned.

Workload (BASELINE.json: "256x256x4, 1000-step DDPM", configs[2] per-GPU shard): NoiseDiffNet
dim=64, sigmoid2 / pred_v, 16 patches of 256x256x4 per GPU.  A *step* is one reverse-diffusion
step over the whole per-GPU batch: the captured graph [write t -> time MLP -> U-Net forward ->
fused posterior/noise update -> advance] -- the unit the 1000-step sampler repeats 1000 times with
identical cost.  K steps are timed after W warm-up steps; one sampled patch = T = 1000 such steps, so
    value = n_gpus * batch_per_gpu / (T * seconds_per_step)       [patches/s, whole job].
`--sample-calls` instead times complete 1000-step .sample() calls (K = number of calls).
The W + K steps are the first steps of one sample (seed 1), started again should they run past its last step, so that the same
arguments time the same steps; `--dump-outputs DIR` writes what the last of them returned -- x_t after it and the network output
(`--sample-calls`: the last sample() call's result) -- as DIR/<name>.npy, float32, for comparing two builds output for output.

A plain run does only what the headline needs: set-up, the untimed soak, the W warm-up and K timed steps, the dump, the JSON line.
`--full` adds, behind the timed steps: `full_sample` (N = 1), one complete sample() call timed on the host clock; `roofline`
(rank 0) for the dominant kernel family (conv3x3: exact-fp32 MFMA bound) measured with HIP events on the library's stream in a
separate instrumented pass over the same steps; and `cpu_baseline` (N = 1): the CPU oracle's p_sample step timed on this box's
host cores.  `--no-full-sample`, `--no-roofline` and `--no-cpu` leave one of them out.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 == FP32 vector peak
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20,
                    help="timed sampler steps; should warm-up + steps run past the sampler's last step, the sample is started again inside the "
                         "timed window (one host synchronisation each, counted as config.sample_restarts_timed on the JSON line)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16, help="patches per GPU (weak scaling)")
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--sampling-timesteps", type=int, default=None, help="DDIM steps (default: DDPM over all timesteps)")
    ap.add_argument("--mid-attn", action="store_true", help="Attention between the mid blocks (BASELINE config 4 extension)")
    ap.add_argument("--config", choices=["cfg2", "cfg3", "cfg4", "ref48"], default=None,
                    help="BASELINE.json presets: cfg2 d64/128x128/B16 DDPM; cfg3 (default workload) d64/256x256/B16 per GPU DDPM; "
                         "cfg4 d128 + mid attention/256x256/B8 per GPU/250-step DDIM")
    ap.add_argument("--sample-calls", action="store_true", help="time whole 1000-step sample() calls instead of K steps")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: one complete sample() call, the roofline pass and the CPU baseline")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline pass")
    ap.add_argument("--eager", action="store_true", help="launch kernels one by one instead of replaying the hipGraph")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl == RCCL on ROCm; gloo for plumbing tests)")
    ap.add_argument("--one-device", action="store_true", help="testing only: every rank uses cuda:0 (single-GPU box)")
    ap.add_argument("--broadcast", choices=["weights", "plan-slices", "arena"], default="weights",
                    help="what the one collective carries: the raw fp32 weights (every rank packs its arena), the packed slices the plan reads, the whole packed arena")
    ap.add_argument("--soak-s", type=float, default=3.0, help="seconds of untimed step replays before the W warm-up steps")
    ap.add_argument("--no-full-sample", action="store_true", help="with --full: skip the one complete sample() call timed behind the K-step leg (N = 1 only)")
    ap.add_argument("--no-alt", action="store_true", help="accepted and ignored (r4 timed a second product form here; there is one form since r5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step (or, with --sample-calls, the last sample() call) returned as DIR/<name>.npy")
    return ap.parse_args()


DUMP_BYTES = 64_000_000


def dump_outputs(dirname, arrays, budget=DUMP_BYTES):
    """Write every tensor of `arrays` as DIR/<name>.npy in float32, `budget` bytes in all at most (each of N ranks writing into the same DIR
    gets DUMP_BYTES / N): a tensor larger than its share is written as the elements at fixed flat indices (drawn from a generator seeded
    with 0, ascending), the same ones for every run of the same shapes.  Returns {name: {"shape", "elements_written"}} for the JSON line."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    share = (budget // len(arrays) - 4096) // 4              # elements per array; 4096 bytes left for each .npy header
    info = {}
    for name, t in arrays.items():
        v = t.detach().to("cpu", torch.float32).numpy()
        if v.size > share:
            v = v.reshape(-1)[np.unique(np.random.default_rng(0).integers(0, v.size, share))]
        np.save(os.path.join(dirname, name + ".npy"), v)
        info[name] = {"shape": list(t.shape), "elements_written": int(v.size)}
    return info


def _pmc_profile(kind):
    """(path, stale): the profiles/r*_<kind>.json (written by tools/pmc_*.py on the GPU box) that was measured on THIS tree's kernel sources -- the files carry
    the git blob ids of conv3x3_wino4.hip / pointwise.hip / pwchain.hip / norm.hip at the time of the PMC pass -- or, when no summary matches, the last one by
    name, marked stale (the figures cited on the line must be tied to the build that is benchmarked)."""
    import glob
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from source_blobs import source_blobs
    mine = source_blobs(REPO)
    files = sorted(glob.glob(os.path.join(REPO, "profiles", f"r*_{kind}.json")))
    for f in reversed(files):
        try:
            if json.load(open(f)).get("source_blobs") == mine:
                return f, False
        except (OSError, ValueError):
            continue
    return (files[-1], True) if files else ("", True)


def conv_flops(m):
    return 18.0 * m["cin"] * m["cout"] * m["H"] * m["W"] * m["B"]          # 2 * 9 * Cin * Cout per output pixel


def conv_bytes(m):
    return 4.0 * m["B"] * m["H"] * m["W"] * (m["cin"] + m["cout"]) + 4.0 * (9 * m["cin"] * m["cout"] + m["cout"])


def executed_gflop_per_step(plan, L):
    """MFMA FLOPs one replay of the step graph EXECUTES (GFLOP): 3x3 convolutions at their kernel's Winograd multiply count, 1x1
    layers / fused chains / the 7x7 stem / attention at 2 MACs per weight use -- what the matrix pipe works off per step, as
    opposed to SURVEY 8d's algorithmic count of the reference's graph."""
    tot = 0.0
    for fn, args, name, meta in plan.step_ops:
        if not meta:
            if name == "nd_conv7x7_c4_f32":
                tot += 2.0 * 196 * plan.e.dim * plan.B * plan.H * plan.W
            elif name == "nd_attention_mfma_f32":
                B_, N, heads, dh = args[4], args[5], args[6], args[7]
                tot += 4.0 * heads * N * N * dh * B_
            continue
        if "tiling" in meta:
            tot += conv_flops(meta) / WINO_FACTOR.get(meta["tiling"], 1.0)
        elif "flop_per_px" in meta:
            tot += meta["flop_per_px"] * meta["B"] * meta["HW"]
        elif "HW" in meta and "cin" in meta:
            tot += 2.0 * meta["cin"] * meta["cout"] * meta["B"] * meta["HW"]
    return tot / 1e9


def instrumented_pass(loop, plan, L, n_steps):
    """Eager replay of n_steps with a HIP event pair around every conv3x3 launch (library stream)."""
    st = plan.e.stream
    CONV = ("nd_conv3x3_nhwc_f32", "nd_conv3x3_wino_nhwc_f32", "nd_conv3x3_wino2_nhwc_f32", "nd_conv3x3_wino4_nhwc_f32", "nd_conv3x3_wino4_16_nhwc_f32",
            "nd_conv3x3_wino4_16_splitk_nhwc_f32", "nd_conv3x3_wino4_splitk_nhwc_f32")
    STREAM = "nd_affine_silu_add_f32"           # the HBM-bound family: GroupNorm-apply + SiLU + residual adds, one pass
    convs = [op for op in plan.step_ops if op[2] in CONV or (op[2] == STREAM and op[3])]
    n_ev = 2 * len(convs)
    evs = []
    for _ in range(n_ev):
        e = C.c_void_p()
        L.call("nd_event_create", C.byref(e))
        evs.append(e)
    per = {}
    for _ in range(n_steps):
        L.call("nd_sampler_begin_step", C.byref(loop.state), st)
        i = 0
        for fn, args, name, meta in plan.step_ops:
            if name in CONV or (name == STREAM and meta):
                L.call("nd_event_record", evs[2 * i], st)
                L.check(fn(*args), name)
                L.call("nd_event_record", evs[2 * i + 1], st)
                i += 1
            else:
                L.check(fn(*args), name)
        fnname = "nd_sampler_step_ddim_f32" if loop.gd.is_ddim_sampling else "nd_sampler_step_ddpm_f32"
        e_ = plan.e
        L.call(fnname, plan.x.data_ptr(), plan.model_out.data_ptr(), None, 0, C.byref(loop.state),
               L.OBJECTIVES[loop.gd.objective], C.c_uint64(1), 0, plan.B, plan.H * plan.W, e_.inp_dim, st)
        L.call("nd_sampler_advance", C.byref(loop.state), st)
        L.call("nd_stream_sync", st)
        for j, op in enumerate(convs):
            ms = C.c_float()
            L.call("nd_event_elapsed_ms", evs[2 * j], evs[2 * j + 1], C.byref(ms))
            m = op[3]
            if op[2] == STREAM:
                d = per.setdefault(("stream", 0), {"ms": 0.0, "flop": 0.0, "bytes": 0.0, "launches": 0})
                d["ms"] += ms.value
                d["bytes"] += m["stream_bytes"]
                d["launches"] += 1
                continue
            # conv3x3_wino4 has two instances per prologue mode: outputs of 48 MB and more are stored with the streaming policy bits
            stream = m["tiling"] in (9004, 9016) and 4 * m["B"] * m["H"] * m["W"] * m["cout"] >= int(os.environ.get("ND_W4_STREAM_MB", "48")) << 20
            d = per.setdefault((m["tiling"], m["mode"], stream, m.get("splits", 1) > 1), {"ms": 0.0, "flop": 0.0, "bytes": 0.0, "launches": 0})
            d["ms"] += ms.value
            d["flop"] += conv_flops(m)
            d["bytes"] += conv_bytes(m)
            d["launches"] += 1
    for e in evs:
        L.call("nd_event_destroy", e)
    return per


def _oracle_step_fn(sd, size, timesteps, batch=1):
    from noisediff_amd import synth
    from oracle import noisediff_oracle as O
    cond = synth.make_condition(batch, size, seed=1)
    buf = O.schedule_buffers("sigmoid2", timesteps)
    z = synth.make_noise(2, "noise.0", batch, 4, size)

    def one_step(img, t):
        out = O.noisediff_forward(sd, img, torch.full((batch,), t, dtype=torch.long), cond)
        _, x0 = O.predict_x0_eps(buf, "pred_v", img, t, out, clip=False)
        x0 = x0.clamp(-1, 1)
        mean = float(buf["posterior_mean_coef1"][t]) * x0 + float(buf["posterior_mean_coef2"][t]) * img
        return mean + math.exp(0.5 * float(buf["posterior_log_variance_clipped"][t])) * z

    return one_step, synth.make_noise(2, "x_T", batch, 4, size)


def _time_steps(f, x, timesteps, n_min, budget_s, n_max):
    """Seconds per step: one untimed step, then >= n_min timed steps until budget_s is spent (at most n_max)."""
    x = f(x, timesteps - 1)
    t0 = time.perf_counter()
    n = 0
    while n < n_min or (time.perf_counter() - t0 < budget_s and n < n_max):
        x = f(x, timesteps - 2 - n)
        n += 1
    return (time.perf_counter() - t0) / n, n


def _cpu_limits():
    """What bounds the host leg on this box, so that its number can be read: the affinity mask, the cgroup CPU quota (v2 cpu.max or v1 cfs quota / period:
    a box may show 128 cores and grant 16 cores' worth of time) and the load average while the leg starts."""
    info = {}
    try:
        cpus = sorted(os.sched_getaffinity(0))
        info["affinity_cpus"] = len(cpus)
        info["affinity_range"] = f"{cpus[0]}-{cpus[-1]}" if cpus else ""
    except AttributeError:
        info["affinity_cpus"] = os.cpu_count()
    info["os_cpu_count"] = os.cpu_count()
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q <= 0 else q / per
        except (OSError, ValueError):
            pass
    info["cgroup_cpu_quota_cores"] = quota
    try:
        info["loadavg_1min"] = os.getloadavg()[0]
    except OSError:
        pass
    return info


def cpu_baseline(sd, dim, size, timesteps, batch):
    """The CPU oracle's p_sample step (one U-Net forward + posterior update) on this host's cores.

    The thread count is calibrated AT THE REAL PROBLEM SIZE (a cgroup-limited box thrashes with one thread per visible
    core, and the best count for a 64x64 toy is not the best one for 256x256): every candidate runs one untimed and two
    timed batch-1 steps; the sweep stops early once a candidate is > 1.6x slower than the best so far.  The best count
    is then timed for ~10 s at batch 1 and for >= 2 steps at batch min(B, 4); `value` is the better of the
    two legs in patches/s, extrapolated x T (steps are identical-cost)."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    limits = _cpu_limits()
    cands = sorted({c for c in (8, 16, 32, 48, 64, 96, 128, avail) if c <= avail})
    sweep = {}
    with torch.no_grad():
        f1, x1 = _oracle_step_fn(sd, size, timesteps, 1)
        best, best_dt = cands[0], float("inf")
        for c in cands:
            torch.set_num_threads(c)
            dt, _ = _time_steps(f1, x1, timesteps, 2, 0.0, 2)
            sweep[c] = round(dt, 4)
            if dt < best_dt:
                best, best_dt = c, dt
            elif dt > 1.6 * best_dt:
                break
        torch.set_num_threads(best)
        dt1, n1 = _time_steps(f1, x1, timesteps, 3, 10.0, 40)
        b4 = min(batch, 4)
        legs = {"batch1": {"s_per_step": dt1, "steps": n1, "threads": best, "patches_per_s": 1.0 / (timesteps * dt1)}}
        sweep4 = {}
        if b4 > 1:
            # the batch-4 leg gets its own calibration (r2: the batch-1 count made it 8x slower for 4x the work): one timed step per
            # candidate around the batch-1 optimum, then >= 2 steps with the best
            f4, x4 = _oracle_step_fn(sd, size, timesteps, b4)
            best4, best4_dt = best, float("inf")
            for c in sorted({c for c in (best // 2, best, best * 2, best * 4) if 4 <= c <= avail}):
                torch.set_num_threads(c)
                dt, _ = _time_steps(f4, x4, timesteps, 1, 0.0, 1)
                sweep4[c] = round(dt, 4)
                if dt < best4_dt:
                    best4, best4_dt = c, dt
            torch.set_num_threads(best4)
            dt4, n4 = _time_steps(f4, x4, timesteps, 2, 6.0, 10)
            legs[f"batch{b4}"] = {"s_per_step": dt4, "steps": n4, "threads": best4, "patches_per_s": b4 / (timesteps * dt4)}
    top = max(legs, key=lambda k: legs[k]["patches_per_s"])
    return {"value": legs[top]["patches_per_s"], "unit": "patches/s", "cores": legs[top]["threads"], "kind": "port", "legs": legs, **limits,
            "thread_sweep_s_per_step_batch1": sweep, "thread_sweep_s_per_step_batch4": sweep4,
            "sample": f"CPU oracle p_sample steps (U-Net forward + posterior update) at dim {dim}, {size}x{size}x4 with {legs[top]['threads']} threads "
                      f"(each leg calibrated at this size: batch 1 over {list(sweep)}, batch 4 over {list(sweep4)}; {avail} cores visible): " +
                      "; ".join(f"{k}: {v['steps']} steps, {v['s_per_step']:.3f} s/step" for k, v in legs.items()) +
                      f"; value = best leg ({top}), extrapolated x{timesteps} steps per patch"}


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(a):
    """`python bench.py --gpus N` without a launcher: start N rank processes (fresh interpreters, nothing in THIS process
    has touched the GPU), relay rank 0's JSON line, fail if any rank fails.  torch.cuda.device_count() does not
    initialise the runtime on this image."""
    import subprocess
    n_dev = torch.cuda.device_count()
    if not a.one_device and n_dev < a.gpus:
        print(f"bench.py: --gpus {a.gpus} but only {n_dev} GPU(s) are visible; refusing to report a smaller job as N={a.gpus}",
              file=sys.stderr)
        return 2
    env = dict(os.environ, WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), ND_BENCH_LAUNCHER="self")
    env.setdefault("OMP_NUM_THREADS", "4")
    procs = []
    for r in range(a.gpus):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(a.gpus))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=e,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    out0, rc = "", 0
    try:
        pending = set(range(a.gpus))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if r == 0:
                    out0 = procs[0].stdout.read()
                if code != 0:
                    rc = rc or code
                    print(f"bench.py: rank {r} exited with code {code}", file=sys.stderr)
            if rc:
                break
            time.sleep(0.2)
    finally:
        for p in procs:                      # exact PIDs of the children started above
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
    if rc:
        return rc
    lines = [ln for ln in out0.splitlines() if ln.startswith("{")]
    if not lines:
        print("bench.py: rank 0 produced no JSON line", file=sys.stderr)
        return 3
    print(lines[-1], flush=True)
    return 0


# MFMA multiplies actually issued per algorithmic multiply: Winograd F(2x2,3x3) does 16 per 2x2 outputs x 9 taps = 1/2.25,
# F(4x4,3x3) 36 per 16 x 9 = 1/4; the direct kernel 1.  tiling ids: 9001 wino, 9002 wino2, 9004 wino4 (16 x 32-pixel regions), 9016 wino4 on 16 x 16-pixel
# regions (two workgroups per CU), else direct <TW,MB,NB>
WINO_FACTOR = {9001: 2.25, 9002: 2.25, 9004: 4.0, 9016: 4.0}
UNIT_GFLOP = {(64, 128): 68.78, (64, 256): 275.12, (128, 256): 1077.65,      # algorithmic GFLOP per patch.step (dim, size)
              (48, 512): 627.61}     # the reference's shipped workload (script.sh:10), counted the same way (tools/count_reference_flops.py: conv3x3 527.27)


def roofline(a, loop, plan, L, per_step):
    n_inst = min(max(a.steps, 1), 3)
    per = instrumented_pass(loop, plan, L, n_inst)
    stream = per.pop(("stream", 0), None)
    tot_ms = sum(d["ms"] for d in per.values())
    tot_flop = sum(d["flop"] for d in per.values())
    tot_exec = sum(d["flop"] / WINO_FACTOR.get(k[0], 1.0) for k, d in per.items())
    kname = lambda k: (f"wino2_kernel<{k[1]}>" if k[0] == 9002 else f"wino4_kernel<{k[1]}, {'true' if k[2] else 'false'}, {'true' if len(k) > 3 and k[3] else 'false'}, {1 if k[0] == 9016 else 2}, 4>{' + reduce' if len(k) > 3 and k[3] else ''}" if k[0] in (9004, 9016) else
                       f"wino_kernel<1, {k[1]}, 32>" if k[0] == 9001 else
                       f"conv3x3_kernel<{k[0] // 100}, {(k[0] // 10) % 10}, {k[0] % 10}, {k[1]}>")   # as rocprofv3 prints it
    tid, d = max(per.items(), key=lambda kv: kv[1]["ms"])
    ach = d["flop"] / (d["ms"] * 1e-3) / 1e12
    wf = WINO_FACTOR.get(tid[0], 1.0)
    headline = (a.dim, a.size, a.batch) == (64, 256, 16)
    traffic = tsrc = busy_pmc = bsrc = None
    tfile, tstale = _pmc_profile("traffic")                          # PMC passes cannot run inside this process
    if os.path.exists(tfile) and headline:
        tk = json.load(open(tfile))["kernels"].get(kname(tid))
        if tk:
            traffic = tk["hbm_bytes_per_launch"]
            tsrc = (f"builder box, profiles/{os.path.basename(tfile)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same "
                    "workload) -- NOT measured in this run")
    bfile, bstale = _pmc_profile("mfma_busy")                        # SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8), own PMC pass
    if os.path.exists(bfile) and headline:
        bk = json.load(open(bfile))["kernels"].get(kname(tid))
        if bk:
            busy_pmc = bk["matrix_pipe_busy_frac"]
            bsrc = f"builder box, profiles/{os.path.basename(bfile)} -- NOT measured in this run"
    unit = UNIT_GFLOP.get((a.dim, a.size))
    exec_gf = executed_gflop_per_step(plan, L)
    out = {
        "bound": "mfma", "kernel": kname(tid), "unit": "TFLOP/s", "peak": PEAK_FP32_MFMA_TFLOPS,
        # `achieved` is priced in ALGORITHMIC conv FLOPs (18*Cin*Cout per output pixel) over the event-timed launch
        # duration of THIS run; a Winograd kernel issues `winograd_multiply_reduction` x fewer MFMA FLOPs than that, so the
        # fraction of the fp32 matrix pipe that is actually busy -- the honest roofline fraction -- is `frac`:
        "achieved": ach, "winograd_multiply_reduction": wf, "executed": ach / wf,
        "frac": ach / wf / PEAK_FP32_MFMA_TFLOPS, "algorithmic_frac": ach / PEAK_FP32_MFMA_TFLOPS,
        "frac_definition": "executed MFMA FLOP/s (= achieved / winograd_multiply_reduction) / peak; algorithmic_frac = achieved / peak "
                           "may exceed 1 for Winograd kernels",
        "traffic": traffic, "traffic_measured_on": tsrc, "traffic_stale": None if traffic is None else tstale,
        "matrix_pipe_busy_pmc": busy_pmc, "matrix_pipe_busy_measured_on": bsrc, "matrix_pipe_busy_stale": None if busy_pmc is None else bstale,
        "stale_definition": "true = the PMC summary was measured on kernel sources (git blob ids in the profiles/*.json) that differ from this tree's",
        "avg_launch_ms": d["ms"] / d["launches"], "launches_per_step": d["launches"] // n_inst,
        "algorithmic_flop_per_launch": d["flop"] / d["launches"],
        "algorithmic_bytes_per_launch": d["bytes"] / d["launches"],
        "hbm_frac_at_algorithmic_bytes": d["bytes"] / (d["ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS,
        "all_conv3x3": {"algorithmic_tflops": tot_flop / (tot_ms * 1e-3) / 1e12, "executed_tflops": tot_exec / (tot_ms * 1e-3) / 1e12,
                        "executed_frac": tot_exec / (tot_ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                        "ms_per_step": tot_ms / n_inst, "share_of_step": (tot_ms / n_inst) / (per_step * 1e3) if not a.sample_calls else None},
        "whole_step": None if (unit is None or a.sample_calls) else {
            "algorithmic_gflop_per_patch_step": unit, "algorithmic_tflops": a.batch * unit / per_step / 1e3,
            "algorithmic_frac_of_fp32_peak": a.batch * unit / per_step / 1e3 / PEAK_FP32_MFMA_TFLOPS,
            "executed_gflop_per_step": exec_gf, "executed_tflops": exec_gf / per_step / 1e3,
            "executed_frac": exec_gf / per_step / 1e3 / PEAK_FP32_MFMA_TFLOPS,
            "launches_per_step": sum(1 for op in plan.step_ops if not op[2].startswith(("nd_event_", "nd_stream_"))) + 3,
            "note": "SURVEY 8d module-hook FLOPs of the reference forward (includes the layers the build eliminates algebraically)"},
        "by_kernel": {kname(k): {"algorithmic_tflops": v["flop"] / (v["ms"] * 1e-3) / 1e12,
                                 "executed_frac": v["flop"] / WINO_FACTOR.get(k[0], 1.0) / (v["ms"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                                 "avg_ms": v["ms"] / v["launches"], "launches_per_step": v["launches"] // n_inst}
                      for k, v in sorted(per.items())},
    }
    if stream:
        # the step's HBM-bound family, judged on GB/s: algorithmic bytes (every operand read once, the result written
        # once) over the summed launch time of the same instrumented pass
        gbs = stream["bytes"] / (stream["ms"] * 1e-3) / 1e9
        out["hbm_bound_family"] = {
            "kernel": "affine_silu_add_kernel", "bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": gbs / PEAK_HBM_GBS, "launches_per_step": stream["launches"] // n_inst,
            "ms_per_step": stream["ms"] / n_inst}
    return out


def main():
    a = parse()
    if a.config == "cfg2":
        a.dim, a.size, a.batch = 64, 128, 16
    elif a.config == "cfg4":
        a.dim, a.size, a.batch, a.sampling_timesteps, a.mid_attn = 128, 256, 8, 250, True
    elif a.config == "ref48":        # the reference's own command line (script.sh:10): --dim 48 --crop_size 512 --batch_size 4, 1000-step DDPM
        a.dim, a.size, a.batch = 48, 512, 4
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(launch_ranks(a))            # nothing above this line initialises the GPU
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != a.gpus:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: a line for a different job size than asked would be "
              "misleading; start it as `python bench.py --gpus N` or with --nproc-per-node N", file=sys.stderr)
        sys.exit(2)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if a.one_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)   # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(a.backend)

    from noisediff_amd import GaussianDiffusion, NoiseDiffNet, synth, _lib as L
    from noisediff_amd import engine as E
    from noisediff_amd.engine import Engine
    from noisediff_amd.spec import noisediff_param_spec

    B, S, T = a.batch, a.size, a.timesteps
    net = NoiseDiffNet(SimpleNamespace(dim=a.dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False,
                                       mid_attn=a.mid_attn))
    sd = None
    if rank == 0:
        sd = synth.make_state_dict(noisediff_param_spec(a.dim), 0)      # synthetic weights, PyTorch default-init statistics
        if a.mid_attn:
            from noisediff_amd.spec import attention_param_spec
            sd.update(synth.make_state_dict(attention_param_spec("mid_attn", 8 * a.dim), 0))
        net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    bcast = None
    if world > 1:
        # the ONE collective of the data path: packed weight arena, rank 0 -> everyone, over xGMI
        eng = Engine(a.dim, dev, mid_attn=a.mid_attn)
        torch.cuda.synchronize(dev)
        dist.barrier()
        t0 = time.perf_counter()
        if a.broadcast == "weights":         # the network's own fp32 weights (150 MB at d=64); every rank packs its arena itself
            nbytes = eng.broadcast_state_dict(sd, src=0)
        else:                                # rank 0's packed arena: all of it, or the slices this plan reads
            if rank == 0:
                eng.load_state_dict(sd)
            eng.plan(B, S, S, allow_empty=True)
            nbytes = eng.broadcast(src=0, only_used=a.broadcast == "plan-slices")
        bt = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        eng.plan(B, S, S)
        net.adopt_engine(eng)
        # evidence that every rank holds rank 0's weights: min and max over ranks of a checksum of the arena
        cs = torch.stack([eng.view(n).double().abs().sum() for n in sorted(eng.used)]).sum().reshape(1)   # over the slices the plan reads
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(bt, op=dist.ReduceOp.MAX)
        bcast = {"ranks_in_broadcast": dist.get_world_size(), "backend": dist.get_backend() + (" (RCCL)" if a.backend == "nccl" else ""),
                 "broadcast_carries": a.broadcast, "broadcast_bytes": nbytes, "arena_bytes": eng.arena.numel() * 4, "broadcast_and_pack_ms": float(bt.item()) * 1e3,
                 "arena_checksum_equal_on_all_ranks": bool(lo.item() == hi.item() and hi.item() > 0),
                 "per_step_collectives": 0, "devices": "all ranks on cuda:0 (--one-device rehearsal)" if a.one_device else
                 f"one GPU per rank (cuda:0..{world - 1})",
                 "launcher": "bench.py started the ranks itself" if os.environ.get("ND_BENCH_LAUNCHER") == "self" else
                 "external (torch.distributed.run)"}
    gd = GaussianDiffusion(net, image_size=S, timesteps=T, sampling_timesteps=a.sampling_timesteps, beta_schedule="sigmoid2",
                           objective="pred_v").to(dev)
    n_sample_steps = a.sampling_timesteps or T
    gd.sample_offset = rank * B
    cond = synth.make_condition(B, S, seed=1, first_sample=rank * B, total=world * B)
    plan = net.hip_engine(dev).plan(B, S, S)
    plan.set_condition({k: v.to(dev) for k, v in cond.items()})

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    soak_steps, timed_restarts, own_restarts = 0, None, None
    if a.sample_calls:
        kw = dict(batch_size=B, condition={k: v.to(dev) for k, v in cond.items()})
        for _ in range(a.warmup):
            gd.sample(seed=1, **kw)
        barrier()
        t0 = time.perf_counter()
        for i in range(a.steps):
            last = gd.sample(seed=2 + i, **kw)
        plan.e.sync()
        barrier()
        dt = time.perf_counter() - t0
        per_step = dt / a.steps
        value = world * B / per_step
        loop = next(iter(gd._loop_cache.values()))
    else:
        from noisediff_amd.diffusion import _Loop
        loop = _Loop(gd, plan)
        start = lambda: loop.start(None, None, seed=1, first_sample=rank * B, use_graph=not a.eager)
        start()
        # untimed soak before the W warm-up steps: the chip reaches the clocks / temperature it holds over a 1000-step
        # sample() (fp32 MFMA load throttles to ~2.1 GHz after the first second), and an outside utilisation probe sees the job
        t_soak = time.perf_counter()
        while a.soak_s > 0 and time.perf_counter() - t_soak < a.soak_s:
            loop.advance(10)
            plan.e.sync()
            soak_steps += 10
        # the soak is a time, not a number of steps: the warm-up and timed steps begin a fresh sample, so that they are the same steps on every run
        start()
        done = 0

        def run_steps(n):
            """n steps of the sampler; a sample that has taken its last step is started again (a step past the last one skips the update).
            Returns the number of restarts: each synchronises the host with the device (Loop.start)."""
            nonlocal done
            restarts = 0
            while n:
                if done == loop.n_steps:
                    start()
                    done, restarts = 0, restarts + 1
                k = min(n, loop.n_steps - done)
                loop.advance(k)
                done, n = done + k, n - k
            return restarts

        run_steps(a.warmup)
        plan.e.sync()
        barrier()
        t0 = time.perf_counter()
        timed_restarts = run_steps(a.steps)
        plan.e.sync()
        barrier()
        dt = time.perf_counter() - t0
        per_step = dt / a.steps
        value = world * B / (n_sample_steps * per_step)
    dumped = None
    if a.dump_outputs:
        outputs = {"sample": last} if a.sample_calls else {"x": plan.read_nchw(plan.x), "model_out": plan.read_nchw(plan.model_out)}
        dumped = dump_outputs(a.dump_outputs, outputs if world == 1 else {f"{k}_rank{rank}": v for k, v in outputs.items()}, DUMP_BYTES // world)
    if world > 1:
        # every rank timed the same K steps between the same two barriers; its own GPU-side time for them (HIP events on the
        # library's stream around a second, untimed-by-the-metric replay of K steps) tells a slow rank from a slow barrier
        own_ms = None
        if not a.sample_calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ext = torch.cuda.ExternalStream(plan.e.stream.value, device=dev)
            e0.record(ext)
            own_restarts = run_steps(a.steps)
            e1.record(ext)
            plan.e.sync()
            own_ms = e0.elapsed_time(e1) / a.steps
        mine = torch.tensor([per_step * 1e3, own_ms if own_ms is not None else per_step * 1e3], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        wall = [float(t[0]) for t in every]
        gpu = [float(t[1]) for t in every]
        per_step = max(wall) * 1e-3
        value = world * B / per_step if a.sample_calls else world * B / (n_sample_steps * per_step)
        if bcast is not None:
            try:
                ver = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as ex:          # noqa: BLE001 -- diagnostic field only
                ver = f"unavailable ({type(ex).__name__})"
            bcast.update({"rccl_version": ver if a.backend == "nccl" else None,
                          "ms_per_step_by_rank_wall": wall, "ms_per_step_by_rank_gpu_events": gpu, "sample_restarts_in_gpu_event_replay": own_restarts,
                          "ms_per_step_min_over_ranks": min(wall), "ms_per_step_max_over_ranks": max(wall)})

    sampler = f"{a.sampling_timesteps}-step DDIM of {T}" if a.sampling_timesteps else f"{T}-step DDPM"
    out = {
        "metric": f"sampled RAW patches/sec ({S}x{S}x4, {sampler})", "value": value, "unit": "patches/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": per_step * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "arithmetic": "fp32 storage and accumulation everywhere; 3x3 convolutions and attention on the exact-fp32 matrix instruction; wide 1x1 / Linear "
                      "layers, the 7x7 stem and the fused per-pixel chains on the bf16 matrix cores with every fp32 operand split exactly into three bf16 terms (six products, "
                      "full 24-bit significand: error against fp64 at or below the fp32 kernels', profiles/r6_split_gemm_accuracy.txt)",
        "config": {"workload": f"NoiseDiffNet dim={a.dim}{' + mid Attention' if a.mid_attn else ''}, {S}x{S}x4 patches, " +
                               sampler + " (sigmoid2, pred_v), "
                               f"{B} patches per GPU; a step = " +
                               ("one full sample() call" if a.sample_calls else
                                "one reverse-diffusion step (U-Net forward + fused posterior/noise update) over the per-GPU batch; "
                                f"patches/s = n_gpus*{B}/({n_sample_steps}*s_per_step)"),
                   "global_batch": world * B, "launch": "eager" if a.eager else "hipGraph replay",
                   "noise": "device Philox4x32-10", "untimed_soak_steps": soak_steps,
                   "sample_restarts_timed": timed_restarts},
    }
    if a.full and rank == 0 and world == 1 and not a.sample_calls and not a.eager and not a.no_full_sample:
        # the metric itself, once: ONE complete sample() call (x_T, every reverse step, the final clamp and the NCHW read-back) on the same condition; the
        # K-step figure above extrapolates a step x n_sample_steps, this is the driver-visible check of that extrapolation
        kw = dict(batch_size=B, condition={k: v.to(dev) for k, v in cond.items()})
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        gd.sample(seed=3, **kw)
        plan.e.sync()
        torch.cuda.synchronize(dev)
        secs = time.perf_counter() - t0
        ratio = (B / secs) / value
        out["full_sample"] = {"seconds": secs, "patches_per_s": B / secs, "steps": n_sample_steps, "ratio_to_value": ratio,
                              "more_than_2_percent_below_value": bool(ratio < 0.98),
                              "note": "one complete GaussianDiffusion.sample() call, wall clock on the host; `value` stays the K-step figure the bench contract "
                                      "defines -- when this call is more than 2 % slower (a box that throttles over 16 s of sustained load), read THIS figure"}
    if bcast:
        out["multi_gpu"] = bcast
    if dumped:
        out["dumped_outputs"] = {"dir": a.dump_outputs, "arrays": dumped}
    if a.full and rank == 0 and not a.no_roofline:
        out["roofline"] = roofline(a, loop, plan, L, per_step)
    if a.full and rank == 0 and world == 1 and not a.no_cpu:
        out["cpu_baseline"] = cpu_baseline({k: v for k, v in sd.items() if not k.startswith("mid_attn.")}, a.dim, S, n_sample_steps, B)
        out["config"]["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    fs = out.get("full_sample")
    if fs and fs["ratio_to_value"] < 0.98:
        # (the JSON line above is complete and carries the flag.  A non-zero exit is kept for a GROSS disagreement only -- the extrapolation itself broken --:
        #  a box whose clock sags a few per cent over a 16-second call must not turn a measured line into a failed run)
        print(f"bench.py: the complete sample() call ran at {fs['patches_per_s']:.4f} patches/s, more than 2 % below the extrapolated value {value:.4f}",
              file=sys.stderr)
        if fs["ratio_to_value"] < 0.90:
            sys.exit(4)


if __name__ == "__main__":
    main()
