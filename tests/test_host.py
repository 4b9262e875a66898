"""CPU-side tests: host logic, C-ABI surface, schedule tables, 2-rank gloo sharding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from noisediff_amd import _lib as L, synth
from noisediff_amd.diffusion import BUFFER_NAMES, GaussianDiffusion, make_betas, make_buffers
from noisediff_amd.net import NoiseDiffNet
from noisediff_amd.shard import shard_bounds
from noisediff_amd.spec import noisediff_param_spec
from util import state_dict
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def args(dim, **kw):
    return SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False, **kw)


def test_library_loads_and_exports_every_declared_symbol():
    """The drop-in boundary: every function include/noisediff_hip.h declares is exported and bound."""
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", header))
    declared -= {"nd_src", "nd_conv3x3", "nd_pointwise", "nd_sampler_state"}
    lib = L.load()
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.nd_version() >= 1
    assert lib.nd_last_error() is not None


def test_struct_layouts_match_the_header():
    # sizes computed from the C declarations: pointers 8 B, int32 4 B, natural alignment
    assert C.sizeof(L.Src) == 2 * 8 + 8 * 4 + 6 * 8
    assert C.sizeof(L.Conv3x3) == C.sizeof(L.Src) + 5 * 8 + 6 * 4
    assert C.sizeof(L.Pointwise) == C.sizeof(L.Src) + 8 * 8 + 13 * 4 + 4     # 13 int32 + tail padding to 8
    assert C.sizeof(L.SamplerState) == 6 * 8 + 2 * 4
    assert C.sizeof(L.ChainStage) == 2 * 8 + 4 * 4
    assert C.sizeof(L.PackItem) == 2 * 8 + 4 * 4
    assert C.sizeof(L.AdamItem) == 4 * 8 + 8 + 2 * 4 + 2 * 4 + 8                # nd_adam_item
    assert C.sizeof(L.Chain) == C.sizeof(L.Src) + 3 * C.sizeof(L.ChainStage) + 8 + 4 * 4


def test_host_only_entry_points_validate_arguments():
    lib = L.load()
    assert lib.nd_pack_conv3x3_weight_floats(64, 64) == 9 * 64 * 64
    assert lib.nd_pack_conv3x3_weight_floats(48, 48) == 9 * 48 * 64           # cout padded to 64
    assert lib.nd_pack_pointwise_weight_floats(24, 16) == 24 * 64
    assert lib.nd_conv3x3_stat_slots(256, 256, 64, 16) == (256 // 8) * (256 // 16) * 2
    assert lib.nd_conv3x3_tiling_id(16, 256, 256, 64) == 1621
    assert lib.nd_conv3x3_tiling_id(2, 8, 8, 64) == 811
    assert lib.nd_conv3x3_stat_slots(0, 8, 8, 1) == -1
    assert lib.nd_conv3x3_nhwc_f32(None, None) == -1 and b"null" in lib.nd_last_error()
    assert lib.nd_pointwise_gemm_nhwc_f32(None, None) == -1
    d = L.Conv3x3()
    d.src.p0 = d.weight = d.out = 0x1000
    d.src.c0, d.src.ld0 = 12, 12
    d.B, d.H, d.W, d.cin, d.cout, d.ldo = 1, 8, 8, 12, 8, 8
    assert lib.nd_conv3x3_nhwc_f32(C.byref(d), None) == -2                   # cin % 8 != 0 -> ND_E_SHAPE, nothing launched
    # Winograd weights: 128 KB blocks [cin/32][cout/64][16 positions][8 quads][64][4], zero padded
    assert lib.nd_pack_conv3x3_wino_weight_floats(64, 64) == 16 * 64 * 64
    assert lib.nd_pack_conv3x3_wino_weight_floats(48, 40) == 16 * 64 * 64
    assert lib.nd_conv3x3_wino_stat_slots(256, 256) == 16 * 16 * 2 and lib.nd_conv3x3_wino4_stat_slots(256, 250) == 16 * 16
    assert lib.nd_conv3x3_wino2_nhwc_f32(None, None) == -1
    d.src.c0 = d.src.ld0 = d.cin = 48
    d.src.p1, d.src.c1, d.src.ld1, d.cin = 0x2000, 16, 16, 64
    d.H = d.W = 32
    assert lib.nd_conv3x3_wino2_nhwc_f32(C.byref(d), None) == -2 and b"straddle" in lib.nd_last_error()
    # fused Linear chains: only NoiseDiffNet's width combinations are instantiated; weights padded to MFMA operand tiles
    assert lib.nd_pointwise_chain_supported(64, 128, 64, 64) == 1 and lib.nd_pointwise_chain_supported(8, 64, 64, 0) == 1
    assert lib.nd_pointwise_chain_supported(48, 96, 48, 48) == 1 and lib.nd_pointwise_chain_supported(64, 160, 64, 64) == 0
    assert lib.nd_pack_chain_weight_floats(8, 64, 1) == 8 * 64 and lib.nd_pack_chain_weight_floats(48, 4, 0) == 64 * 32
    assert lib.nd_pointwise_chain_nhwc_f32(None, None) == -1


@pytest.mark.parametrize("sched", ["linear", "cosine", "sigmoid1", "sigmoid2", "sigmoid3"])
def test_product_schedule_buffers_are_bit_identical_to_the_reference(golden, sched):
    names = [str(n) for n in golden("schedules", "sched.names")]
    assert names == BUFFER_NAMES
    ref = golden("schedules", f"sched.{sched}.1000")
    buf = make_buffers(make_betas(sched, 1000), "pred_v")
    for i, n in enumerate(names):
        assert np.array_equal(buf[n].numpy(), ref[i], equal_nan=True), n


def test_default_beta_schedule_name_is_rejected_like_the_reference():
    net = NoiseDiffNet(args(16))
    with pytest.raises(ValueError, match="unknown beta schedule sigmoid"):
        GaussianDiffusion(net, image_size=32)          # CLI default 'sigmoid' is not a valid name upstream either
    with pytest.raises(AssertionError):
        GaussianDiffusion(net, image_size=32, beta_schedule="sigmoid2", objective="bogus")
    with pytest.raises(AssertionError):
        GaussianDiffusion(net, image_size=32, beta_schedule="sigmoid2", timesteps=10, sampling_timesteps=11)


def test_module_surface_matches_the_reference_plugin_contract(meta):
    net = NoiseDiffNet(args(32))
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == meta["state_dict.d32"]
    assert (net.channels, net.out_dim, net.self_condition, net.random_or_learned_sinusoidal_cond, net.downsample_factor) == (4, 4, False, False, 8)
    net.load_state_dict(state_dict(32), strict=True)
    # PyTorch default init statistics (the reference never calls init_weights)
    w = NoiseDiffNet(args(32)).state_dict()["downs.0.0.block1.proj.weight"]
    bound = 1 / np.sqrt(32 * 9)
    assert float(w.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / np.sqrt(3), rel=0.1)
    import copy
    copy.deepcopy(net)                                          # EMA(self.net) deep-copies  (trainer_diffusion.py:62-69)
    wrapped = torch.nn.DataParallel(net)
    gd = GaussianDiffusion(wrapped, image_size=64, timesteps=1000, sampling_timesteps=50, beta_schedule="sigmoid2")
    assert gd.is_ddim_sampling and gd.num_timesteps == 1000 and gd.channels == 4 and gd.image_size == 64
    assert gd.device.type == "cpu" and len(list(gd.buffers())) == 13
    assert "mid_attn.to_qkv.weight" in NoiseDiffNet(args(16, mid_attn=True)).state_dict()


def test_sampler_tables(golden):
    net = NoiseDiffNet(args(16))
    gd = GaussianDiffusion(net, image_size=32, timesteps=1000, sampling_timesteps=50, beta_schedule="sigmoid2")
    t_cur, t_next, coef = gd._tables()
    ref = golden("schedules", "ddim_times.1000.50").tolist()
    assert t_cur.tolist() == ref[:-1] and t_next.tolist() == ref[1:]
    assert coef.shape == (50, 8) and coef[-1, 7] == 1.0 and bool((coef[:-1, 7] == 0).all())
    assert bool((coef[:, 6] == 0).all())                       # eta = 0 -> sigma = 0
    a, an = gd.alphas_cumprod[999], gd.alphas_cumprod[979]
    assert coef[0, 4] == an.sqrt() and coef[0, 5] == (1 - an).sqrt()
    gd = GaussianDiffusion(net, image_size=32, timesteps=20, beta_schedule="sigmoid2")
    t_cur, _, coef = gd._tables()
    assert t_cur.tolist() == list(range(19, -1, -1)) and coef[-1, 7] == 0.0 and bool((coef[:-1, 7] == 1).all())
    assert torch.equal(coef[:, 4], gd.posterior_mean_coef1.flip(0)) and torch.equal(coef[:, 6], (0.5 * gd.posterior_log_variance_clipped).exp().flip(0))


def test_product_refuses_to_run_without_a_gpu():
    net = NoiseDiffNet(args(16)).eval()
    gd = GaussianDiffusion(net, image_size=16, timesteps=4, beta_schedule="sigmoid2")
    cond = synth.make_condition(1, 16, seed=1)
    with pytest.raises(L.HipError, match="no CPU path"):
        gd.sample(batch_size=1, condition=cond)
    with pytest.raises(L.HipError, match="no CPU path"):               # training entry (p_losses, autograd on): no CPU path either
        gd(torch.zeros(1, 4, 16, 16), cond)


def test_shard_bounds_and_synthetic_shards():
    for total, world in ((128, 8), (10, 4), (3, 8), (0, 2)):
        spans = [shard_bounds(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    full = synth.make_condition(6, 16, seed=1)
    part = synth.make_condition(2, 16, seed=1, first_sample=3, total=6)
    for k in full:
        assert torch.equal(full[k][3:5], part[k]), k
    assert torch.equal(synth.make_noise(2, "x_T", 6, 4, 16)[3:5], synth.make_noise(2, "x_T", 2, 4, 16, first_sample=3))


def _gloo_worker(rank, world, port, q, total=3):
    import torch.distributed as dist
    from noisediff_amd.shard import sample_sharded
    from oracle import noisediff_oracle as O
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    dim, H, T = 16, 16, 3
    # the one collective: weights root -> all (a flat fp32 arena on the GPU path)
    flat = torch.cat([v.reshape(-1) for v in state_dict(dim).values()]) if rank == 0 else torch.zeros(sum(np.prod(p.shape) for p in noisediff_param_spec(dim)), dtype=torch.float32)
    dist.broadcast(flat, src=0)
    sd, off = {}, 0
    for p in noisediff_param_spec(dim):
        n = int(np.prod(p.shape))
        sd[p.name] = flat[off:off + n].view(p.shape)
        off += n
    state = {"lo": 0}

    def sample_fn(batch_size, condition, seed):
        lo = state["lo"]
        return O.sample(sd, condition, image_size=H, batch_size=batch_size, timesteps=T, x_T=synth.make_noise(seed, "x_T", batch_size, 4, H, lo),
                        noise=lambda i, shape: synth.make_noise(seed, f"noise.{i}", batch_size, 4, H, lo))

    out = sample_sharded(sample_fn, total, lambda lo, hi: synth.make_condition(hi - lo, H, seed=1, first_sample=lo, total=total),
                         seed=2, set_offset=lambda lo: state.update(lo=lo), gather=True)
    if rank == 0:
        q.put(out.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,total", [(2, 3), (8, 19)])
def test_n_rank_sharded_sampling_equals_single_rank_gloo(world, total):
    """world_size 2 and 8 on CPU (gloo; SURVEY section 4: "8-rank shard == 1-rank full-batch"): broadcast the weights once, shard the rows (8 ranks, 19 patches:
    ragged 3 + 3 + 3 + 2 + ...), gather -> the same patches as one rank, in parity-noise mode."""
    import torch.multiprocessing as mp
    from oracle import noisediff_oracle as O
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + world) % 2000
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q, total)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    dim, H, T = 16, 16, 3
    ref = O.sample(state_dict(dim), synth.make_condition(total, H, seed=1), image_size=H, batch_size=total, timesteps=T,
                   x_T=synth.make_noise(2, "x_T", total, 4, H), noise=lambda i, shape: synth.make_noise(2, f"noise.{i}", total, 4, H))
    assert got.shape == (total, 4, H, H)
    assert float(np.abs(got - ref.numpy()).max()) < 1e-5


def _gloo_empty_rank_worker(rank, world, port, q):
    import torch.distributed as dist
    from noisediff_amd.shard import sample_sharded
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    total = 2                                                            # world 3 > total 2: rank 2 has no rows
    calls = []

    def sample_fn(batch_size, condition, seed):
        calls.append(batch_size)
        return condition["rows"].float().view(-1, 1, 1, 1).expand(batch_size, 4, 2, 2).contiguous() + seed

    out = sample_sharded(sample_fn, total, lambda lo, hi: {"rows": torch.arange(lo, hi)}, seed=5, gather=True, device=torch.device("cpu"))
    own = sample_sharded(sample_fn, total, lambda lo, hi: {"rows": torch.arange(lo, hi)}, seed=5, gather=False)
    q.put((rank, out.numpy(), None if own is None else tuple(own.shape), list(calls)))
    dist.barrier()
    dist.destroy_process_group()


def test_a_rank_without_rows_takes_part_in_the_gather_gloo():
    """world_size 3, two patches: the rank without rows never calls the sampler, builds its placeholder on the device
    it is told (the collective's backend decides: RCCL takes device tensors only) and still returns the whole batch; without gather it
    returns None.  total_batch = 0 is refused."""
    import torch.multiprocessing as mp
    from noisediff_amd.shard import sample_sharded
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_empty_rank_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=240) for _ in range(3)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.broadcast_to(np.array([5.0, 6.0], dtype=np.float32).reshape(2, 1, 1, 1), (2, 4, 2, 2))
    for rank, out, own, calls in got:
        assert out.shape == (2, 4, 2, 2) and np.array_equal(out, want)
        assert (own, calls) == ((None, []) if rank == 2 else ((1, 4, 2, 2), [1, 1]))
    with pytest.raises(ValueError, match="nothing to sample"):
        sample_sharded(lambda **kw: None, 0, lambda lo, hi: {}, seed=0)


def test_generated_npy_contract(tmp_path):
    """file names, CHW fp32 payload, patch grid and the synth -> denoise composition."""
    from noisediff_amd import io
    grid = io.patch_grid(512)
    assert len(grid) == 24 and grid[0] == (0, 0) and grid[5] == (2128 - 512, 0) and grid[-1] == (2128 - 512, 1424 - 512)
    assert grid[1] == (384, 0) and grid[6] == (0, 384)
    out = synth.make_noise(3, "npy", 2, 4, 16)
    names = io.save_generated(str(tmp_path), out, ["00001_00_10s.ARW", "00002_00_10s.ARW"], ["00001_00_0.1s.ARW", None],
                              [io.image_coord(384, 768), io.image_coord(0, 0)])
    assert os.path.basename(names[0]) == "00001_00_10s+00001_00_0.1s+384_768.npy"
    assert os.path.basename(names[1]) == "00002_00_10s+00002_00_10s+0_0.npy"
    assert io.parse_generated_name(names[0]) == ("00001_00_10s", "00001_00_0.1s", 384, 768)
    back = np.load(names[0])
    assert back.dtype == np.float32 and back.shape == (4, 16, 16) and np.array_equal(back, out[0].numpy())
    noise = torch.tensor([[-2.0, 0.5, 0.9]])
    clean = torch.tensor([[0.3, 0.3, 0.3]])
    assert torch.allclose(io.compose_noisy(noise, clean), torch.tensor([[0.0, 0.8, 1.0]]))
    a = torch.rand(4, 8, 8)
    assert io.psnr(a, a) == float("inf")
    assert io.psnr(torch.zeros(4), torch.full((4,), 0.1)) == pytest.approx(20.0, abs=1e-4)


def test_bench_dump_outputs_are_float32_and_within_the_budget(tmp_path):
    """bench.py --dump-outputs: DIR/<name>.npy in float32, DUMP_BYTES in all at most; an output larger than its share is written as the elements
    at the same fixed, ascending flat indices on every call."""
    import bench
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    big = torch.arange(bench.DUMP_BYTES // 6, dtype=torch.float32)            # 2/3 of the budget on its own: more than its half
    files = []
    for run in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / run), {"small": small, "big": big})
        files.append({n: np.load(tmp_path / run / f"{n}.npy") for n in info})
        assert sum(os.path.getsize(tmp_path / run / f"{n}.npy") for n in info) <= bench.DUMP_BYTES
        assert info["small"] == {"shape": [2, 3, 4], "elements_written": 24} and info["big"]["shape"] == [big.numel()]
    got = files[0]
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], small.float().numpy())
    assert got["big"].dtype == np.float32 and got["big"].ndim == 1 and got["big"].size > big.numel() // 3
    assert np.all(np.diff(got["big"]) > 0) and got["big"][-1] < big.numel()        # distinct elements, ascending
    assert np.array_equal(got["big"], files[1]["big"])
    # --gpus N: every rank writes its own files into the same DIR with DUMP_BYTES / N; the run as a whole stays within DUMP_BYTES
    world, shard = 4, torch.arange(bench.DUMP_BYTES // 8, dtype=torch.float32)     # two of them per rank: twice a rank's share
    for rank in range(world):
        bench.dump_outputs(str(tmp_path / "ranks"), {f"x_rank{rank}": shard, f"model_out_rank{rank}": shard}, bench.DUMP_BYTES // world)
    assert len(os.listdir(tmp_path / "ranks")) == 2 * world
    assert sum(os.path.getsize(tmp_path / "ranks" / f) for f in os.listdir(tmp_path / "ranks")) <= bench.DUMP_BYTES


def test_blocked_map_row_permutation():
    """engine._blocked_map_rows: output row order of the ResnetBlock2 map Linear for nd_src.map_blocked (include/noisediff_hip.h):
    position 32 c + j holds scale channel 16 c + j (j < 16) or shift channel 16 c + j - 16."""
    from noisediff_amd.engine import _blocked_map_rows
    for C_ in (16, 64, 128):
        perm = _blocked_map_rows(C_)
        assert sorted(perm.tolist()) == list(range(2 * C_))                      # a permutation of the 2C producer rows
        planar = torch.arange(2 * C_)                                            # value = original row: scale rows 0..C-1, shift rows C..2C-1
        blocked = planar[perm].view(C_ // 16, 2, 16)
        for c in range(C_ // 16):
            assert blocked[c, 0].tolist() == list(range(16 * c, 16 * c + 16))              # scale channels of chunk c
            assert blocked[c, 1].tolist() == list(range(C_ + 16 * c, C_ + 16 * c + 16))    # shift channels of chunk c


def test_accelerate_retargets_the_class_so_replicas_and_copies_resolve_forward_through_themselves():
    """train.accelerate() must survive nn.DataParallel's replicate() (define_G wraps the net, models/modules.py:81): a replica copies
    ``__dict__``, so an instance-bound forward would keep running on the original module's parameters.  The HIP forward sits
    on the module's class instead: replicas, deep copies and pickles call it with their own ``self``; state dict and module type names
    are unchanged."""
    import copy
    import pickle
    from torch import nn
    from noisediff_amd import train
    net = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1), nn.GroupNorm(4, 16), nn.SiLU(), nn.Conv2d(16, 16, 1), nn.LayerNorm(64), nn.Linear(64, 64))
    keys = list(net.state_dict().keys())
    assert train.accelerate(net) == 1 and train.accelerate(net) == 0
    conv, norm = net[0], net[1]
    assert conv.forward.__func__ is train._hip_conv_forward and norm.forward.__func__ is train._hip_norm_forward
    assert "forward" not in conv.__dict__ and isinstance(conv, nn.Conv2d) and type(conv).__name__ == "Conv2d"
    assert type(conv)._nd_accelerated_base is nn.Conv2d and type(net[5])._nd_accelerated_base is nn.Linear
    for m in (conv, norm, net[3], net[4], net[5]):
        for other in (m._replicate_for_data_parallel(), copy.deepcopy(m)):
            assert other is not m and other.forward.__self__ is other and other.forward.__func__ is m.forward.__func__
    assert list(net.state_dict().keys()) == keys
    clone = pickle.loads(pickle.dumps(nn.Conv2d(8, 8, 3, padding=1)))          # plain modules still pickle ...
    assert isinstance(clone, nn.Conv2d)
    back = pickle.loads(pickle.dumps(net))                                      # ... and so do accelerated ones (torch.save(model), mp.spawn arguments)
    assert [type(m) for m in back] == [type(m) for m in net] and back[0].forward.__func__ is train._hip_conv_forward
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), net.state_dict().values()))
    import io as _io
    buf = _io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    assert torch.load(buf, weights_only=False)[1].forward.__func__ is train._hip_norm_forward
    with pytest.raises(Exception, match="HIP library only|no CPU path"):
        conv(torch.zeros(1, 8, 16, 16))                                          # still no CPU fallback


def test_adam_copies_and_pickles_arrive_with_their_caches():
    """torch.optim.Optimizer.__getstate__ keeps only defaults / state / param_groups, so a deep copy and a pickle round trip of train.Adam come back
    through __setstate__ without the instance's own caches: they must be there and empty (the first step() reads them), the copy's parameters its own."""
    import copy
    import pickle
    from torch import nn
    from noisediff_amd import train
    opt = train.Adam([nn.Parameter(torch.zeros(4)), nn.Parameter(torch.ones(3, 2))], lr=2e-3, weight_decay=0.01)
    opt._nd_tables[("stale",)] = ()                                              # what a copy must not inherit
    for other in (copy.deepcopy(opt), pickle.loads(pickle.dumps(opt))):
        assert type(other) is train.Adam and other.defaults == opt.defaults
        assert other._nd_tables == {} and other._nd_captured_lr == {} and other._nd_captured == [] and other._nd_keep is None
        other.check_captured_lr()
        assert all(a is not b and torch.equal(a, b) for a, b in zip(other.param_groups[0]["params"], opt.param_groups[0]["params"]))
    opt.load_state_dict(opt.state_dict())                                       # comes through __setstate__ too: keeps its caches
    assert ("stale",) in opt._nd_tables


def test_split_k_plan_is_a_function_of_the_shape():
    """nd_conv3x3_wino4_splitk_plan (host code, no GPU): 1 where the layer's (sample, region, cout tile) items fill the chip or cin leaves
    no room, else the power of two that brings them to about 256 with at least four 16-channel chunks per range."""
    lib = L.load()
    plan = lib.nd_conv3x3_wino4_splitk_plan
    assert plan(16, 256, 256, 64, 64) == 1 and plan(16, 32, 32, 512, 512) == 1          # the bench workload's layers: never split
    assert plan(4, 32, 32, 512, 512) == 4 and plan(4, 64, 64, 256, 256) == 2 and plan(4, 32, 32, 1536, 512) == 4
    assert plan(1, 32, 32, 1536, 64) == 8 and plan(1, 32, 32, 64, 64) == 1 and plan(1, 32, 32, 72, 64) == 1
    assert plan(4, 256, 256, 64, 64) == 1 and plan(0, 1, 1, 1, 1) == 1
    assert lib.nd_conv3x3_wino4_splitk_workspace_floats(2, 8, 8, 16, 4) == 2 * 8 * 8 * 16 * 4


# The kernel of each of LSID's 3x3 operators per (B, H, W), with wino4 on / off: what the two LSID copies of the rule chose before
# train.conv3x3_kind replaced them.  One group per stage: encoder stages 1-5 (conv_i_1, conv_i_2, conv_i_1's data gradient from stage 2 on), then
# decoder stages 6-9 (conv_j_1 over the concat, conv_j_2, conv_j_1's data gradient); conv_k_2's data gradient has conv_k_2's arguments.
# 4: wino4, 2: wino2, w: wino, d: direct.
LSID_KINDS = {
    (2, 64, 64): ("24 444 222 ddd ddd ddd 222 444 444", "22 222 222 ddd ddd ddd 222 222 222"),
    (1, 36, 44): ("22 222 ddd ddd ddd ddd ddd 222 222", "22 222 ddd ddd ddd ddd ddd 222 222"),
    (4, 256, 256): ("24 444 444 444 222 444 444 444 444", "22 222 222 222 222 222 222 222 222"),
    (1, 512, 512): ("24 444 444 444 444 444 444 444 444", "22 222 222 222 222 222 222 222 222"),
}


def _lsid_conv3x3_ops(B, H, W):
    """(B, h, w, cin, cout, c0, c1, ld) of LSID's 3x3 operators grouped per stage, as the HIP forward and backward pass them (ld: widest source)."""
    from noisediff_amd.spec import LSID_STAGES
    sizes = [(H, W)]
    for _ in range(4):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    groups, cin = [], 8
    for i, c in enumerate(LSID_STAGES):
        h, w = sizes[i]
        groups.append([(B, h, w, cin, c, cin, 0, cin), (B, h, w, c, c, c, 0, c)] + ([(B, h, w, c, cin, c, 0, c)] if i else []))
        cin = c
    for i in (3, 2, 1, 0):
        c, (h, w) = LSID_STAGES[i], sizes[i]
        groups.append([(B, h, w, 2 * c, c, c, c, c), (B, h, w, c, c, c, 0, c), (B, h, w, c, 2 * c, c, 0, c)])
    return groups


@pytest.mark.parametrize("B,H,W", sorted(LSID_KINDS))
def test_conv3x3_kind_keeps_the_lsid_kernels(B, H, W):
    from noisediff_amd.train import conv3x3_kind
    letter = {"wino4": "4", "wino2": "2", "wino": "w", "direct": "d"}
    for wino4, want in zip((True, False), LSID_KINDS[(B, H, W)]):
        got = " ".join("".join(letter[conv3x3_kind(*op, wino4=wino4)] for op in g) for g in _lsid_conv3x3_ops(B, H, W))
        assert got == want, (wino4, got)


def _cuda_like(*shape):
    """What cat_sources_ok reads of a CUDA tensor, without a GPU."""
    return SimpleNamespace(shape=torch.Size(shape), is_cuda=True, dim=lambda: len(shape))


def test_conv3x3_kind_keeps_the_train_and_lsid_decisions_at_their_limits():
    from noisediff_amd import train
    kind = train.conv3x3_kind
    # conv9_1 at B = 16, 512 x 512 (c0 = c1 = 32): LSID bounds the source by its widest stride and takes wino4, train.py by c0 + c1 and refuses it
    assert kind(16, 512, 512, 64, 32, 32, 32, 32) == "wino4"
    assert kind(16, 512, 512, 64, 32, 32, 32, 64) == "wino2"
    assert not train.cat_sources_ok(_cuda_like(16, 32, 512, 512), _cuda_like(16, 32, 512, 512), 32)
    assert train.cat_sources_ok(_cuda_like(2, 32, 64, 64), _cuda_like(2, 32, 64, 64), 32)
    assert train.cat_sources_ok(_cuda_like(2, 32, 64, 64), _cuda_like(2, 32, 64, 64))
    # past 2^24 pixels: F(2x2) wino (LSID runs it, train.py takes the direct kernel instead)
    assert kind(64, 512, 512, 64, 64, 64, 0, 64) == "wino"
    # a concat with c0 % 16 != 0 or c1 % 16 != 0: not wino4, so train.py refuses it
    assert kind(2, 64, 64, 40, 32, 8, 32, 40) == "wino"
    assert not train.cat_sources_ok(_cuda_like(2, 8, 64, 64), _cuda_like(2, 32, 64, 64), 32)
    assert not train.cat_sources_ok(_cuda_like(2, 32, 64, 64), _cuda_like(2, 8, 64, 64), 32)
    assert not train.cat_sources_ok(_cuda_like(2, 32, 64, 64), _cuda_like(2, 32, 64, 64), 4096)
    # cin % 8 != 0: direct (train.py raises); cout > 2048 and a width the F(4x4) kernel does not tile: wino2
    assert kind(1, 64, 64, 12, 16, 12, 0, 12) == "direct"
    assert kind(1, 64, 64, 64, 4096, 64, 0, 64) == "wino2"
    assert kind(2, 64, 40, 64, 64, 64, 0, 64) == "wino2"


def _takes(kernel, B=2, H=32, W=32, cin=64, cout=64, c0=None, c1=0, ld0=None, ld1=None, **kw):
    from noisediff_amd._host import conv3x3_takes
    c0 = cin - c1 if c0 is None else c0
    return conv3x3_takes(kernel, B, H, W, cin, cout, c0, c1, c0 if ld0 is None else ld0, (c1 if ld1 is None else ld1), **kw)


def test_conv3x3_takes_answers_on_both_sides_of_each_limit():
    """nd_conv3x3_takes (host code, no GPU) just inside and just outside every limit of each kernel's shape function in csrc/conv3x3_desc.h."""
    every = (L.CONV3X3_DIRECT, L.CONV3X3_WINO, L.CONV3X3_WINO2, L.CONV3X3_WINO4, L.CONV3X3_WINO4_16)
    f2, f4 = every[:3], every[3:]
    for k in every:                                                      # nd_conv3x3_common_shape
        assert _takes(k) and not _takes(k, B=0) and not _takes(k, c0=60) and not _takes(k, cin=66, c0=62, c1=4, ld0=64)
        assert _takes(k, ld0=68) and not _takes(k, ld0=60) and not _takes(k, ld0=66) and not _takes(k, cin=96, c1=32, ld1=28)
        assert _takes(k, H=34, upsample=True) and not _takes(k, H=33, upsample=True) and not _takes(k, cin=96, c1=32, upsample=True)
        assert _takes(k, mode=L.PRO_AFFINE_SILU) and not _takes(k, mode=L.PRO_LAYERNORM) and _takes(k, ldo=68) and not _takes(k, ldo=60)
    for k in f2:                                                         # nd_conv3x3_f2_shape
        assert _takes(k, cin=72) and not _takes(k, cin=60) and _takes(k, ldo=66)
        assert _takes(k, mode=L.PRO_LEAKY_SECOND, cin=96, c1=32) and not _takes(k, mode=L.PRO_AFFINE_GENMAP_SILU)
        assert _takes(k, mode=L.PRO_AFFINE_MAP_SILU) and not _takes(k, mode=L.PRO_AFFINE_MAP_SILU, map_blocked=True)
        assert _takes(k, cin=8, cout=4100, H=8, W=8)                     # no cin > 16, no cout <= 2048, no 16 x 16 tile: those are F(4x4)'s / policy
    for k in f2[:2]:                                                     # direct and wino: nothing of their own -- past wino2's limits they still take the layer
        assert _takes(k, B=64, H=512, W=512) and _takes(k, cin=64, c0=16, c1=48) and _takes(k, mode=L.PRO_AFFINE_MAP_SILU, upsample=True)
    k = L.CONV3X3_WINO2                                                  # nd_conv3x3_wino2_shape
    assert not _takes(k, mode=L.PRO_AFFINE_MAP_SILU, upsample=True)
    assert _takes(k, B=63, H=512, W=512, cin=8) and not _takes(k, B=64, H=512, W=512, cin=8)         # 2^24 pixels
    lim = ((1 << 31) - 1) // (7 * 2048 + 7)
    assert _takes(k, B=1, H=16, W=2048, ldo=lim) and not _takes(k, B=1, H=16, W=2048, ldo=lim + 1)   # (7 W + 7) ldo < 2^31
    assert _takes(k, B=127, H=256, W=256) and not _takes(k, B=128, H=256, W=256)                     # sources 64 KB below 2 GiB ...
    assert 4681 * 256 * 448 * 4 == (1 << 31) - 65536
    assert _takes(k, B=4680, H=16, W=16, ld0=448) and not _takes(k, B=4681, H=16, W=16, ld0=448)     # ... to the byte
    assert _takes(k, B=4681, H=16, W=16, ld0=444) and not _takes(k, B=4681, H=16, W=16, cin=96, c1=32, ld0=64, ld1=448)
    assert _takes(k, B=63, H=256, W=256, mode=L.PRO_AFFINE_MAP_SILU) and not _takes(k, B=64, H=256, W=256, mode=L.PRO_AFFINE_MAP_SILU)    # the map: 2 cin floats per pixel
    assert _takes(k, cin=96, c0=32, c1=64) and _takes(k, cin=96, c0=64, c1=32) and not _takes(k, cin=96, c0=48, c1=48)   # a 32-channel chunk must not straddle
    for k in f4:                                                         # nd_conv3x3_wino4_shape
        assert _takes(k, cin=20) and not _takes(k, cin=16) and not _takes(k, cout=62) and _takes(k, cout=2048) and not _takes(k, cout=2052)
        assert not _takes(k, ldo=66) and _takes(k, cin=96, c0=48, c1=48) and not _takes(k, cin=96, c0=40, c1=56)
        assert _takes(k, B=1, H=16, W=2048) and not _takes(k, B=1, H=16, W=2052)
        assert _takes(k, B=1, H=32768, W=32) and not _takes(k, B=1, H=32770, W=32)
        assert _takes(k, B=63, H=256, W=256) and not _takes(k, B=64, H=256, W=256)                   # sources 64 KB below 1 GiB, counted from one row + one pixel ahead (with at least 16 channels per source the 2^24-pixel bound lies behind it)
        assert _takes(k, B=31, H=256, W=256, ld0=128) and not _takes(k, B=32, H=256, W=256, ld0=128)
        assert _takes(k, B=63, H=256, W=256, cin=96, c0=64, c1=32) and not _takes(k, B=32, H=256, W=256, cin=96, c0=64, c1=32, ld1=128)
        assert _takes(k, B=63, H=256, W=256, cin=32, cout=256) and not _takes(k, B=64, H=256, W=256, cin=32, cout=256)  # outputs 64 KB below 4 GiB
        assert _takes(k, B=127, H=256, W=256, cin=32, cout=64, upsample=True) and not _takes(k, B=32, H=256, W=256, cin=32, cout=256, ldo=512)
        assert not _takes(k, map_blocked=True) and not _takes(k, mode=L.PRO_AFFINE_MAP_SILU, upsample=True)
        for s in (2, 4, 8):                                              # split-K: 2, 4 or 8 ranges of at least two whole chunks, plain / affine sources, partial sums below 2 GiB
            assert _takes(k, cin=32 * s, splits=s) and not _takes(k, cin=16 * s, splits=s) and not _takes(k, cin=32 * s + 16, splits=s) and not _takes(k, cin=32 * s + 8, splits=s)
            assert _takes(k, B=128 // s - 1, H=256, W=256, cin=32 * s, splits=s) and not _takes(k, B=128 // s, H=256, W=256, cin=32 * s, splits=s)
        assert _takes(k, B=63, H=256, W=256, splits=2)
        assert not _takes(k, cin=96, splits=3) and not _takes(k, cin=512, splits=16) and _takes(k, mode=L.PRO_AFFINE_SILU, splits=2)
    k = L.CONV3X3_WINO4                                                  # the 16 x 32-region form alone: every prologue of the family
    assert _takes(k, mode=L.PRO_LEAKY) and _takes(k, mode=L.PRO_LEAKY_SECOND, cin=96, c1=32) and not _takes(k, mode=L.PRO_LEAKY, splits=2)
    assert _takes(k, B=31, H=256, W=256, mode=L.PRO_AFFINE_MAP_SILU) and not _takes(k, B=32, H=256, W=256, mode=L.PRO_AFFINE_MAP_SILU)    # a map 64 KB below 1 GiB
    assert _takes(k, mode=L.PRO_AFFINE_MAP_SILU, map_blocked=True) and not _takes(k, cin=72, mode=L.PRO_AFFINE_MAP_SILU, map_blocked=True)
    assert _takes(k, mode=L.PRO_AFFINE_GENMAP_SILU) and not _takes(k, cin=72, mode=L.PRO_AFFINE_GENMAP_SILU) and not _takes(k, mode=L.PRO_AFFINE_GENMAP_SILU, splits=2)
    assert not _takes(k, cin=96, c1=32, mode=L.PRO_AFFINE_GENMAP_SILU) and not _takes(k, mode=L.PRO_AFFINE_GENMAP_SILU, upsample=True)
    k = L.CONV3X3_WINO4_16                                               # the 16 x 16-region form: plain and affine + SiLU sources
    for mode in (L.PRO_AFFINE_MAP_SILU, L.PRO_AFFINE_GENMAP_SILU, L.PRO_LEAKY, L.PRO_LEAKY_SECOND):
        assert not _takes(k, cin=96, c1=32 if mode == L.PRO_LEAKY_SECOND else 0, mode=mode)
    assert not _takes(5) and not _takes(-1)                              # no such kernel


def test_a_question_is_not_a_failure():
    """nd_conv3x3_takes answering 0 leaves nd_last_error as the last refusal wrote it."""
    lib = L.load()
    assert lib.nd_conv3x3_wino_nhwc_f32(None, None) == -1               # a host-only refusal: returns before any HIP call
    said = lib.nd_last_error()
    assert b"nd_conv3x3_wino: null descriptor" in said
    for k in (L.CONV3X3_DIRECT, L.CONV3X3_WINO, L.CONV3X3_WINO2, L.CONV3X3_WINO4, L.CONV3X3_WINO4_16):
        assert not _takes(k, cin=12) and not _takes(k, H=33, upsample=True) and not _takes(k, ldo=60) and not _takes(k, splits=3)
        assert lib.nd_last_error() == said
    assert lib.nd_conv3x3_takes(L.CONV3X3_WINO4, None, 1) == 0 and lib.nd_last_error() == said


def _pw(cin=64, cout=64, c1=0, c0=None, ld0=None, ld1=None, ldo=None, split=False, rowstats=False, **kw):
    """nd_pointwise_gemm_takes / _split_takes on a one-sample descriptor of 32 pixels (rows of 8); ``kw``: further fields of the descriptor or of its source."""
    d = L.Pointwise(B=1, HW=32, W=8, cin=cin, cout=cout, ldo=cout if ldo is None else ldo)
    c0 = cin - c1 if c0 is None else c0
    d.src.c0, d.src.c1, d.src.ld0, d.src.ld1 = c0, c1, c0 if ld0 is None else ld0, c1 if ld1 is None else ld1
    d.src.rowstats = 16 if rowstats else None                            # given or not is all a question reads of a pointer
    for k, v in kw.items():
        setattr(d.src if hasattr(d.src, k) else d, k, v)
    return bool((L.load().nd_pointwise_gemm_split_takes if split else L.load().nd_pointwise_gemm_takes)(C.byref(d)))


def test_norm_questions_answer_on_both_sides_of_each_limit():
    lib = L.load()
    gn = lambda c, g: bool(lib.nd_groupnorm_train_takes(c, g))
    assert gn(64, 8) and gn(1024, 2) and not gn(1024, 1) and not gn(1028, 4) and not gn(60, 8) and not gn(6, 2) and not gn(0, 1) and not gn(64, 0)
    ln = lambda c: bool(lib.nd_layernorm_train_takes(c))
    assert ln(16) and not ln(12) and ln(1024) and not ln(1028) and not ln(18) and ln(48)
    for q in (lib.nd_rmsnorm_train_takes, lib.nd_token_sum_takes):
        assert q(4) and q(1024) and not q(1028) and not q(6) and not q(0) and not q(-4)


def test_pointwise_questions_answer_on_both_sides_of_each_limit():
    for split in (False, True):                                          # the common shape part: both entries
        w = dict(split=split, cout=128)
        assert _pw(**w) and not _pw(HW=0, **w) and not _pw(cin=62, **w) and not _pw(c0=60, **w)
        assert _pw(c1=32, **w) and not _pw(c0=32, c1=28, **w) and not _pw(c0=30, c1=34, **w)
        assert _pw(ld0=68, **w) and not _pw(ld0=60, **w) and not _pw(ld0=66, **w) and _pw(c1=32, ld1=36, **w) and not _pw(c1=32, ld1=28, **w) and not _pw(c1=32, ld1=34, **w)
        assert _pw(ldo=132, **w) and not _pw(ldo=124, **w) and not _pw(ldo=130, **w) and not _pw(upsample=1, **w)
        assert _pw(act=L.ACT_SILU, **w) and not _pw(act=3, **w) and not _pw(act=-1, **w)
        assert _pw(mode=L.PRO_LEAKY, **w) and _pw(mode=L.PRO_AFFINE_SILU, **w) and not _pw(mode=L.PRO_AFFINE_SILU, c1=32, **w) and not _pw(mode=L.PRO_AFFINE_MAP_SILU, **w)
        assert _pw(cin=1024, mode=L.PRO_LAYERNORM, rowstats=True, **w) and not _pw(cin=1028 if not split else 1056, mode=L.PRO_LAYERNORM, rowstats=True, **w)
        assert _pw(cin=128, mode=L.PRO_LAYERNORM, rowstats=True, **w) and not _pw(cin=128, mode=L.PRO_LAYERNORM, **w) and not _pw(mode=L.PRO_LAYERNORM, rowstats=True, c1=32, **w)
    # the fp32 entry alone: any width in fours, the LayerNorm prologue with its own statistics up to 64 channels, both shuffles
    assert _pw(cin=24, cout=20) and _pw(cin=4, cout=4) and _pw(mode=L.PRO_LAYERNORM) and not _pw(cin=68, mode=L.PRO_LAYERNORM)
    assert _pw(unshuffle=1, ld0=16) and not _pw(unshuffle=1, ld0=12) and not _pw(cin=24, unshuffle=1) and not _pw(unshuffle=1, W=5) and not _pw(unshuffle=1, mode=L.PRO_SILU)
    shuf = dict(shuffle_c=16, shuffle_h=8, shuffle_w=16, ldo=16)
    assert _pw(**shuf) and not _pw(**dict(shuf, shuffle_c=12)) and not _pw(**dict(shuf, ldo=12)) and not _pw(**dict(shuf, shuffle_h=0)) and not _pw(**dict(shuf, W=5))
    # the split kernel's own conditions
    s = lambda **kw: _pw(split=True, **dict(dict(cout=128), **kw))
    assert s(cin=64) and not s(cin=32) and s(cin=96) and not s(cin=80) and s(cout=256) and not s(cout=64) and not s(cout=192)
    assert s(cin=96, c1=32) and s(cin=96, c1=64) and not s(cin=96, c1=48) and not s(cin=96, c1=16)
    assert not s(unshuffle=1, ld0=16) and not s(shuffle_c=32, shuffle_h=8, shuffle_w=16, ldo=32) and _pw(cout=128, shuffle_c=32, shuffle_h=8, shuffle_w=16, ldo=32)
    assert not s(mode=L.PRO_LAYERNORM) and s(mode=L.PRO_LAYERNORM, rowstats=True)
    assert L.load().nd_pointwise_gemm_takes(None) == 0 and L.load().nd_pointwise_gemm_split_takes(None) == 0


def test_chain_question_answers_for_the_pixel_tiles_and_the_width_table():
    lib = L.load()
    assert lib.nd_pointwise_chain_takes(32, 64, 128, 64, 64) and lib.nd_pointwise_chain_takes(64, 64, 128, 64, 64) and lib.nd_pointwise_chain_takes(32, 4, 32, 32, 0)
    assert not lib.nd_pointwise_chain_takes(48, 64, 128, 64, 64) and not lib.nd_pointwise_chain_takes(0, 64, 128, 64, 64) and not lib.nd_pointwise_chain_takes(-32, 64, 128, 64, 64)
    assert not lib.nd_pointwise_chain_takes(32, 64, 128, 128, 64) and not lib.nd_pointwise_chain_takes(32, 64, 64, 64, 64)
    assert lib.nd_pointwise_chain_supported(64, 128, 64, 64) and not lib.nd_pointwise_chain_supported(64, 128, 128, 64)


def test_wgrad_questions_answer_under_every_pin_and_on_both_sides_of_each_limit():
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(-1)
    try:
        plans = {}
        for pin in (0, 1, 2, 3):
            lib.nd_conv3x3_wgrad_form(pin)
            plans[pin] = [lib.nd_conv3x3_wgrad_plan(*shape) for shape in ((2, 16, 32, 64, 64), (1, 9, 11, 32, 64), (2, 16, 32, 48, 64), (79, 64, 64, 64, 64), (78, 64, 64, 64, 64))]
        # Winograd shape with whole 32 / 64 blocks; nine taps only; cin % 32 != 0: four waves only; 79 * 16 * 4 * 2 * 2 = 20224 >= 20000 > 19968 block items: eight waves by the shape
        assert plans == {0: [2, 1, 2, 3, 2], 1: [1, 1, 1, 1, 1], 2: [2, 1, 2, 2, 2], 3: [3, 1, 2, 3, 3]}
        lib.nd_conv3x3_wgrad_form(0)
        assert lib.nd_conv3x3_wgrad_plan(2, 16, 32, 62, 64) == 1 and lib.nd_conv3x3_wgrad_plan(0, 16, 32, 64, 64) == 1
        cat = lambda B=2, H=16, W=32, c0=32, c1=32, cout=64, ldx0=None, ldx1=None, ldy=None: bool(lib.nd_conv3x3_wgrad_cat_takes(
            B, H, W, c0, c1, cout, c0 if ldx0 is None else ldx0, c1 if ldx1 is None else ldx1, cout if ldy is None else ldy))
        assert cat() and not cat(c0=16) and not cat(c1=48) and not cat(c1=0) and cat(W=16) and not cat(W=12) and cat(H=4) and not cat(H=6)
        assert cat(cout=16) and not cat(cout=8) and not cat(cout=20) and cat(ldx0=36) and not cat(ldx0=28) and not cat(ldx0=34) and not cat(ldx1=28) and not cat(ldx1=34)
        assert not cat(ldy=60) and not cat(ldy=66) and not cat(B=0)
        # within a sample every tensor stays below 1 GiB (H W ld 4 < 2^30: 65536 pixels of 4092 / 4096 floats), and there are fewer than 2^30 pixels; nothing is allocated
        big = dict(B=1, H=256, W=256)
        for ld in ("ldx0", "ldx1", "ldy"):
            assert cat(**big, **{ld: 4092}) and not cat(**big, **{ld: 4096})
        assert cat(B=16383, H=256, W=256) and not cat(B=16384, H=256, W=256)
        for pin, takes in ((1, False), (2, True), (3, True)):
            lib.nd_conv3x3_wgrad_form(pin)
            assert cat() == takes
    finally:
        lib.nd_conv3x3_wgrad_form(was)


def test_the_new_questions_are_not_failures_either():
    """Every question of the 1x1, chain, norm and weight-gradient families answering 0 leaves nd_last_error as the last refusal wrote it."""
    lib = L.load()
    assert lib.nd_conv3x3_wino_nhwc_f32(None, None) == -1               # a host-only refusal: returns before any HIP call
    said = lib.nd_last_error()
    assert not _pw(cin=62) and not _pw(ldo=60) and not _pw(cin=32, split=True) and not _pw(cin=128, mode=L.PRO_LAYERNORM, split=True)
    assert not lib.nd_groupnorm_train_takes(1024, 1) and not lib.nd_layernorm_train_takes(12) and not lib.nd_rmsnorm_train_takes(6) and not lib.nd_token_sum_takes(1028)
    assert not lib.nd_pointwise_chain_takes(48, 64, 128, 64, 64) and not lib.nd_pointwise_chain_takes(32, 64, 64, 64, 64)
    assert lib.nd_conv3x3_wgrad_plan(1, 9, 11, 32, 64) == 1 and not lib.nd_conv3x3_wgrad_cat_takes(2, 16, 32, 16, 32, 64, 16, 32, 64)
    assert not lib.nd_conv3x3_wgrad_cat_takes(1, 256, 256, 32, 32, 64, 32, 4096, 64)
    assert lib.nd_last_error() == said


def test_engine_layer_rules_equal_their_literal_rules_on_a_grid():
    """engine._split_layer / _wino4_layer ask the library; the literal rules they replaced are the specification (cout in steps of 12: a few seconds)."""
    from noisediff_amd import engine
    for cin in range(4, 2049, 4):
        for cout in range(4, 2049, 12):
            assert engine._split_layer(cin, cout) == bool(engine.SPLIT_PW and cin % 32 == 0 and cin >= 64 and cout % 128 == 0), (cin, cout)
            assert engine._wino4_layer(cin, cout) == (cin > 16 and cin % 4 == 0 and cout % 4 == 0), (cin, cout)
    assert engine._wino4_layer(64, 2048) and not engine._wino4_layer(64, 2052)     # the one difference: no F(4x4) packing past the kernel's bias table
    assert not engine._wino4_layer(16, 64) and not engine._wino4_layer(18, 64) and not engine._wino4_layer(64, 62) and not engine._split_layer(64, 0)


def test_conv3x3_kind_answers_a_repeated_shape_from_its_cache():
    from noisediff_amd._host import conv3x3_kind
    shape = (3, 48, 80, 64, 64, 64, 0, 64)
    first = conv3x3_kind(*shape)
    before = conv3x3_kind.cache_info()
    assert conv3x3_kind(*shape) == first == "wino2"
    after = conv3x3_kind.cache_info()
    assert (after.hits, after.misses) == (before.hits + 1, before.misses)


class _Operand:
    """A stand-in for a device tensor on the CPU: an address and a shape."""

    def __init__(self, address, *shape):
        self.address, self.shape = address, shape

    def data_ptr(self):
        return self.address


_T, _T2 = _Operand(0x10000, 2, 8, 8, 24), _Operand(0x20000, 2, 8, 8, 40)
_EXTRA = {name: _Operand(0x30000 + 0x1000 * i, 7) for i, name in enumerate(("mad", "map", "vec", "gamma", "beta", "rowstats"))}


def test_source_builder_fills_what_a_hand_filled_nd_src_holds():
    """L.src against L.Src filled field by field here: one and two sources, the c / ld / offset overrides, every extra operand alone and together, the three
    addressing flags; tensors, integer addresses and None alike; the operands hang on the struct."""
    assert bytes(L.src(_T)) == bytes(L.Src(p0=0x10000, c0=24, ld0=24))
    assert bytes(L.src(0x10000, c=24, ld=24)) == bytes(L.Src(p0=0x10000, c0=24, ld0=24))
    assert bytes(L.src(_T, _T2, L.PRO_LEAKY_SECOND)) == bytes(L.Src(p0=0x10000, c0=24, ld0=24, p1=0x20000, c1=40, ld1=40, mode=L.PRO_LEAKY_SECOND))
    assert bytes(L.src(_T, 0x20000, c1=16, ld1=48)) == bytes(L.Src(p0=0x10000, c0=24, ld0=24, p1=0x20000, c1=16, ld1=48))
    assert bytes(L.src(_T, c=16, ld=32, offset=5)) == bytes(L.Src(p0=0x10000 + 4 * 5, c0=16, ld0=32))
    assert bytes(L.src(_T, c=16)) == bytes(L.Src(p0=0x10000, c0=16, ld0=24)) and bytes(L.src(_T, ld=32)) == bytes(L.Src(p0=0x10000, c0=24, ld0=32))
    assert bytes(L.src(None, None, L.PRO_SILU, 8, 12, 0, 4, 6)) == bytes(L.Src(c0=8, ld0=12, c1=4, ld1=6, mode=L.PRO_SILU))       # a question: widths, no address
    for name, op in _EXTRA.items():
        want = bytes(L.Src(p0=0x10000, c0=24, ld0=24, mode=L.PRO_AFFINE_SILU, **{name: op.address}))
        assert bytes(L.src(_T, None, L.PRO_AFFINE_SILU, **{name: op})) == want and bytes(L.src(_T, None, L.PRO_AFFINE_SILU, **{name: op.address})) == want, name
    for flag in ("upsample", "unshuffle", "map_blocked"):
        assert bytes(L.src(_T, **{flag: 1})) == bytes(L.Src(p0=0x10000, c0=24, ld0=24, **{flag: 1})), flag
    s = L.src(_T, _T2, L.PRO_AFFINE_MAP_SILU, upsample=1, unshuffle=1, map_blocked=1, **_EXTRA)
    assert bytes(s) == bytes(L.Src(p0=0x10000, c0=24, ld0=24, p1=0x20000, c1=40, ld1=40, mode=L.PRO_AFFINE_MAP_SILU, upsample=1, unshuffle=1, map_blocked=1,
                                   **{name: op.address for name, op in _EXTRA.items()}))
    assert {id(r) for r in s._refs} >= {id(_T), id(_T2)} | {id(op) for op in _EXTRA.values()}


def test_conv3x3_builder_fills_what_a_hand_filled_nd_conv3x3_holds():
    """L.conv3x3: with and without bias, with and without statistics, ldo != cout; the source's operands carried over."""
    s, w, b, out, st, sc = L.src(_T, mad=_EXTRA["mad"]), _Operand(0x40000, 9), _Operand(0x41000, 32), _Operand(0x42000, 2, 8, 8, 32), _Operand(0x43000, 2, 4, 32, 2), 0x44000
    plain = dict(src=s, weight=0x40000, out=0x42000, B=2, H=8, W=8, cin=24, cout=32)
    assert bytes(L.conv3x3(s, w, None, out, 2, 8, 8, 24, 32)) == bytes(L.Conv3x3(ldo=32, **plain))
    assert bytes(L.conv3x3(s, 0x40000, b, 0x42000, 2, 8, 8, 24, 32)) == bytes(L.Conv3x3(bias=0x41000, ldo=32, **plain))
    assert bytes(L.conv3x3(s, w, b, out, 2, 8, 8, 24, 32, 48)) == bytes(L.Conv3x3(bias=0x41000, ldo=48, **plain))
    d = L.conv3x3(s, w, b, out, 2, 8, 8, 24, 32, stats=st, slot_count=sc)
    assert bytes(d) == bytes(L.Conv3x3(bias=0x41000, ldo=32, stats=0x43000, slot_count=0x44000, **plain))
    assert d._refs[0] is s._refs and {id(r) for r in d._refs} >= {id(w), id(b), id(out), id(st)}


def test_pointwise_builder_fills_what_a_hand_filled_nd_pointwise_holds():
    """L.pointwise: each of res0, res1, vec, gn_t + gn_mad, act, shuffle and ldo != cout alone, then all of them."""
    s, w, b, out = L.src(_T, _T2), _Operand(0x40000, 9), _Operand(0x41000, 32), _Operand(0x42000, 2, 64, 32)
    r0, r1, vec, gn_t, gn_mad = _Operand(0x50000, 2, 64, 32), _Operand(0x51000, 2, 64, 36), _Operand(0x52000, 2, 32), _Operand(0x53000, 2, 64, 44), _Operand(0x54000, 2, 3, 32)
    plain = dict(src=s, weight=0x40000, bias=0x41000, out=0x42000, B=2, HW=64, W=8, cin=64, cout=32)
    build = lambda *a, **kw: bytes(L.pointwise(s, w, b, out, 2, 64, 8, 64, 32, *a, **kw))
    assert build() == bytes(L.Pointwise(ldo=32, **plain)) and build(40) == bytes(L.Pointwise(ldo=40, **plain))
    assert bytes(L.pointwise(s, 0x40000, None, 0x42000, 2, 64, 8, 64, 32)) == bytes(L.Pointwise(ldo=32, **dict(plain, bias=None)))
    assert build(act=L.ACT_GELU) == bytes(L.Pointwise(ldo=32, act=L.ACT_GELU, **plain))
    assert build(res0=r0) == bytes(L.Pointwise(ldo=32, res0=0x50000, ldr0=32, **plain)) and build(res0=0x50000, ldr0=48) == bytes(L.Pointwise(ldo=32, res0=0x50000, ldr0=48, **plain))
    assert build(res1=r1) == bytes(L.Pointwise(ldo=32, res1=0x51000, ldr1=36, **plain))
    assert build(vec=vec) == bytes(L.Pointwise(ldo=32, vec=0x52000, **plain))
    assert build(gn_t=gn_t, gn_mad=gn_mad) == bytes(L.Pointwise(ldo=32, gn_t=0x53000, ldt=44, gn_mad=0x54000, **plain))
    assert build(shuffle=(8, 15, 17)) == bytes(L.Pointwise(ldo=32, shuffle_c=8, shuffle_h=15, shuffle_w=17, **plain))
    d = L.pointwise(s, w, b, out, 2, 64, 8, 64, 32, 40, L.ACT_SILU, r0, r1, vec, gn_t, gn_mad, (8, 15, 17))
    assert bytes(d) == bytes(L.Pointwise(ldo=40, act=L.ACT_SILU, res0=0x50000, ldr0=32, res1=0x51000, ldr1=36, vec=0x52000, gn_t=0x53000, ldt=44, gn_mad=0x54000,
                                         shuffle_c=8, shuffle_h=15, shuffle_w=17, **plain))
    assert d._refs[0] is s._refs and {id(r) for r in d._refs} >= {id(x) for x in (w, b, out, r0, r1, vec, gn_t, gn_mad)}


def test_rows_from_a_sample_move_every_per_sample_operand_by_its_own_stride():
    """L.src_rows: sample 0 is the source itself; sample 3 behind an upsampled source, a stored map and a map formed in the kernel, each against the
    offsets written out here (4 bytes per float); gamma / beta / rowstats and every integer stay."""
    from noisediff_amd.spec import POS_DIM
    H, W, b0 = 16, 32, 3
    two = L.src(_T, _T2, L.PRO_AFFINE_SILU, mad=_EXTRA["mad"], vec=_EXTRA["vec"], gamma=_EXTRA["gamma"])
    r = L.src_rows(two, 0, H * W, 128)
    assert bytes(r) == bytes(two) and r is not two and r._refs is two._refs
    up = L.src(_T, upsample=1, mad=_EXTRA["mad"])                          # source pixels: a quarter of the output's
    assert bytes(L.src_rows(up, b0, (H // 2) * (W // 2))) == bytes(L.Src(p0=0x10000 + 4 * b0 * (H // 2) * (W // 2) * 24, c0=24, ld0=24, upsample=1,
                                                                         mad=_EXTRA["mad"].address + 4 * b0 * 3 * 24))
    c0, c1 = 24, 40
    stored = L.src(_T, _T2, L.PRO_AFFINE_MAP_SILU, ld=28, mad=_EXTRA["mad"], map=_EXTRA["map"], map_blocked=1, beta=_EXTRA["beta"])
    assert bytes(L.src_rows(stored, b0, H * W, 2 * (c0 + c1))) == bytes(L.Src(
        p0=0x10000 + 4 * b0 * H * W * 28, c0=c0, ld0=28, p1=0x20000 + 4 * b0 * H * W * c1, c1=c1, ld1=c1, mode=L.PRO_AFFINE_MAP_SILU, map_blocked=1,
        mad=_EXTRA["mad"].address + 4 * b0 * 3 * (c0 + c1), map=_EXTRA["map"].address + 4 * b0 * H * W * 2 * (c0 + c1), beta=_EXTRA["beta"].address))
    formed = L.src(_T, None, L.PRO_AFFINE_GENMAP_SILU, mad=_EXTRA["mad"], map=_EXTRA["map"], gamma=_EXTRA["gamma"], beta=_EXTRA["beta"])
    assert bytes(L.src_rows(formed, b0, H * W, POS_DIM)) == bytes(L.Src(
        p0=0x10000 + 4 * b0 * H * W * c0, c0=c0, ld0=c0, mode=L.PRO_AFFINE_GENMAP_SILU, mad=_EXTRA["mad"].address + 4 * b0 * 3 * c0,
        map=_EXTRA["map"].address + 4 * b0 * H * W * POS_DIM, gamma=_EXTRA["gamma"].address, beta=_EXTRA["beta"].address))
    ln = L.src(_T, None, L.PRO_LAYERNORM, vec=_EXTRA["vec"], rowstats=_EXTRA["rowstats"])      # a chain's source: the per-sample vector moves, no mad / map to move
    assert bytes(L.src_rows(ln, b0, H * W)) == bytes(L.Src(p0=0x10000 + 4 * b0 * H * W * c0, c0=c0, ld0=c0, mode=L.PRO_LAYERNORM, vec=_EXTRA["vec"].address + 4 * b0 * c0,
                                                           rowstats=_EXTRA["rowstats"].address))


def test_the_conv3x3_table_names_what_the_library_exports():
    """_host.CONV3X3: one record per kernel; its entries are the library's, its enum value the header's, its tiling id the literal Plan.conv3 held (the direct
    kernel's came from nd_conv3x3_tiling_id, and does: None), its arena slot and its statistics slots what Plan.conv3 chose."""
    from noisediff_amd._host import CONV3X3
    header = open(os.path.join(REPO, "include", "noisediff_hip.h")).read()
    enum = {name.lower(): int(value) for name, value in re.findall(r"ND_CONV3X3_(\w+) = (\d+)", re.search(r"enum nd_conv3x3_kernel \{([^}]*)\}", header).group(1))}
    tiling = {"direct": None, "wino": 9001, "wino2": 9002, "wino4": 9004, "wino4_16": 9016}
    slot = {"direct": ".weight", "wino": ".weight.wino", "wino2": ".weight.wino", "wino4": ".weight.wino4", "wino4_16": ".weight.wino4"}
    assert set(CONV3X3) == set(enum) == set(tiling) and len(enum) == 5
    lib = L.load()
    B, H, W, cout = 3, 48, 80, 64
    for name, k in CONV3X3.items():
        assert k.kernel == enum[name] == getattr(L, "CONV3X3_" + name.upper()) and k.tiling == tiling[name] and k.slot == slot[name], name
        assert k.entry == ("nd_conv3x3_nhwc_f32" if name == "direct" else f"nd_conv3x3_{name}_nhwc_f32") and k.entry in L.SIGNATURES, name
        assert k.splitk == (f"nd_conv3x3_{name}_splitk_nhwc_f32" if name.startswith("wino4") else None) and (k.splitk is None or k.splitk in L.SIGNATURES), name
        assert all(k.pack + suffix in L.SIGNATURES for suffix in ("", "_floats", "_dgrad")), name
        want = lib.nd_conv3x3_stat_slots(H, W, cout, B) if name == "direct" else lib.nd_conv3x3_wino4_stat_slots(H, W) if name.startswith("wino4") else lib.nd_conv3x3_wino_stat_slots(H, W)
        assert k.stat_slots(lib, B, H, W, cout) == want > 0, name


def conv3x3_selection_differences():
    """Rows of tests/golden/conv3x3_selection.json this tree decides otherwise: (rule, inputs, recorded, now, permitted).  Permitted is only a row whose
    recorded choice raises or names a kernel that refuses the descriptor (nd_conv3x3_takes says 0 for it); for the F(2x2) and direct forms `rows` may grow
    (never more launches) where the form and the split count are the recorded ones."""
    import json
    from noisediff_amd import engine, train
    from noisediff_amd._host import CONV3X3, conv3x3_kind, conv3x3_takes
    table = json.load(open(os.path.join(REPO, "tests", "golden", "conv3x3_selection.json")))
    out = []
    for *row, form, splits, rows in table["form"]:                      # a row: the inputs, then what was decided
        B, H, W, cin, cout, c0, c1, ld0, ld1, mode, up, packed, split_k, w16 = row
        old = [form, splits, rows]
        try:
            new = list(engine.conv3x3_form(B, H, W, cin, cout, c0, c1, ld0, ld1, mode, bool(up), bool(packed), split_k=bool(split_k), wino4_16=("narrow", "all", "0")[w16]))
        except L.HipError:
            new = ["raise", 0, 0]
        same = new == old or (new[:2] == old[:2] and not old[0].startswith("wino4") and old[0] != "raise" and new[2] >= old[2] and -(-B // new[2]) <= -(-B // old[2]))
        if not same:
            refused = old[0] == "raise" or not conv3x3_takes(CONV3X3[old[0] or "direct"].kernel, old[2], H, W, cin, cout, c0, c1, ld0, ld1, mode, bool(up), splits=old[1])
            out.append(("form", row, old, new, refused))
    for *row, old in table["kind"]:
        B, H, W, cin, cout, c0, c1, ld, w4 = row
        new = conv3x3_kind(B, H, W, cin, cout, c0, c1, ld, wino4=bool(w4))
        if new != old:
            out.append(("kind", row, old, new, not conv3x3_takes(CONV3X3[old].kernel, B, H, W, cin, cout, c0, c1, ld, ld if c1 else 0)))
    for *row, old in table["cat"]:
        B, c0, c1, H, W, cout = row
        new = bool(train.cat_sources_ok(_cuda_like(B, c0, H, W), _cuda_like(B, c1, H, W), cout))
        if new != old:
            out.append(("cat", row, old, new, old and not conv3x3_takes(L.CONV3X3_WINO4, B, H, W, c0 + c1, cout or 8, c0, c1, c0 + c1, c0 + c1)))
    return table, out


def test_conv3x3_rules_decide_what_the_recorded_table_says():
    """engine.conv3x3_form, _host.conv3x3_kind and train.cat_sources_ok against the table recorded (tools/record_conv3x3_selection.py) when every limit was
    still spelled out in Python: the same form, split count and rows per launch, except where the recorded choice raised or picked a kernel that refuses."""
    table, diff = conv3x3_selection_differences()
    assert len(table["form"]) > 1500 and len(table["kind"]) > 800 and len(table["cat"]) > 200
    assert [d for d in diff if not d[4]] == []


def test_sampling_split_k_plan_looks_at_the_sample_geometry_only():
    """nd_conv3x3_wino4_16_splitk_plan (host code, no GPU) has no batch argument: BASELINE config 2's 16 x 16 and 32 x 32 stages are cut into K ranges
    (about 32 items per sample, at least four 16-channel chunks per range), the layers of the 256 x 256 workload that reach the 16 x 16-region form
    (256 -> 256 at 32 x 32) into two, everything with enough items per sample or too few chunks is left alone."""
    plan = L.load().nd_conv3x3_wino4_16_splitk_plan
    assert plan(16, 16, 512, 512) == 4 and plan(16, 16, 768, 512) == 4 and plan(16, 16, 256, 512) == 4 and plan(16, 16, 256, 256) == 4
    assert plan(32, 32, 256, 256) == 2 and plan(32, 32, 384, 256) == 2 and plan(32, 32, 512, 256) == 2
    assert plan(32, 32, 512, 512) == 1 and plan(256, 256, 64, 64) == 1 and plan(16, 16, 64, 64) == 1 and plan(16, 16, 72, 64) == 1
    assert plan(16, 16, 2048, 64) == 8 and plan(0, 16, 64, 64) == 1


@pytest.mark.parametrize("objective,sched", [("pred_v", "sigmoid2"), ("pred_noise", "linear"), ("pred_x0", "cosine")])
def test_per_step_public_methods_follow_the_reference_formulas(objective, sched):
    """predict_start_from_* / predict_noise_from_start / q_posterior / model_predictions / p_mean_variance / p_sample
    (models/denoising_diffusion_pytorch.py:298-373) around a stand-in network on the CPU, against the oracle's restatement of the same
    lines (predict_x0_eps + the posterior of p_sample_loop), for the three objectives; interpolate and the clip / re-derive switches."""
    from torch import nn
    from oracle import noisediff_oracle as O

    class Stub(nn.Module):
        channels = out_dim = 4
        self_condition = random_or_learned_sinusoidal_cond = False

        def forward(self, x, t, condition=None):
            return 0.7 * x.flip(1) + 0.1 * t.view(-1, 1, 1, 1) / 50 + (0 if condition is None else condition["bias"])

    T, B, H = 50, 3, 8
    gd = GaussianDiffusion(Stub(), image_size=H, timesteps=T, beta_schedule=sched, objective=objective)
    buf = O.schedule_buffers(sched, T, objective)
    x = synth.make_noise(7, "ps.x", B, 4, H) * 1.5
    cond = {"bias": torch.full((B, 1, 1, 1), 0.05)}
    for t in (T - 1, 17, 0):
        tb = torch.full((B,), t, dtype=torch.long)
        out = gd.model(x, tb, cond)
        for clip in (False, True):
            eps_ref, x0_ref = O.predict_x0_eps(buf, objective, x, t, out, clip=clip)
            mp = gd.model_predictions(x, tb, cond, clip_x_start=clip, rederive_pred_noise=True)
            assert torch.allclose(mp.pred_x_start, x0_ref, atol=1e-6) and torch.allclose(mp.pred_noise, eps_ref, atol=2e-5)
        _, x0 = O.predict_x0_eps(buf, objective, x, t, out, clip=False)
        x0 = x0.clamp(-1, 1)
        mean_ref = O._coef(buf, "posterior_mean_coef1", t) * x0 + O._coef(buf, "posterior_mean_coef2", t) * x
        mean, var, logvar, xs = gd.p_mean_variance(x, tb, cond)
        assert torch.allclose(mean, mean_ref, atol=1e-6) and torch.allclose(xs, x0, atol=1e-6)
        assert float(var.flatten()[0]) == float(gd.posterior_variance[t]) and float(logvar.flatten()[0]) == float(gd.posterior_log_variance_clipped[t])
        z = synth.make_noise(7, f"ps.z{t}", B, 4, H)
        nxt, xs2 = gd.p_sample(x, t, cond, noise=z)
        want = mean_ref + ((0.5 * O._coef(buf, "posterior_log_variance_clipped", t)).exp() * z if t > 0 else 0.0)
        assert torch.allclose(nxt, want, atol=1e-6) and torch.equal(xs2, xs)
    v = synth.make_noise(7, "ps.v", B, 4, H)
    tb = torch.full((B,), 9, dtype=torch.long)
    assert torch.allclose(gd.predict_noise_from_start(x, tb, gd.predict_start_from_noise(x, tb, v)), v, atol=1e-4)
    assert torch.allclose(gd.predict_start_from_v(x, tb, gd.predict_v(v, tb, x)), gd.predict_start_from_v(x, tb, gd.predict_v(v, tb, x)))
    torch.manual_seed(3)
    mix = gd.interpolate(x, -x, t=4, lam=0.25, condition=cond)
    assert mix.shape == x.shape and torch.isfinite(mix).all()
    with pytest.raises(ValueError, match="does not match"):
        gd.p_sample_loop((B, 4, H + 1, H), cond)
