"""The sampler's non-convolution kernels at the shapes a sampling step runs, against float64 on the CPU.

``INFER_SHAPES`` lists every (entry point, integer arguments) pair that is not a 3x3 convolution or a pointwise GEMM / chain in the recorded launch
lists (``Plan.cond_ops`` / ``Plan.step_ops``) of the benchmark's configurations and of the two per-stage attention wirings of
tests/test_stage_attn.py; a re-recorded plan pins it to the product.  The sampler update is launched by ``diffusion._Loop``, not by the plan: its
(B, H W, 4) per configuration is ``SAMPLER_SHAPES``.  The tests then run each kernel at those shapes and at the edges next to them -- second trips
of the capped grids, strides wider than the channel count, every template instance -- with outputs pre-filled with NaN and wider than the kernel
writes: the written region is finite and right, the columns and rows beyond it are still NaN.

Criterion: O(1) outputs use ``util.close`` (TOL = 2e-5 and the element-wise floor).  Where the output scale is far from 1 or TOL is
not known to hold for a correct fp32 evaluation, the bound is derived from the reference: the same formula in fp32 torch on the CPU, its error against
float64 on the same inputs; the kernel may be 4 x that far off plus one fp32 ulp of max|ref| (``derived``).  The figures of every check are logged to
ND_TEST_ELEM_LOG (profiles/infer_kernels_float64.txt)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from noisediff_amd import _lib as L, synth
from oracle import noisediff_oracle as O
from util import close, derived

TOL = 2e-5
ULP = 2.0 ** -23

# configuration -> (dim, size, batch, Engine keywords): bench.py's presets and the per-stage attention wirings of tests/test_stage_attn.py
CONFIGS = {
    "headline": (64, 256, 16, {}),
    "cfg2": (64, 128, 16, {}),
    "cfg4": (128, 256, 8, {"mid_attn": True}),
    "ref48": (48, 512, 4, {}),
    "stage16": (16, 64, 2, {"stage_attn": True}),
    "stage64": (64, 128, 2, {"stage_attn": ("linear", None, "linear", "full")}),
}
# the sampler update (nd_sampler_step_*_f32): (B, H W, 4) per configuration, launched by diffusion._Loop on plan.x / plan.model_out
SAMPLER_SHAPES = {name: (b, s * s, 4) for name, (_, s, b, _) in CONFIGS.items()}


# (entry point, its integer arguments in the order of the C prototype) -> the configurations whose plan launches it.  Strides first where the entry has them:
# affine_silu_add (ldt, ldr0, ldr1, ldo, B, HW, C); attention / linear attention (ld_qkv, ld_out, B, N, heads, dh); cond_step_ptable (ld_out, B, dim, J, table rows);
# conv7x7 (ldo, B, H, W, cout); embedding_rows (B, rows, dim); groupnorm_finalize (slots, ld_ss, B, C, groups); layernorm_stats (ldx, B, HW, C);
# linear_rows (ld_in, ld_out, B, K, N, act_in, act_out); pos_enc (B, H, W, hid); rmsnorm (ldx, ldo, B, HW, C); rmsnorm_add (ldx, ldr, ldo, B, HW, C).
INFER_SHAPES = {
    ('nd_affine_silu_add_f32', (8, 8, 8, 8, 2, 16384, 8)): ('stage64',),
    ('nd_affine_silu_add_f32', (8, 8, 8, 8, 4, 262144, 8)): ('ref48',),
    ('nd_affine_silu_add_f32', (8, 8, 8, 8, 8, 65536, 8)): ('cfg4',),
    ('nd_affine_silu_add_f32', (8, 8, 8, 8, 16, 16384, 8)): ('cfg2',),
    ('nd_affine_silu_add_f32', (8, 8, 8, 8, 16, 65536, 8)): ('headline',),
    ('nd_affine_silu_add_f32', (16, 16, 16, 16, 2, 1024, 16)): ('stage16',),
    ('nd_affine_silu_add_f32', (16, 16, 16, 16, 2, 4096, 16)): ('stage16',),
    ('nd_affine_silu_add_f32', (32, 32, 32, 32, 2, 256, 32)): ('stage16',),
    ('nd_affine_silu_add_f32', (48, 48, 48, 48, 4, 65536, 48)): ('ref48',),
    ('nd_affine_silu_add_f32', (48, 48, 48, 48, 4, 262144, 48)): ('ref48',),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 2, 64, 64)): ('stage16',),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 2, 4096, 64)): ('stage64',),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 2, 16384, 64)): ('stage64',),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 16, 4096, 64)): ('cfg2',),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 16, 16384, 64)): ('headline', 'cfg2'),
    ('nd_affine_silu_add_f32', (64, 64, 64, 64, 16, 65536, 64)): ('headline',),
    ('nd_affine_silu_add_f32', (96, 96, 96, 96, 4, 16384, 96)): ('ref48',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 2, 64, 128)): ('stage16',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 2, 1024, 128)): ('stage64',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 8, 16384, 128)): ('cfg4',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 8, 65536, 128)): ('cfg4',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 16, 1024, 128)): ('cfg2',),
    ('nd_affine_silu_add_f32', (128, 128, 128, 128, 16, 4096, 128)): ('headline',),
    ('nd_affine_silu_add_f32', (192, 192, 192, 192, 4, 4096, 192)): ('ref48',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 2, 256, 256)): ('stage64',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 2, 1024, 256)): ('stage64',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 8, 4096, 256)): ('cfg4',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 8, 16384, 256)): ('cfg4',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 16, 256, 256)): ('cfg2',),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 16, 1024, 256)): ('headline', 'cfg2'),
    ('nd_affine_silu_add_f32', (256, 256, 256, 256, 16, 4096, 256)): ('headline',),
    ('nd_affine_silu_add_f32', (384, 384, 384, 384, 4, 4096, 384)): ('ref48',),
    ('nd_affine_silu_add_f32', (512, 512, 512, 512, 2, 256, 512)): ('stage64',),
    ('nd_affine_silu_add_f32', (512, 512, 512, 512, 8, 1024, 512)): ('cfg4',),
    ('nd_affine_silu_add_f32', (512, 512, 512, 512, 8, 4096, 512)): ('cfg4',),
    ('nd_affine_silu_add_f32', (512, 512, 512, 512, 16, 256, 512)): ('cfg2',),
    ('nd_affine_silu_add_f32', (512, 512, 512, 512, 16, 1024, 512)): ('headline',),
    ('nd_affine_silu_add_f32', (1024, 1024, 1024, 1024, 8, 1024, 1024)): ('cfg4',),
    ('nd_attention_mfma_f32', (384, 128, 2, 64, 4, 32)): ('stage16',),
    ('nd_attention_mfma_f32', (384, 128, 2, 256, 4, 32)): ('stage64',),
    ('nd_attention_mfma_f32', (384, 128, 8, 1024, 4, 32)): ('cfg4',),
    ('nd_cond_step_ptable_f32', (2048, 2, 16, 2048, 1000)): ('stage16',),
    ('nd_cond_step_ptable_f32', (6144, 4, 48, 6144, 1000)): ('ref48',),
    ('nd_cond_step_ptable_f32', (8192, 2, 64, 8192, 1000)): ('stage64',),
    ('nd_cond_step_ptable_f32', (8192, 16, 64, 8192, 1000)): ('headline', 'cfg2'),
    ('nd_cond_step_ptable_f32', (16384, 8, 128, 16384, 1000)): ('cfg4',),
    ('nd_conv7x7_c4_split_f32', (16, 2, 64, 64, 16)): ('stage16',),
    ('nd_conv7x7_c4_split_f32', (48, 4, 512, 512, 48)): ('ref48',),
    ('nd_conv7x7_c4_split_f32', (64, 2, 128, 128, 64)): ('stage64',),
    ('nd_conv7x7_c4_split_f32', (64, 16, 128, 128, 64)): ('cfg2',),
    ('nd_conv7x7_c4_split_f32', (64, 16, 256, 256, 64)): ('headline',),
    ('nd_conv7x7_c4_split_f32', (128, 8, 256, 256, 128)): ('cfg4',),
    ('nd_embedding_rows_f32', (2, 100, 16)): ('stage16', 'stage64'),
    ('nd_embedding_rows_f32', (4, 100, 16)): ('ref48',),
    ('nd_embedding_rows_f32', (8, 100, 16)): ('cfg4',),
    ('nd_embedding_rows_f32', (16, 100, 16)): ('headline', 'cfg2'),
    ('nd_groupnorm_finalize_f32', (1, 2048, 2, 32, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (1, 2048, 2, 64, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (1, 8192, 2, 256, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (1, 8192, 2, 512, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (1, 8192, 16, 256, 8)): ('cfg2',),
    ('nd_groupnorm_finalize_f32', (1, 8192, 16, 512, 8)): ('cfg2',),
    ('nd_groupnorm_finalize_f32', (2, 2048, 2, 64, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (2, 2048, 2, 128, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (4, 2048, 2, 32, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (4, 8192, 2, 128, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (4, 8192, 2, 256, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (4, 8192, 16, 128, 8)): ('cfg2',),
    ('nd_groupnorm_finalize_f32', (4, 8192, 16, 256, 8)): ('headline', 'cfg2'),
    ('nd_groupnorm_finalize_f32', (4, 8192, 16, 512, 8)): ('headline',),
    ('nd_groupnorm_finalize_f32', (4, 16384, 8, 512, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (4, 16384, 8, 1024, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (8, 2048, 2, 16, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (16, 2048, 2, 16, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (16, 6144, 4, 192, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (16, 6144, 4, 384, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (16, 8192, 2, 64, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (16, 8192, 2, 128, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (16, 8192, 16, 64, 8)): ('cfg2',),
    ('nd_groupnorm_finalize_f32', (16, 8192, 16, 128, 8)): ('headline', 'cfg2'),
    ('nd_groupnorm_finalize_f32', (16, 8192, 16, 256, 8)): ('headline',),
    ('nd_groupnorm_finalize_f32', (16, 16384, 8, 256, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (16, 16384, 8, 512, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (32, 2048, 2, 16, 2)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (32, 2048, 2, 16, 8)): ('stage16',),
    ('nd_groupnorm_finalize_f32', (64, 6144, 4, 96, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (64, 6144, 4, 192, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (64, 8192, 2, 64, 2)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (64, 8192, 2, 64, 8)): ('stage64',),
    ('nd_groupnorm_finalize_f32', (64, 8192, 16, 64, 2)): ('cfg2',),
    ('nd_groupnorm_finalize_f32', (64, 8192, 16, 64, 8)): ('headline', 'cfg2'),
    ('nd_groupnorm_finalize_f32', (64, 8192, 16, 128, 8)): ('headline',),
    ('nd_groupnorm_finalize_f32', (64, 16384, 8, 128, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (64, 16384, 8, 256, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (256, 6144, 4, 48, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (256, 6144, 4, 96, 8)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (256, 8192, 16, 64, 2)): ('headline',),
    ('nd_groupnorm_finalize_f32', (256, 8192, 16, 64, 8)): ('headline',),
    ('nd_groupnorm_finalize_f32', (256, 16384, 8, 128, 2)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (256, 16384, 8, 128, 8)): ('cfg4',),
    ('nd_groupnorm_finalize_f32', (1024, 6144, 4, 48, 2)): ('ref48',),
    ('nd_groupnorm_finalize_f32', (1024, 6144, 4, 48, 8)): ('ref48',),
    ('nd_layernorm_stats_f32', (96, 4, 16384, 96)): ('ref48',),
    ('nd_layernorm_stats_f32', (96, 4, 65536, 96)): ('ref48',),
    ('nd_layernorm_stats_f32', (128, 2, 64, 128)): ('stage16',),
    ('nd_layernorm_stats_f32', (128, 2, 1024, 128)): ('stage64',),
    ('nd_layernorm_stats_f32', (128, 2, 4096, 128)): ('stage64',),
    ('nd_layernorm_stats_f32', (128, 8, 16384, 128)): ('cfg4',),
    ('nd_layernorm_stats_f32', (128, 8, 65536, 128)): ('cfg4',),
    ('nd_layernorm_stats_f32', (128, 16, 1024, 128)): ('cfg2',),
    ('nd_layernorm_stats_f32', (128, 16, 4096, 128)): ('headline', 'cfg2'),
    ('nd_layernorm_stats_f32', (128, 16, 16384, 128)): ('headline',),
    ('nd_layernorm_stats_f32', (192, 4, 4096, 192)): ('ref48',),
    ('nd_layernorm_stats_f32', (192, 4, 16384, 192)): ('ref48',),
    ('nd_layernorm_stats_f32', (256, 2, 256, 256)): ('stage64',),
    ('nd_layernorm_stats_f32', (256, 2, 1024, 256)): ('stage64',),
    ('nd_layernorm_stats_f32', (256, 8, 4096, 256)): ('cfg4',),
    ('nd_layernorm_stats_f32', (256, 8, 16384, 256)): ('cfg4',),
    ('nd_layernorm_stats_f32', (256, 16, 256, 256)): ('cfg2',),
    ('nd_layernorm_stats_f32', (256, 16, 1024, 256)): ('headline', 'cfg2'),
    ('nd_layernorm_stats_f32', (256, 16, 4096, 256)): ('headline',),
    ('nd_layernorm_stats_f32', (384, 4, 4096, 384)): ('ref48',),
    ('nd_layernorm_stats_f32', (512, 2, 256, 512)): ('stage64',),
    ('nd_layernorm_stats_f32', (512, 8, 1024, 512)): ('cfg4',),
    ('nd_layernorm_stats_f32', (512, 8, 4096, 512)): ('cfg4',),
    ('nd_layernorm_stats_f32', (512, 16, 256, 512)): ('cfg2',),
    ('nd_layernorm_stats_f32', (512, 16, 1024, 512)): ('headline',),
    ('nd_layernorm_stats_f32', (1024, 8, 1024, 1024)): ('cfg4',),
    ('nd_linear_attention_f32', (384, 128, 2, 256, 4, 32)): ('stage16',),
    ('nd_linear_attention_f32', (384, 128, 2, 1024, 4, 32)): ('stage16', 'stage64'),
    ('nd_linear_attention_f32', (384, 128, 2, 4096, 4, 32)): ('stage16',),
    ('nd_linear_attention_f32', (384, 128, 2, 16384, 4, 32)): ('stage64',),
    ('nd_linear_rows_f32', (16, 128, 2, 16, 128, 0, 0)): ('stage16', 'stage64'),
    ('nd_linear_rows_f32', (16, 128, 4, 16, 128, 0, 0)): ('ref48',),
    ('nd_linear_rows_f32', (16, 128, 8, 16, 128, 0, 0)): ('cfg4',),
    ('nd_linear_rows_f32', (16, 128, 16, 16, 128, 0, 0)): ('headline', 'cfg2'),
    ('nd_linear_rows_f32', (128, 16, 2, 128, 16, 0, 0)): ('stage16',),
    ('nd_linear_rows_f32', (128, 32, 2, 128, 32, 0, 0)): ('stage16',),
    ('nd_linear_rows_f32', (128, 48, 4, 128, 48, 0, 0)): ('ref48',),
    ('nd_linear_rows_f32', (128, 64, 2, 128, 64, 0, 0)): ('stage16', 'stage64'),
    ('nd_linear_rows_f32', (128, 64, 16, 128, 64, 0, 0)): ('headline', 'cfg2'),
    ('nd_linear_rows_f32', (128, 96, 4, 128, 96, 0, 0)): ('ref48',),
    ('nd_linear_rows_f32', (128, 128, 2, 128, 128, 0, 0)): ('stage16', 'stage64'),
    ('nd_linear_rows_f32', (128, 128, 8, 128, 128, 0, 0)): ('cfg4',),
    ('nd_linear_rows_f32', (128, 128, 16, 128, 128, 0, 0)): ('headline', 'cfg2'),
    ('nd_linear_rows_f32', (128, 192, 4, 128, 192, 0, 0)): ('ref48',),
    ('nd_linear_rows_f32', (128, 256, 2, 128, 256, 0, 0)): ('stage64',),
    ('nd_linear_rows_f32', (128, 256, 8, 128, 256, 0, 0)): ('cfg4',),
    ('nd_linear_rows_f32', (128, 256, 16, 128, 256, 0, 0)): ('headline', 'cfg2'),
    ('nd_linear_rows_f32', (128, 384, 4, 128, 384, 0, 0)): ('ref48',),
    ('nd_linear_rows_f32', (128, 512, 2, 128, 512, 0, 0)): ('stage64',),
    ('nd_linear_rows_f32', (128, 512, 8, 128, 512, 0, 0)): ('cfg4',),
    ('nd_linear_rows_f32', (128, 512, 16, 128, 512, 0, 0)): ('headline', 'cfg2'),
    ('nd_linear_rows_f32', (128, 1024, 8, 128, 1024, 0, 0)): ('cfg4',),
    ('nd_pos_enc_f32', (2, 64, 64, 8)): ('stage16',),
    ('nd_pos_enc_f32', (2, 128, 128, 8)): ('stage64',),
    ('nd_pos_enc_f32', (4, 512, 512, 8)): ('ref48',),
    ('nd_pos_enc_f32', (8, 256, 256, 8)): ('cfg4',),
    ('nd_pos_enc_f32', (16, 128, 128, 8)): ('cfg2',),
    ('nd_pos_enc_f32', (16, 256, 256, 8)): ('headline',),
    ('nd_rmsnorm_add_nhwc_f32', (16, 16, 16, 2, 1024, 16)): ('stage16',),
    ('nd_rmsnorm_add_nhwc_f32', (16, 16, 16, 2, 4096, 16)): ('stage16',),
    ('nd_rmsnorm_add_nhwc_f32', (32, 32, 32, 2, 256, 32)): ('stage16',),
    ('nd_rmsnorm_add_nhwc_f32', (32, 32, 32, 2, 1024, 32)): ('stage16',),
    ('nd_rmsnorm_add_nhwc_f32', (64, 64, 64, 2, 256, 64)): ('stage16',),
    ('nd_rmsnorm_add_nhwc_f32', (64, 64, 64, 2, 16384, 64)): ('stage64',),
    ('nd_rmsnorm_add_nhwc_f32', (128, 128, 128, 2, 1024, 128)): ('stage64',),
    ('nd_rmsnorm_add_nhwc_f32', (256, 256, 256, 2, 1024, 256)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (16, 16, 2, 1024, 16)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (16, 16, 2, 4096, 16)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (32, 32, 2, 256, 32)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (32, 32, 2, 1024, 32)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (64, 64, 2, 64, 64)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (64, 64, 2, 256, 64)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (64, 64, 2, 16384, 64)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (128, 128, 2, 64, 128)): ('stage16',),
    ('nd_rmsnorm_nhwc_f32', (128, 128, 2, 1024, 128)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (256, 256, 2, 256, 256)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (256, 256, 2, 1024, 256)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (512, 512, 2, 256, 512)): ('stage64',),
    ('nd_rmsnorm_nhwc_f32', (1024, 1024, 8, 1024, 1024)): ('cfg4',),
}


def record_plans():
    """{(entry point, its integer arguments in order): configurations} of every recorded launch that is not a 3x3 convolution or a pointwise GEMM / chain."""
    from noisediff_amd.engine import Engine
    seen = {}
    for name, (dim, size, batch, kw) in CONFIGS.items():
        eng = Engine(dim, torch.device("cuda", 0), **kw)
        plan = eng.plan(batch, size, size, allow_empty=True)
        for _fn, args, entry, _meta in plan.cond_ops + plan.step_ops:
            if "conv3x3" in entry or "pointwise" in entry:
                continue
            types = L.SIGNATURES[entry][1]
            ints = tuple(int(a) for a, t in zip(args, types) if t in (L.i32, L.i64))
            cfgs = seen.setdefault((entry, ints), [])
            if name not in cfgs:
                cfgs.append(name)
        del plan, eng
        torch.cuda.empty_cache()
    return {k: tuple(v) for k, v in seen.items()}


# ====================================================================================================== helpers
@pytest.fixture(scope="module")
def ctx():
    import hiputil as hu
    return hu.Ctx()


def U(name, shape, lo=-1.0, hi=1.0):
    """Small named inputs (the repository's hash streams)."""
    return synth.uniform(29, name, shape, lo, hi)


def R(seed, shape, lo=-1.0, hi=1.0):
    """Large inputs: torch's CPU generator (the hash streams take seconds per ten million values)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo


def _log(line):
    path = os.environ.get("ND_TEST_ELEM_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?')}: {line}\n")


def o1(got, ref64, what=""):
    """O(1) outputs: finite, then both criteria of DESIGN section 6 against float64."""
    got = torch.as_tensor(got)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values in the written region"
    close(got.double().numpy(), torch.as_tensor(ref64).double().numpy(), TOL)


def untouched(buf, cols, rows=None, what=""):
    """The canary: columns ``cols``.. of every row and rows ``rows``.. of a NaN-filled buffer are still NaN."""
    b = buf.reshape(-1, buf.shape[-1]) if rows is None else buf
    assert bool(torch.isnan(b[..., cols:]).all()), f"{what}: wrote past column {cols}"
    if rows is not None:
        assert bool(torch.isnan(buf[rows:]).all()), f"{what}: wrote past row {rows}"


def rows_of(entry):
    return sorted(k[1] for k in INFER_SHAPES if k[0] == entry)


# ====================================================================================================== 1. the table is the product's
def test_the_shape_table_is_what_the_plans_launch():
    """Re-records Engine.plan(B, H, W, allow_empty=True) of every configuration: the launches that are not 3x3 convolutions or pointwise GEMMs are exactly
    INFER_SHAPES, configuration by configuration; the sampler's (B, H W, 4) follows the same configurations."""
    seen = record_plans()
    assert not set(seen) - set(INFER_SHAPES), f"launches missing from INFER_SHAPES: {sorted(set(seen) - set(INFER_SHAPES))}"
    assert not set(INFER_SHAPES) - set(seen), f"INFER_SHAPES rows no plan launches: {sorted(set(INFER_SHAPES) - set(seen))}"
    assert seen == INFER_SHAPES, {k: (seen[k], INFER_SHAPES[k]) for k in seen if seen[k] != INFER_SHAPES[k]}
    assert SAMPLER_SHAPES["headline"] == (16, 65536, 4) and set(SAMPLER_SHAPES) == set(CONFIGS)
    for entry in ("nd_linear_attention_f32", "nd_rmsnorm_add_nhwc_f32", "nd_rmsnorm_nhwc_f32", "nd_attention_mfma_f32", "nd_layernorm_stats_f32",
                  "nd_affine_silu_add_f32", "nd_groupnorm_finalize_f32", "nd_linear_rows_f32", "nd_pos_enc_f32", "nd_embedding_rows_f32"):
        assert rows_of(entry), entry


# ====================================================================================================== 2. attention
DH = 32
ATT_N = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1024, 4096]
HEADS_B = [(1, 1), (4, 1), (1, 3), (4, 3)]


def _qkv(tag, kind, B, N, heads, seed):
    """(B, N, 3 hid) q | k | v.  'uniform': U(-2, 2).  'rising': k_j = 0.25 u_j + d 12 j / N, q = 0.25 u + 4 d for a unit vector d per head -- logits up to
    about 11 and a running maximum that moves in every key tile.  'wide_k' (linear attention): k columns spanning +-20 along the pixels."""
    hid = heads * DH
    if kind == "uniform":
        return R(seed, (B, N, 3 * hid), -2, 2)
    u = R(seed, (B, N, 3, heads, DH))
    q, k, v = u[:, :, 0].clone(), u[:, :, 1].clone(), 2 * u[:, :, 2]
    if kind == "rising":
        d = F.normalize(R(seed + 1, (heads, DH)), dim=-1)
        ramp = torch.arange(N, dtype=torch.float32)[None, :, None, None] / N
        q, k = 0.25 * q + 4 * d, 0.25 * k + d * 12 * ramp
    else:
        k = 20 * k
    return torch.stack((q, k, v), 2).reshape(B, N, 3 * hid).contiguous()


def _strided(t, ld):
    """Device copy of (rows..., C) with pixel stride ld >= C; the pad columns hold NaN (a kernel that reads them poisons its output)."""
    import hiputil as hu
    buf = torch.full(t.shape[:-1] + (ld,), float("nan"))
    buf[..., :t.shape[-1]] = t
    return hu.dev(buf)


def _attention_ref64(qkv, B, N, heads):
    """softmax(q k^T / sqrt(dh)) v in float64, head by head (N = 4096 stays under 1 GB)."""
    hid = heads * DH
    x = qkv.double().reshape(B, N, 3, heads, DH)
    out = torch.empty(B, N, hid, dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            out[b, :, h * DH:(h + 1) * DH] = torch.softmax(q @ k.T * DH ** -0.5, -1) @ v
    return out


@pytest.mark.parametrize("kind", ["uniform", "rising"])
@pytest.mark.parametrize("N", ATT_N)
def test_attention_mfma_against_float64(ctx, N, kind):
    """nd_attention_mfma_f32 at every tail of the 128-query / 64-key / 32-key tiling, heads in {1, 4}, B in {1, 3}, ld_qkv = 3 hid + 8, ld_out = hid + 4.
    The rising input moves the running maximum in every key tile (the alpha rescale of o and l_run), and from N = 1024 on whole 32-key sub-tiles lie far
    below it.  The fp32 torch evaluation stays within 6e-7 of float64 on both inputs up to N = 4096 (measured), so TOL holds for a correct kernel."""
    import hiputil as hu
    for heads, B in HEADS_B:
        hid = heads * DH
        qkv = _qkv("att", kind, B, N, heads, 1000 + N)
        qd = _strided(qkv, 3 * hid + 8)
        out = hu.full((B * N + 2, hid + 4))
        L.call("nd_attention_mfma_f32", qd.data_ptr(), 3 * hid + 8, out.data_ptr(), hid + 4, B, N, heads, DH, ctx.stream)
        ctx.sync()
        got = out.cpu()
        o1(got[:B * N, :hid].reshape(B, N, hid), _attention_ref64(qkv, B, N, heads), f"heads {heads} B {B}")
        untouched(got, hid, B * N, f"heads {heads} B {B}")


def test_attention_mfma_at_the_table_rows(ctx):
    """The launches of INFER_SHAPES (dense strides, as the engine passes them)."""
    import hiputil as hu
    for ldq, ldo, B, N, heads, dh in rows_of("nd_attention_mfma_f32"):
        qkv = _qkv("att", "rising", B, N, heads, 77)
        qd, out = _strided(qkv, ldq), hu.full((B * N + 2, ldo))
        L.call("nd_attention_mfma_f32", qd.data_ptr(), ldq, out.data_ptr(), ldo, B, N, heads, dh, ctx.stream)
        ctx.sync()
        got = out.cpu()
        o1(got[:B * N].reshape(B, N, ldo), _attention_ref64(qkv, B, N, heads), str((B, N, heads)))
        untouched(got, ldo, B * N)


# ====================================================================================================== 3. linear attention
LA_N = [1, 31, 33, 64, 2047, 2048, 2049, 4096 + 200, 65536]


def _linear_attention_ref(qkv, B, N, heads, dtype):
    """LinearAttention.forward's core (Diffusion_arch.py:223-234) in ``dtype``, in the reference's operation order."""
    q, k, v = (t.reshape(B, N, heads, DH).permute(0, 2, 3, 1) for t in qkv.to(dtype).chunk(3, dim=-1))      # b h c n
    q = q.softmax(dim=-2) * DH ** -0.5
    k = k.softmax(dim=-1)
    ctxm = torch.einsum("bhdn,bhen->bhde", k, v)
    return torch.einsum("bhde,bhdn->bhen", ctxm, q).permute(0, 3, 1, 2).reshape(B, N, heads * DH)


@pytest.mark.parametrize("kind", ["uniform", "wide_k"])
@pytest.mark.parametrize("N", LA_N)
def test_linear_attention_against_float64(ctx, N, kind):
    """nd_linear_attention_f32 around the 32-row statistics merge (N < 32: empty row partials) and the 2048-pixel chunks, up to a full-resolution stage's
    65536 tokens; 'wide_k' spreads the k columns over +-20 (the online max / sum-exp of la_kstat_kernel and its merge).  The outputs shrink with N
    (max|ref| 0.079 at N = 64, 0.0024 at 65536), so the scale is max|ref| and the bound is the derived one.  Twice: the same bits (fixed reduction order).
    The workspace is exactly nd_linear_attention_workspace_floats, with a NaN canary behind it."""
    import hiputil as hu
    for heads, B in HEADS_B:
        hid = heads * DH
        qkv = _qkv("lat", kind, B, N, heads, 2000 + N)
        qd = _strided(qkv, 3 * hid + 8)
        nws = int(ctx.lib.nd_linear_attention_workspace_floats(B, N, heads))
        assert nws == B * heads * (2 * DH + -(-N // 2048) * DH * DH)
        runs = []
        for _ in range(2):
            out, ws = hu.full((B * N + 2, hid + 4)), hu.full((nws + 64,))
            L.call("nd_linear_attention_f32", qd.data_ptr(), 3 * hid + 8, out.data_ptr(), hid + 4, ws.data_ptr(), B, N, heads, DH, ctx.stream)
            ctx.sync()
            wsc = ws.cpu()
            assert bool(torch.isfinite(wsc[:nws]).all()) and bool(torch.isnan(wsc[nws:]).all()), "workspace"
            runs.append(out.cpu())
        got = runs[0]
        assert torch.equal(torch.nan_to_num(runs[0], nan=7.0), torch.nan_to_num(runs[1], nan=7.0)), "not bitwise repeatable"
        derived(got[:B * N, :hid], _linear_attention_ref(qkv, B, N, heads, torch.float64), _linear_attention_ref(qkv, B, N, heads, torch.float32),
                f"heads {heads} B {B}")
        untouched(got, hid, B * N, f"heads {heads} B {B}")


def test_linear_attention_at_the_table_rows(ctx):
    import hiputil as hu
    for ldq, ldo, B, N, heads, dh in rows_of("nd_linear_attention_f32"):
        qkv = _qkv("lat", "uniform", B, N, heads, 78)
        qd, out = _strided(qkv, ldq), hu.full((B * N + 2, ldo))
        ws = hu.full((int(ctx.lib.nd_linear_attention_workspace_floats(B, N, heads)),))
        L.call("nd_linear_attention_f32", qd.data_ptr(), ldq, out.data_ptr(), ldo, ws.data_ptr(), B, N, heads, dh, ctx.stream)
        ctx.sync()
        got = out.cpu()
        derived(got[:B * N], _linear_attention_ref(qkv, B, N, heads, torch.float64), _linear_attention_ref(qkv, B, N, heads, torch.float32), str((B, N)))
        untouched(got, ldo, B * N)


# ====================================================================================================== 4. RMSNorm
RMS_C = [4, 48, 64, 192, 256, 260, 384, 512, 1024]
RMS_NPIX = [1, 5, 16384, 16385, 3 * 16384 + 7]          # the grid is capped at 4096 blocks of four pixels: one, two and several trips


def _rms_ref(x, g, res, dtype):
    x, g = x.to(dtype), g.to(dtype)
    y = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * g * (x.shape[-1] ** 0.5)
    return y if res is None else y + res.to(dtype)


@pytest.mark.parametrize("C_", RMS_C)
def test_rmsnorm_and_rmsnorm_add_against_float64(ctx, C_):
    """nd_rmsnorm_nhwc_f32 and nd_rmsnorm_add_nhwc_f32 (the closing RMSNorm of a stage's LinearAttention plus the residual; the engine writes a fresh
    buffer, res never aliases out): one and several 256-channel passes of a lane, partial last pass (C = 260), every trip count of the pixel loop, strides
    wider than C on every tensor, an all-zero row (F.normalize's 1e-12 clamp)."""
    import hiputil as hu
    ldx, ldr, ldo = C_ + 4, C_ + 12, C_ + 8
    g = U(f"rms.g.{C_}", (C_,), 0.5, 1.5)
    gd = hu.dev(g)
    for npix in RMS_NPIX:
        B = 1 if npix < 16 else (3 if npix % 3 == 0 else 1)
        x, res = R(300 + C_, (npix, C_), -2, 2), R(301 + C_, (npix, C_))
        x[npix // 2] = 0.0
        xd, rd = _strided(x, ldx), _strided(res, ldr)
        for entry, r in (("nd_rmsnorm_nhwc_f32", None), ("nd_rmsnorm_add_nhwc_f32", res)):
            out = hu.full((npix + 2, ldo))
            if r is None:
                L.call(entry, xd.data_ptr(), ldx, gd.data_ptr(), out.data_ptr(), ldo, B, npix // B, C_, ctx.stream)
            else:
                L.call(entry, xd.data_ptr(), ldx, gd.data_ptr(), rd.data_ptr(), ldr, out.data_ptr(), ldo, B, npix // B, C_, ctx.stream)
            ctx.sync()
            got = out.cpu()
            o1(got[:npix, :C_], _rms_ref(x, g, r, torch.float64), f"{entry} npix {npix}")
            assert torch.equal(got[npix // 2, :C_], torch.zeros(C_) if r is None else res[npix // 2]), "the all-zero row"
            untouched(got, C_, npix, f"{entry} npix {npix}")


def test_rmsnorm_at_the_table_rows(ctx):
    import hiputil as hu
    for entry in ("nd_rmsnorm_nhwc_f32", "nd_rmsnorm_add_nhwc_f32"):
        for row in rows_of(entry):
            B, HW, C_ = row[-3:]
            x, res, g = R(310, (B * HW, C_), -2, 2), R(311, (B * HW, C_)), U(f"rms.g.{C_}", (C_,), 0.5, 1.5)
            xd, rd, gd, out = hu.dev(x), hu.dev(res), hu.dev(g), hu.full((B * HW + 2, C_))
            if entry == "nd_rmsnorm_nhwc_f32":
                assert row[:2] == (C_, C_)
                L.call(entry, xd.data_ptr(), C_, gd.data_ptr(), out.data_ptr(), C_, B, HW, C_, ctx.stream)
            else:
                assert row[:3] == (C_, C_, C_)
                L.call(entry, xd.data_ptr(), C_, gd.data_ptr(), rd.data_ptr(), C_, out.data_ptr(), C_, B, HW, C_, ctx.stream)
            ctx.sync()
            got = out.cpu()
            o1(got[:B * HW], _rms_ref(x, g, None if entry == "nd_rmsnorm_nhwc_f32" else res, torch.float64), f"{entry} {row}")
            untouched(got, C_, B * HW)


# ====================================================================================================== 5. LayerNorm statistics
LN_C = [4, 8, 12, 48, 64, 128, 132, 256, 260, 384, 512, 516, 768, 1024]       # every lpr, the three instances, nj == 3 (516, 768), partial last quads
# (C, B, HW) with B HW above 16384 waves x rows per pass: a second trip of the loop for each instance (NJ = 1 at 64 rows x 4 and 4 x 4 per pass; 2; 3 -> <4>; 4)
LN_BIG = [(4, 3, 1398139), (64, 3, 87492), (260, 3, 10925), (516, 3, 5477), (1024, 1, 16387)]
LN_EPS = 1e-5


def _ln_ref(x, vec, B, dtype):
    """{mean, rstd} of (x + vec[b]) over the channels: the two-pass formula in ``dtype``."""
    v = x.to(dtype).reshape(B, -1, x.shape[-1])
    if vec is not None:
        v = v + vec.to(dtype)[:, None]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return torch.cat((mean, (var + LN_EPS).rsqrt()), -1).reshape(-1, 2)


def _ln_run(ctx, x, vec, B, HW, C_, ldx):
    import hiputil as hu
    xd, vd = _strided(x, ldx), None if vec is None else hu.dev(vec)
    st = hu.full((B * HW + 3, 2))
    L.call("nd_layernorm_stats_f32", xd.data_ptr(), ldx, L.ptr(vd), st.data_ptr(), B, HW, C_, LN_EPS, ctx.stream)
    ctx.sync()
    got = st.cpu()
    untouched(got, 2, B * HW, f"C {C_}")
    return got[:B * HW]


@pytest.mark.parametrize("C_", LN_C)
def test_layernorm_stats_against_float64(ctx, C_):
    """nd_layernorm_stats_f32 with and without the per-sample vector, ldx > C, a pixel count that is no multiple of the rows a wave takes per pass; and a
    row with mean 1e3 and spread 1e-2 (rstd about 150, carried by the cancellation in x - mean), whose bound is the fp32 two-pass formula's own error."""
    B, HW = 3, 37
    x, vec = U(f"ln.x.{C_}", (B * HW, C_), -2, 2), U(f"ln.v.{C_}", (B, C_))
    for v in (None, vec):
        o1(_ln_run(ctx, x, v, B, HW, C_, C_ + 4), _ln_ref(x, v, B, torch.float64), f"vec {v is not None}")
    tight = 1e3 + U(f"ln.t.{C_}", (B * HW, C_), -1e-2, 1e-2)
    got, r64, r32 = _ln_run(ctx, tight, None, B, HW, C_, C_ + 4), _ln_ref(tight, None, B, torch.float64), _ln_ref(tight, None, B, torch.float32)
    derived(got[:, 0], r64[:, 0], r32[:, 0], "tight row, mean")
    derived(got[:, 1], r64[:, 1], r32[:, 1], "tight row, rstd")


@pytest.mark.parametrize("shape", LN_BIG, ids=lambda s: "x".join(map(str, s)))
def test_layernorm_stats_second_trip_of_the_loop(ctx, shape):
    C_, B, HW = shape
    x, vec = R(400 + C_, (B * HW, C_), -2, 2), U(f"ln.bv.{C_}", (B, C_))
    o1(_ln_run(ctx, x, vec, B, HW, C_, C_ + 4), _ln_ref(x, vec, B, torch.float64), str(shape))


def test_layernorm_stats_at_the_table_rows(ctx):
    for ldx, B, HW, C_ in rows_of("nd_layernorm_stats_f32"):
        x, vec = R(410 + C_, (B * HW, C_), -2, 2), U(f"ln.tv.{C_}", (B, C_))
        o1(_ln_run(ctx, x, vec, B, HW, C_, ldx), _ln_ref(x, vec, B, torch.float64), str((B, HW, C_)))


# ====================================================================================================== 6. the ResnetBlock tail
def _asa_ref(t, mad, r0, r1, dtype):
    t, mad = t.to(dtype), mad.to(dtype)
    y = F.silu((t - mad[:, None, 0]) * mad[:, None, 1] + mad[:, None, 2])
    for r in (r0, r1):
        if r is not None:
            y = y + r.to(dtype)
    return y


def _asa_run(ctx, t, mad, r0, r1, ld):
    """ld = (ldt, ldr0, ldr1, ldo); returns the written (B, HW, C) after the canary check."""
    import hiputil as hu
    B, HW, C_ = t.shape
    td, md = _strided(t, ld[0]), hu.dev(mad)
    r0d, r1d = (None if r is None else _strided(r, l) for r, l in ((r0, ld[1]), (r1, ld[2])))
    out = hu.full((B * HW + 2, ld[3]))
    L.call("nd_affine_silu_add_f32", td.data_ptr(), ld[0], md.data_ptr(), L.ptr(r0d), ld[1], L.ptr(r1d), ld[2], out.data_ptr(), ld[3], B, HW, C_, ctx.stream)
    ctx.sync()
    got = out.cpu()
    untouched(got, C_, B * HW)
    return got[:B * HW, :C_].reshape(B, HW, C_)


def _asa_inputs(seed, B, HW, C_):
    return (R(seed, (B, HW, C_), -2, 2), torch.stack((R(seed + 1, (B, C_)), R(seed + 2, (B, C_), 0.5, 1.5), R(seed + 3, (B, C_))), 1).contiguous(),
            R(seed + 4, (B, HW, C_)), R(seed + 5, (B, HW, C_)))


@pytest.mark.parametrize("shape", [(3, 100, 48), (2, 333, 260), (5, 256 * 256, 64)], ids=lambda s: "x".join(map(str, s)))
def test_affine_silu_add_against_float64(ctx, shape):
    """nd_affine_silu_add_f32 with the four null / non-null combinations of res0 and res1 and strides wider than C; (5, 65536, 64) is 1.25 trips of the grid
    capped at 16384 blocks (4.19 M quads).  The engine writes a fresh buffer (Plan.resnet): out aliases neither residual."""
    B, HW, C_ = shape
    t, mad, r0, r1 = _asa_inputs(500, B, HW, C_)
    for a, b in ((None, None), (r0, None), (None, r1), (r0, r1)):
        o1(_asa_run(ctx, t, mad, a, b, (C_ + 4, C_ + 8, C_ + 12, C_ + 16)), _asa_ref(t, mad, a, b, torch.float64), f"res0 {a is not None} res1 {b is not None}")


def test_affine_silu_add_at_the_headline_rows(ctx):
    """Every launch of the headline configuration in INFER_SHAPES, both residuals present (shot_time's tail carries shot_emb + r)."""
    for row in sorted(k[1] for k, cfgs in INFER_SHAPES.items() if k[0] == "nd_affine_silu_add_f32" and "headline" in cfgs):
        ldt, ldr0, ldr1, ldo, B, HW, C_ = row
        t, mad, r0, r1 = _asa_inputs(510, B, HW, C_)
        o1(_asa_run(ctx, t, mad, r0, r1, (ldt, ldr0, ldr1, ldo)), _asa_ref(t, mad, r0, r1, torch.float64), str(row))


# ====================================================================================================== 7. GroupNorm finalize
GN_EPS = 1e-5


def _mad_ref(raw, gamma, beta, ss, G, dtype):
    """[B][3][C] M, A, D of Block.forward's GroupNorm -> x (scale + 1) + shift from the raw tensor (B, P, C): biased variance, eps inside the root."""
    B, P, C_ = raw.shape
    x = raw.to(dtype).reshape(B, P, G, C_ // G)
    mean = x.mean((1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean((1, 3))
    mean, rstd = (v.repeat_interleave(C_ // G, 1) for v in (mean, (var + GN_EPS).rsqrt()))
    sc = ss[:, :C_].to(dtype) if ss is not None else torch.zeros(B, C_, dtype=dtype)
    sh = ss[:, C_:2 * C_].to(dtype) if ss is not None else torch.zeros(B, C_, dtype=dtype)
    return torch.stack((mean, rstd * gamma.to(dtype) * (sc + 1), beta.to(dtype) * (sc + 1) + sh), 1)


def _finalize(ctx, st, sc, slots, gamma, beta, ss, ld_ss, B, C_, G):
    import hiputil as hu
    mad = hu.full((B * 3 + 1, C_))
    ssd, gd, bd = None if ss is None else _strided(ss, ld_ss), hu.dev(gamma), hu.dev(beta)
    L.call("nd_groupnorm_finalize_f32", st.data_ptr(), sc.data_ptr(), slots, gd.data_ptr(), bd.data_ptr(), L.ptr(ssd), ld_ss,
           mad.data_ptr(), B, C_, G, GN_EPS, ctx.stream)
    ctx.sync()
    got = mad.cpu()
    untouched(got, C_, B * 3)
    return got[:B * 3].reshape(B, 3, C_)


@pytest.mark.parametrize("C_,G", [(48, 8), (64, 8), (48, 2), (256, 2)])
@pytest.mark.parametrize("spread", ["wide", "small_variance"])
def test_groupnorm_finalize_against_float64_statistics_of_the_raw_tensor(ctx, C_, G, spread):
    """nd_groupnorm_finalize_f32 on the statistics nd_conv3x3_nhwc_f32's epilogue emits (group widths 6, 8, 24, 128), against float64 statistics of the
    convolution's own output; time scale / shift rows of stride ld_ss > 2 C, and without them.  'small_variance': weights of 1e-3 under a bias of
    order 1, so the variance is of the order of eps and A = rstd gamma is about 150: scale max|ref|, bound derived from the fp32 torch statistics."""
    import hiputil as hu
    B, H, W, cin = 2, 24, 40, 8
    wamp = 0.2 if spread == "wide" else 1e-3
    x, w, b = U("gn.x", (B, cin, H, W), -1.5, 1.5), U(f"gn.w.{C_}", (C_, cin, 3, 3), -wamp, wamp), U(f"gn.b.{C_}", (C_,))
    out, st, sc, slots = hu.conv3x3(ctx, hu.src(hu.nhwc(x)), hu.pack_conv3(ctx, w), hu.dev(b), B, H, W, cin, C_, stats=True)
    raw = out.cpu().reshape(B, H * W, C_)
    gamma, beta, ss = U(f"gn.g.{C_}", (C_,), 0.5, 1.5), U(f"gn.be.{C_}", (C_,)), U(f"gn.ss.{C_}", (B, 2 * C_), -0.5, 0.5)
    for s in (ss, None):
        got = _finalize(ctx, st, sc, slots, gamma, beta, s, 2 * C_ + 12, B, C_, G)
        r64, r32 = _mad_ref(raw, gamma, beta, s, G, torch.float64), _mad_ref(raw, gamma, beta, s, G, torch.float32)
        for i, nm in enumerate("MAD"):
            if spread == "wide":
                o1(got[:, i], r64[:, i], nm)
            else:
                derived(got[:, i], r64[:, i], r32[:, i], f"{nm}, scale_shift {s is not None}")


def test_groupnorm_finalize_skips_zero_count_slots(ctx):
    """A hand-built statistics buffer: the pixels of a raw tensor cut into slots of uneven size, {sum, centred M2} per (slot, channel), with zero-count slots
    holding NaN interleaved; the result is the float64 statistics of the whole tensor."""
    import hiputil as hu
    B, C_, G = 2, 48, 8
    counts = [0, 7, 0, 0, 33, 1, 0, 64, 15, 0]
    P = sum(counts)
    raw = U("gn.hand", (B, P, C_), -1.5, 1.5) + 2.0 * U("gn.hand.m", (B, 1, C_))
    st = torch.full((B, len(counts), C_, 2), float("nan"))
    at = 0
    for s, n in enumerate(counts):
        if n:
            seg = raw[:, at:at + n].double()
            st[:, s, :, 0], st[:, s, :, 1] = seg.sum(1).float(), ((seg - seg.mean(1, keepdim=True)) ** 2).sum(1).float()
            at += n
    gamma, beta = U("gn.hand.g", (C_,), 0.5, 1.5), U("gn.hand.b", (C_,))
    got = _finalize(ctx, hu.dev(st), hu.dev(torch.tensor(counts, dtype=torch.float32)), len(counts), gamma, beta, None, 0, B, C_, G)
    o1(got, _mad_ref(raw, gamma, beta, None, G, torch.float64))


def test_groupnorm_finalize_at_the_table_rows(ctx):
    """(slots, ld_ss, B, C, groups) of every launch, on hand-built statistics of a random raw tensor with one pixel block per slot."""
    import hiputil as hu
    for slots, ld_ss, B, C_, G in rows_of("nd_groupnorm_finalize_f32"):
        n = 8
        raw = R(600 + C_, (B, slots * n, C_), -1.5, 1.5) + 2.0 * R(601 + C_, (B, 1, C_))
        seg = raw.double().reshape(B, slots, n, C_)
        st = torch.stack((seg.sum(2), ((seg - seg.mean(2, keepdim=True)) ** 2).sum(2)), -1).float()
        gamma, beta, ss = R(602, (C_,), 0.5, 1.5), R(603, (C_,)), R(604, (B, ld_ss), -0.5, 0.5)
        got = _finalize(ctx, hu.dev(st), hu.dev(torch.full((slots,), float(n))), slots, gamma, beta, ss, ld_ss, B, C_, G)
        o1(got, _mad_ref(raw, gamma, beta, ss, G, torch.float64), str((slots, B, C_, G)))


# ====================================================================================================== 8. dense rows
ACT_PAIRS = [(L.ACT_NONE, L.ACT_NONE), (L.ACT_NONE, L.ACT_GELU), (L.ACT_NONE, L.ACT_SILU)]      # every (act_in, act_out) Plan.linear_rows is called with


def _act(v, a):
    return F.gelu(v) if a == L.ACT_GELU else F.silu(v) if a == L.ACT_SILU else v


def _linear_rows(ctx, x, w, b, ld_in, ld_out, act):
    import hiputil as hu
    (B, K), N = x.shape, w.shape[0]
    xd, wd, bd, out = _strided(x, ld_in), hu.dev(w), None if b is None else hu.dev(b), hu.full((B + 1, ld_out))
    L.call("nd_linear_rows_f32", xd.data_ptr(), ld_in, wd.data_ptr(), L.ptr(bd), out.data_ptr(), ld_out, B, K, N, act[0], act[1], ctx.stream)
    ctx.sync()
    got = out.cpu()
    untouched(got, N, B)
    o1(got[:B, :N], _act(F.linear(_act(x.double(), act[0]), w.double(), None if b is None else b.double()), act[1]), str((B, K, N, act)))


@pytest.mark.parametrize("K", [1, 3, 256, 2048])
@pytest.mark.parametrize("N", [1, 333, 2048])
def test_linear_rows_against_float64(ctx, K, N):
    for B in (1, 16, 64):
        x, w, b = U(f"lr.x.{K}.{B}", (B, K), -2, 2), U(f"lr.w.{K}.{N}", (N, K), -1, 1) * K ** -0.5, U(f"lr.b.{N}", (N,))
        for act in ACT_PAIRS:
            _linear_rows(ctx, x, w, b, K + 5, N + 3, act)
        _linear_rows(ctx, x, w, None, K, N, ACT_PAIRS[0])


def test_linear_rows_at_the_table_rows(ctx):
    for ld_in, ld_out, B, K, N, a_in, a_out in rows_of("nd_linear_rows_f32"):
        assert (a_in, a_out) in ACT_PAIRS
        x, w, b = R(700 + K, (B, K), -2, 2), R(701 + N, (N, K)) * K ** -0.5, R(702 + N, (N,))
        _linear_rows(ctx, x, w, b, ld_in, ld_out, (a_in, a_out))


# ====================================================================================================== 9. the time conditioning
COND_T = [0, 1, 499, 998, 999, 499, 999, 0]


def _freqs(dim):
    half = dim // 2
    return torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).to(torch.float32)


def _emb64(t, dim):
    """SinusoidalPosEmb in float64 of the reference's own angle: the product int64 x fp32 -> fp32 (Diffusion_arch.py:105) is part of the function."""
    ang = (t[:, None].float() * _freqs(dim)[None]).double()
    return torch.cat((ang.sin(), ang.cos()), -1)


def _cond_shapes():
    """(dim, B, J) of every conditioning launch in INFER_SHAPES (whichever of the three forms the plan records)."""
    out = set()
    for (entry, ints) in INFER_SHAPES:
        if entry.startswith("nd_cond_step"):
            out.add((ints[2], ints[1], ints[3]))            # (ld_out, B, dim, J, ...)
    return sorted(out)


@pytest.mark.parametrize("shape", _cond_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_cond_step_forms_against_float64_and_each_other(ctx, shape):
    """nd_cond_step_f32, nd_cond_table_build_f32 + nd_cond_step_table_f32 and nd_cond_step_ptable_f32 at (dim, B, J) of the plans, the timesteps 0, 1, 499,
    998, 999 with repeats: each against float64, and the same bits from all three (DESIGN: the table forms are the same arithmetic)."""
    import hiputil as hu
    dim, B, J = shape
    t = torch.tensor([COND_T[i % len(COND_T)] for i in range(B)], dtype=torch.long)
    W1, b1 = U(f"cs.W1.{dim}", (4 * dim, dim), -0.2, 0.2), U(f"cs.b1.{dim}", (4 * dim,))
    W2, b2 = U(f"cs.W2.{dim}", (4 * dim, 4 * dim), -0.1, 0.1), U(f"cs.b2.{dim}", (4 * dim,))
    Wp, bp = R(800 + dim, (J, 4 * dim), -0.1, 0.1), R(801 + dim, (J,))
    W1d, b1d, W2d, b2d, Wpd, bpd = (w.double() for w in (W1, b1, W2, b2, Wp, bp))
    head = lambda tt: F.silu(F.linear(F.gelu(F.linear(_emb64(tt, dim), W1d, b1d)), W2d, b2d))
    ref = F.linear(head(t), Wpd, bpd)
    td, fd = hu.dev(t), hu.dev(_freqs(dim))
    dev = [hu.dev(v) for v in (W1, b1, W2, b2, Wp, bp)]
    common = [fd.data_ptr()] + [v.data_ptr() for v in dev]
    rows, ld = 1000, J + 4
    table = hu.full((rows + 1, 4 * dim))
    L.call("nd_cond_table_build_f32", *common[:5], table.data_ptr(), rows, dim, ctx.stream)
    ctx.sync()
    tab = table.cpu()
    o1(tab[:rows], head(torch.arange(rows)), "table")
    untouched(tab, 4 * dim, rows)
    outs = {}
    ptable = None
    if J % 4 == 0:
        ptable, ts = hu.full((rows, J)), hu.dev(torch.arange(rows, dtype=torch.int64))
        for t0 in range(0, rows, 16):
            nb = min(16, rows - t0)
            L.call("nd_cond_step_table_f32", ts.data_ptr() + 8 * t0, *common, ptable.data_ptr() + 4 * t0 * J, J, nb, dim, J, table.data_ptr(), rows, ctx.stream)
        ctx.sync()
    for form in ("plain", "table", "ptable"):
        out = hu.full((B + 1, ld))
        if form == "plain":
            L.call("nd_cond_step_f32", td.data_ptr(), *common, out.data_ptr(), ld, B, dim, J, ctx.stream)
        elif form == "table":
            L.call("nd_cond_step_table_f32", td.data_ptr(), *common, out.data_ptr(), ld, B, dim, J, table.data_ptr(), rows, ctx.stream)
        elif ptable is not None:
            L.call("nd_cond_step_ptable_f32", td.data_ptr(), *common, out.data_ptr(), ld, B, dim, J, table.data_ptr(), rows, ptable.data_ptr(), ctx.stream)
        else:
            continue
        ctx.sync()
        got = out.cpu()
        o1(got[:B, :J], ref, form)
        untouched(got, J, B, form)
        outs[form] = got[:B, :J]
    assert torch.equal(outs["plain"], outs["table"]) and ("ptable" not in outs or torch.equal(outs["plain"], outs["ptable"]))


def test_time_embedding_iso_embedding_and_position_encoding_at_the_table_shapes(ctx):
    """nd_sinusoidal_time_emb_f32 at (B, dim / 2) of every configuration (the plans launch it only where the one-launch conditioning does not fit),
    nd_embedding_rows_f32 and nd_pos_enc_f32 at their INFER_SHAPES rows."""
    import hiputil as hu
    for dim, B in sorted({(d, b) for d, _, b, _ in CONFIGS.values()}):
        t = torch.tensor([COND_T[i % len(COND_T)] for i in range(B)], dtype=torch.long)
        emb, td, fd = hu.full((B + 1, dim)), hu.dev(t), hu.dev(_freqs(dim))
        L.call("nd_sinusoidal_time_emb_f32", td.data_ptr(), fd.data_ptr(), emb.data_ptr(), B, dim // 2, ctx.stream)
        ctx.sync()
        o1(emb.cpu()[:B], _emb64(t, dim), f"time emb {dim} {B}")
        untouched(emb.cpu(), dim, B)
    for B, rows, dim in rows_of("nd_embedding_rows_f32"):
        table, idx = U("em.t", (rows, dim)), torch.tensor([rows - 1, 0] + [(37 * i) % rows for i in range(B - 2)])
        out, idd, tabd = hu.full((B + 1, dim)), hu.dev(idx), hu.dev(table)
        L.call("nd_embedding_rows_f32", idd.data_ptr(), tabd.data_ptr(), out.data_ptr(), B, rows, dim, ctx.stream)
        ctx.sync()
        assert torch.equal(out.cpu()[:B], table[idx])
        untouched(out.cpu(), dim, B)
    for B, H, W, hid in rows_of("nd_pos_enc_f32"):
        pos, w, b = R(900, (B, 2, H, W)), U("pe.w", (hid, 2)), U("pe.b", (hid,))
        out, pd, wd, bd = hu.full((B * H * W + 1, 3 * hid)), hu.dev(pos), hu.dev(w), hu.dev(b)
        L.call("nd_pos_enc_f32", pd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W, hid, ctx.stream)
        ctx.sync()
        v = torch.einsum("bchw,kc->bhwk", pos.double(), w.double()) + b.double()
        got = out.cpu()
        o1(got[:B * H * W].reshape(B, H, W, 3 * hid), torch.cat((v, (2 * math.pi * v).sin(), (2 * math.pi * v).cos()), -1), f"pos_enc {B} {H} {W}")
        untouched(got, 3 * hid, B * H * W)


# ====================================================================================================== 10. layout and pooling
LAYOUT_SHAPES = sorted({(b, 4, s, s) for _, s, b, _ in CONFIGS.values()}) + [(3, 4, 7, 13), (2, 3, 9, 5), (1, 1, 1, 1)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_kernels_are_exact(ctx, shape):
    """nd_nchw_to_nhwc_f32, nd_nhwc_to_nchw_f32 (set_condition / load_x / read_nchw run them at (B, 4, H, W) of the plan) and nd_nchw_to_nhwc_pad_f32
    with Cpad in {C, 8}: the same values, zero pad lanes, nothing written behind the tensor."""
    import hiputil as hu
    B, C_, H, W = shape
    x = R(1000, shape, -3, 3)
    n = x.numel()
    xd, a, b = hu.dev(x), hu.full((n + 5,)), hu.full((n + 5,))
    L.call("nd_nchw_to_nhwc_f32", xd.data_ptr(), a.data_ptr(), B, C_, H, W, ctx.stream)
    L.call("nd_nhwc_to_nchw_f32", a.data_ptr(), b.data_ptr(), B, C_, H, W, ctx.stream)
    ctx.sync()
    ac, bc = a.cpu(), b.cpu()
    assert torch.equal(ac[:n].reshape(B, H, W, C_), x.permute(0, 2, 3, 1)) and torch.equal(bc[:n].reshape(shape), x)
    assert bool(torch.isnan(ac[n:]).all()) and bool(torch.isnan(bc[n:]).all())
    for cpad in (C_, 8):
        p = hu.full((B * H * W * cpad + 5,))
        L.call("nd_nchw_to_nhwc_pad_f32", xd.data_ptr(), p.data_ptr(), B, C_, H, W, cpad, ctx.stream)
        ctx.sync()
        pc = p.cpu()
        got = pc[:B * H * W * cpad].reshape(B, H, W, cpad)
        assert torch.equal(got[..., :C_], x.permute(0, 2, 3, 1)) and bool((got[..., C_:] == 0).all()) and bool(torch.isnan(pc[B * H * W * cpad:]).all())


@pytest.mark.parametrize("shape", [(2, 13, 9, 32), (1, 1, 1, 4), (3, 8, 16, 64), (1, 257, 255, 32), (2, 5, 6, 512)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool2x2_is_exact(ctx, shape):
    """nn.MaxPool2d(2, 2, ceil_mode=True) on NHWC at odd and even sizes (LSID's stages): windows over the border take the in-bounds values; -0.0 and equal
    neighbours give the window's value."""
    import hiputil as hu
    B, H, W, C_ = shape
    x = (R(1100, shape, -3, 3) * 4).round() / 4                     # a coarse grid: many equal neighbours
    x[x == 0] = -0.0
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out, xd = hu.full((B * Ho * Wo * C_ + 4,)), hu.dev(x)
    L.call("nd_maxpool2x2_nhwc_f32", xd.data_ptr(), out.data_ptr(), B, H, W, C_, ctx.stream)
    ctx.sync()
    ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    got = out.cpu()
    assert torch.equal(got[:B * Ho * Wo * C_].reshape(B, Ho, Wo, C_).double(), ref) and bool(torch.isnan(got[B * Ho * Wo * C_:]).all())


# ====================================================================================================== 11. the sampler update
class _Net(torch.nn.Module):
    channels = out_dim = 4
    self_condition = False
    random_or_learned_sinusoidal_cond = False


SCHEDULES = {                                  # name -> GaussianDiffusion keywords
    "ddpm1000": dict(timesteps=1000, beta_schedule="sigmoid2"),
    "ddim50_eta0": dict(timesteps=1000, sampling_timesteps=50, ddim_sampling_eta=0.0, beta_schedule="sigmoid2"),
    "ddim50_eta05": dict(timesteps=1000, sampling_timesteps=50, ddim_sampling_eta=0.5, beta_schedule="sigmoid2"),
    "ddim8_eta1": dict(timesteps=1000, sampling_timesteps=8, ddim_sampling_eta=1.0, beta_schedule="sigmoid2"),
    "ddpm_linear": dict(timesteps=1000, beta_schedule="linear"),
    "ddim50_cosine": dict(timesteps=1000, sampling_timesteps=50, ddim_sampling_eta=0.5, beta_schedule="cosine"),
}
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def _gd(name, objective="pred_v"):
    from noisediff_amd import GaussianDiffusion
    return GaussianDiffusion(_Net(), image_size=32, objective=objective, **SCHEDULES[name])


def _step_ref(x, o, z, cf, obj, ddim, dtype):
    """The update of sampler.hip's header comment, from the fp32 coefficient row ``cf``, in ``dtype`` and in the kernel's written operation order."""
    x, o, z = x.to(dtype), o.to(dtype), z.to(dtype)
    c0, c1, c2, c3, c4, c5, c6, c7 = (v.to(dtype) for v in cf)
    x0 = c0 * x - c1 * o if obj == 2 else c2 * x - c3 * o if obj == 0 else o
    x0 = x0.clamp(-1.0, 1.0)
    if ddim:
        if float(c7) != 0.0:
            return x0
        eps = (c2 * x - x0) / c3
        return x0 * c4 + c5 * eps + (c6 * z if float(c6) != 0.0 else 0.0)
    return (c4 * x0 + c5 * x) + (c6 * z if float(c7) != 0.0 else 0.0)


class _Sampler:
    """The device-resident loop state of one GaussianDiffusion, as diffusion._Loop builds it."""

    def __init__(self, gd, B, rng=None):
        import hiputil as hu
        self.t_cur, self.t_next, self.coef = gd._tables()
        self.ddim, self.n = gd.is_ddim_sampling, int(self.t_cur.numel())
        self.d = [hu.dev(self.t_cur), hu.dev(self.t_next), hu.dev(self.coef)]
        self.step, self.time = hu.dev(torch.zeros(1, dtype=torch.int32)), hu.dev(torch.full((B + 2,), -7, dtype=torch.int64))
        self.rng = None if rng is None else hu.dev(torch.tensor(rng, dtype=torch.int64))
        st = L.SamplerState()
        st.step, st.t_cur, st.t_next, st.coef = self.step.data_ptr(), self.d[0].data_ptr(), self.d[1].data_ptr(), self.d[2].data_ptr()
        st.time_out, st.rng, st.n_steps, st.B = self.time.data_ptr(), L.ptr(self.rng), self.n, B
        self.state = st
        self.entry = "nd_sampler_step_ddim_f32" if self.ddim else "nd_sampler_step_ddpm_f32"

    def set_step(self, i):
        self.step.fill_(i)
        torch.cuda.synchronize()

    def update(self, ctx, x, o, noise, stride, obj, seed=0, first=0):
        """x (B, HW, C) on the CPU -> the updated tensor (the kernel works in place on a device copy followed by a NaN canary)."""
        import hiputil as hu
        B, HW, C_ = x.shape
        buf = hu.full((x.numel() + 8,))
        buf[:x.numel()] = x.reshape(-1).to(hu.DEV)
        torch.cuda.synchronize()
        od = hu.dev(o)
        L.call(self.entry, buf.data_ptr(), od.data_ptr(), L.ptr(noise), stride, C.byref(self.state), obj, C.c_uint64(seed), first, B, HW, C_, ctx.stream)
        ctx.sync()
        got = buf.cpu()
        assert bool(torch.isnan(got[x.numel():]).all()), "wrote behind x"
        return got[:x.numel()].reshape(x.shape)


def _steps_of(n):
    return sorted({0, 1, n // 2, n - 2, n - 1})


def _oracle_noise(seed, first, B, per_q, draw, quads=None):
    """(B, quads, 4) float64 normals of the device stream: Philox4x32-10 keyed by seed, counter {quad, first + b, draw, 0}."""
    q = np.arange(per_q, dtype=np.uint32) if quads is None else np.asarray(quads, dtype=np.uint32)
    key = np.tile(np.array([[seed & 0xFFFFFFFF, seed >> 32]], dtype=np.uint32), (q.size, 1))
    out = []
    for b in range(B):
        ctr = np.stack([q, np.full(q.size, first + b, np.uint32), np.full(q.size, draw, np.uint32), np.zeros(q.size, np.uint32)], -1)
        out.append(O.philox_normal4(O.philox4x32_10(ctr, key)))
    return np.stack(out)


@pytest.mark.parametrize("objective", sorted(OBJ))
@pytest.mark.parametrize("sched", sorted(SCHEDULES))
def test_sampler_step_against_float64(ctx, sched, objective):
    """nd_sampler_step_ddpm_f32 / _ddim_f32 in place on x, inputs in U(-3, 3) (the clamp of x_0 is active on a good share), at the first two, the middle
    and the last two steps, noise supplied through ``noise`` + ``noise_step_stride``.  The bound is derived from the fp32 torch evaluation of the same
    formula (the DDIM update divides by sqrt_recipm1_alphas_cumprod, about 4e-3 at the last steps, which amplifies rounding: the fp32 reference itself
    is 6.8e-5 off float64 for pred_noise at step 0 of the 8-step schedule, the kernel 2.6e-5).  A DDIM step with sigma = 0 draws nothing: NaN in its noise slice does not reach x."""
    import hiputil as hu
    B, HW, C_ = 3, 1024, 4
    s = _Sampler(_gd(sched, objective), B)
    x, o = U("ss.x", (B, HW, C_), -3, 3), U("ss.o", (B, HW, C_), -3, 3)
    stride = x.numel() + 16
    steps = _steps_of(s.n)
    z = {i: synth.normal(31, f"ss.z.{i}", (B, HW, C_)) for i in steps}
    noise = torch.full((s.n * stride,), float("nan"))
    for i in steps:
        cf = s.coef[i]
        draws = (float(cf[7]) == 0.0 and float(cf[6]) != 0.0) if s.ddim else float(cf[7]) != 0.0
        if draws:
            noise[i * stride:i * stride + x.numel()] = z[i].reshape(-1)
    nd = hu.dev(noise)
    for i in steps:
        s.set_step(i)
        got = s.update(ctx, x, o, nd, stride, OBJ[objective])
        zi = torch.nan_to_num(noise[i * stride:i * stride + x.numel()].reshape(x.shape), nan=0.0)
        derived(got, _step_ref(x, o, zi, s.coef[i], OBJ[objective], s.ddim, torch.float64), _step_ref(x, o, zi, s.coef[i], OBJ[objective], s.ddim, torch.float32),
                f"step {i}")
    assert float(((x * s.coef[steps[2]][0] - o * s.coef[steps[2]][1]).abs() > 1).float().mean()) > 0.1       # the clamp was at work (pred_v's x_0)


@pytest.mark.parametrize("sched", ["ddpm1000", "ddim50_eta05"])
def test_sampler_step_noise_from_the_device_stream(ctx, sched):
    """noise = NULL: the draw of step i is Philox draw i + 1 of sample first_sample + b.  Against the float64 formula on the oracle's normals (the bound
    adds c6 x the Philox comparison's own tolerance, 2e-5 + 1e-4 |z|: the device forms its uniforms in fp32); the same bits as the update fed with
    nd_philox_normal_f32(step = i); the device rng pair overrides the seed / first_sample arguments; a shard starting one sample later computes the same rows."""
    import hiputil as hu
    B, HW, C_, seed, first = 3, 512, 4, 0x1234567890ABCDEF, 5
    gd = _gd(sched)
    s = _Sampler(gd, B)
    x, o = U("sn.x", (B, HW, C_), -3, 3), U("sn.o", (B, HW, C_), -3, 3)
    for i in (0, 1, s.n // 2, s.n - 2):
        s.set_step(i)
        got = s.update(ctx, x, o, None, 0, 2, seed, first)
        z = torch.from_numpy(_oracle_noise(seed, first, B, HW * C_ // 4, i + 1)).reshape(B, HW, C_)
        r64 = _step_ref(x, o, z, s.coef[i], 2, s.ddim, torch.float64)
        c6 = float(s.coef[i][6])
        assert c6 > 0
        e_ref = float((_step_ref(x, o, z.float(), s.coef[i], 2, s.ddim, torch.float32).double() - r64).abs().max())
        excess = float(((got.double() - r64).abs() - c6 * (2e-5 + 1e-4 * z.abs())).max())
        _log(f"step {i}: fp32 reference error {e_ref:.3e}, kernel error beyond the noise tolerance {excess:.3e}")
        assert bool(torch.isfinite(got).all()) and excess <= 4 * e_ref + ULP * float(r64.abs().max())
        zd = hu.full((B, HW, C_))
        L.call("nd_philox_normal_f32", zd.data_ptr(), C.c_uint64(seed), first, i, B, HW, C_, ctx.stream)
        ctx.sync()
        assert torch.equal(got, s.update(ctx, x, o, zd, 0, 2)), "generated noise != the same draw supplied"
        s2 = _Sampler(gd, B, rng=(seed, first))
        s2.set_step(i)
        assert torch.equal(got, s2.update(ctx, x, o, None, 0, 2, 99, 1234)), "the device rng pair does not override the arguments"
        s3 = _Sampler(gd, 2)
        s3.set_step(i)
        assert torch.equal(got[1:], s3.update(ctx, x[1:].contiguous(), o[1:].contiguous(), None, 0, 2, seed, first + 1)), "shard invariance"


@pytest.mark.parametrize("sched", ["ddpm1000", "ddim50_eta05"])
def test_sampler_step_second_trip_and_the_table_shapes(ctx, sched):
    """The grid is capped at 2048 blocks (524288 quads): B = 10 of the headline's 65536 x 4 samples is 1.25 trips; then SAMPLER_SHAPES' headline itself."""
    s = None
    for B, HW, C_ in ((10, 65536, 4), SAMPLER_SHAPES["headline"]):
        s = _Sampler(_gd(sched), B)
        x, o, z = R(1200, (B, HW, C_), -3, 3), R(1201, (B, HW, C_), -3, 3), R(1202, (B, HW, C_), -2, 2)
        import hiputil as hu
        i = s.n // 2
        s.set_step(i)
        got = s.update(ctx, x, o, hu.dev(z), 0, 2)            # stride 0: every step reads the same slice
        derived(got, _step_ref(x, o, z, s.coef[i], 2, s.ddim, torch.float64), _step_ref(x, o, z, s.coef[i], 2, s.ddim, torch.float32), str((B, HW, C_)))


@pytest.mark.parametrize("sched", ["ddpm1000", "ddim8_eta1"])
def test_sampler_loop_state(ctx, sched):
    """nd_sampler_begin_step writes t_cur[step] to the B entries of time_out (0 once past the end) and nothing behind them; nd_sampler_advance adds one per
    call; a step kernel launched with *step >= n_steps leaves x untouched, bit for bit."""
    B = 5
    s = _Sampler(_gd(sched), B)
    for i in (0, 1, s.n - 1):
        s.set_step(i)
        L.call("nd_sampler_begin_step", C.byref(s.state), ctx.stream)
        ctx.sync()
        t = s.time.cpu()
        assert t[:B].tolist() == [int(s.t_cur[i])] * B and t[B:].tolist() == [-7, -7], (i, t)
    s.set_step(s.n - 2)
    for want in (s.n - 1, s.n, s.n + 1):
        L.call("nd_sampler_advance", C.byref(s.state), ctx.stream)
        ctx.sync()
        assert int(s.step.cpu()) == want
    L.call("nd_sampler_begin_step", C.byref(s.state), ctx.stream)
    ctx.sync()
    assert s.time.cpu()[:B].tolist() == [0] * B
    x, o = U("sl.x", (B, 64, 4), -3, 3), U("sl.o", (B, 64, 4), -3, 3)
    for step in (s.n, s.n + 1):
        s.set_step(step)
        assert torch.equal(s.update(ctx, x, o, None, 0, 2, 1, 0), x)


def test_philox_normal_above_one_trip_of_the_grid(ctx):
    """nd_philox_normal_f32 at 3 x 200000 quads (1.14 trips of the 524288-quad grid) and step = -1 (draw 0, x_T) against the oracle on more than 4096 quads per
    sample: a stride of 47, the first and last quad of every sample and both sides of the 524288 boundary.  Tolerance of the small-shape Philox test."""
    import hiputil as hu
    B, HW, C_, seed, first = 3, 200000, 4, 0xFEDCBA9876543210, 11
    per_q = HW * C_ // 4
    out = hu.full((B * HW * C_ + 4,))
    L.call("nd_philox_normal_f32", out.data_ptr(), C.c_uint64(seed), first, -1, B, HW, C_, ctx.stream)
    ctx.sync()
    got = out.cpu()
    assert bool(torch.isnan(got[B * HW * C_:]).all()) and bool(torch.isfinite(got[:B * HW * C_]).all())
    got = got[:B * HW * C_].reshape(B, per_q, 4).numpy()
    edge = [524287 - 2 * per_q, 524288 - 2 * per_q]                    # global quads 524287 / 524288 lie in sample 2
    quads = np.unique(np.concatenate([np.arange(0, per_q, 47), [0, per_q - 1], edge]))
    assert quads.size >= 4096 and 0 <= edge[0] < per_q - 1
    ref = _oracle_noise(seed, first, B, per_q, 0, quads)
    np.testing.assert_allclose(got[:, quads], ref, atol=2e-5, rtol=1e-4)
    _log(f"philox: max |device - oracle| {np.abs(got[:, quads] - ref).max():.3e} on {quads.size} quads per sample")


# ====================================================================================================== 12. ConvTranspose2d's data gradient
@pytest.mark.parametrize("size", [(72, 72), (40, 52)], ids=lambda s: "x".join(map(str, s)))
def test_pointwise_unshuffle_crop_against_float64(ctx, size):
    """nd_pointwise_gemm_unshuffle_crop_nhwc_f32 as lsid_train.convt2x2_dgrad launches it, for up6 .. up9 of an LSID on a (B, 4, H, W) frame: d_up is the
    first c channels of the (B, up_h, up_w, 2 c) concat gradient; ceil-mode pooling makes (up_h, up_w) equal to twice the output at some stages and one
    row / column short of it at others ((72, 72): 9 of 10; (40, 52): 5 of 6 and 13 of 14).  Against float64 F.pixel_unshuffle of the zero-filled source ->
    1x1 with the ConvTranspose weight (cin, c, 2, 2) read as (cin, 4 c)."""
    import hiputil as hu
    from noisediff_amd.lsid import LSID_STAGES, _sizes
    B, sizes = 2, _sizes(*size)
    cropped = set()
    for j, c in zip(range(6, 10), reversed(LSID_STAGES[:-1])):
        i = 10 - j
        (up_h, up_w), (h, w_), cin = sizes[i - 1], sizes[i], 2 * c
        cropped.add((up_h < 2 * h, up_w < 2 * w_))
        wt = U(f"uc.w.{j}", (cin, c, 2, 2)) * (4 * c) ** -0.5
        dcat = U(f"uc.d.{j}.{size}", (B, up_h, up_w, 2 * c), -2, 2)
        dd = hu.dev(dcat)
        s = hu.src(dd, c=4 * c, ld=2 * c, unshuffle=1)
        wp = hu.pack_pw(ctx, wt.reshape(cin, 4 * c).contiguous(), unshuffle_c=c)
        out = hu.full((B * h * w_ + 2, cin + 4))
        d = L.Pointwise()
        d.src, d.weight, d.out = s, wp.data_ptr(), out.data_ptr()
        d.B, d.HW, d.W, d.cin, d.cout, d.ldo = B, h * w_, w_, 4 * c, cin, cin + 4
        L.call("nd_pointwise_gemm_unshuffle_crop_nhwc_f32", C.byref(d), up_h, up_w, ctx.stream)
        ctx.sync()
        src = F.pad(dcat[..., :c].double().permute(0, 3, 1, 2), (0, 2 * w_ - up_w, 0, 2 * h - up_h))
        ref = F.conv2d(F.pixel_unshuffle(src, 2), wt.double().reshape(cin, 4 * c, 1, 1)).permute(0, 2, 3, 1)
        got = out.cpu()
        o1(got[:B * h * w_, :cin].reshape(B, h, w_, cin), ref, f"up{j}")
        untouched(got, cin, B * h * w_, f"up{j}")
    assert len(cropped) > 1, cropped                                 # both: a source equal to and smaller than twice the output


# ====================================================================================================== 13. argument checks
def test_bad_arguments_return_their_error_code_without_a_launch(ctx):
    """Every entry point above: a null pointer (ND_E_BADARG), a pointer 4 bytes off (ND_E_ALIGN), a stride below the channel count, C not a multiple of 4,
    dh != 32 (ND_E_SHAPE); the valid call next to each returns 0.  nd_rmsnorm_nhwc_f32 and nd_affine_silu_add_f32 reject strides below C as
    nd_rmsnorm_add_nhwc_f32 does."""
    import hiputil as hu
    lib, st = ctx.lib, ctx.stream
    BAD, SHAPE, ALIGN = -1, -2, -3
    a, b, c, o = (hu.full((4096,), 0.5) for _ in range(4))
    i64 = hu.dev(torch.zeros(16, dtype=torch.int64))
    pa, pb, pc, po, pi = a.data_ptr(), b.data_ptr(), c.data_ptr(), o.data_ptr(), i64.data_ptr()

    def check(entry, good, bads):
        fn = getattr(lib, entry)
        assert fn(*good, st) == 0, (entry, L.load().nd_last_error())
        for at, value, code in bads:
            args = list(good)
            args[at] = value
            assert fn(*args, st) == code, (entry, at, value, code)
        ctx.sync()

    check("nd_attention_mfma_f32", [pa, 96, po, 32, 1, 4, 1, 32], [(0, None, BAD), (2, None, BAD), (0, pa + 4, ALIGN), (1, 92, SHAPE), (3, 28, SHAPE), (7, 16, SHAPE), (7, 64, SHAPE)])
    check("nd_linear_attention_f32", [pa, 96, po, 32, pc, 1, 4, 1, 32],
          [(0, None, BAD), (2, None, BAD), (4, None, BAD), (0, pa + 4, ALIGN), (1, 92, SHAPE), (3, 28, SHAPE), (8, 16, SHAPE)])
    check("nd_rmsnorm_nhwc_f32", [pa, 8, pb, po, 8, 1, 4, 8], [(0, None, BAD), (2, None, BAD), (3, None, BAD), (0, pa + 4, ALIGN), (3, po + 4, ALIGN), (1, 4, SHAPE), (4, 4, SHAPE), (7, 6, SHAPE)])
    check("nd_rmsnorm_add_nhwc_f32", [pa, 8, pb, pc, 8, po, 8, 1, 4, 8],
          [(0, None, BAD), (3, None, BAD), (5, None, BAD), (3, pc + 4, ALIGN), (1, 4, SHAPE), (4, 4, SHAPE), (6, 4, SHAPE), (9, 6, SHAPE)])
    check("nd_layernorm_stats_f32", [pa, 8, pb, po, 1, 4, 8, 1e-5], [(0, None, BAD), (3, None, BAD), (0, pa + 4, ALIGN), (2, pb + 4, ALIGN), (1, 4, SHAPE), (6, 6, SHAPE), (6, 1028, SHAPE)])
    check("nd_affine_silu_add_f32", [pa, 8, pb, pc, 8, pc, 8, po, 8, 1, 4, 8],
          [(0, None, BAD), (2, None, BAD), (7, None, BAD), (0, pa + 4, ALIGN), (3, pc + 4, ALIGN), (7, po + 4, ALIGN), (1, 4, SHAPE), (4, 4, SHAPE), (6, 4, SHAPE), (8, 4, SHAPE),
           (11, 6, SHAPE)])
    assert lib.nd_affine_silu_add_f32(pa, 8, pb, None, 0, None, 0, po, 8, 1, 4, 8, st) == 0          # the stride of an absent residual is not looked at
    check("nd_groupnorm_finalize_f32", [pa, pb, 4, pc, pc, pc, 16, po, 1, 8, 2, 1e-5], [(0, None, BAD), (1, None, BAD), (3, None, BAD), (7, None, BAD), (6, 12, SHAPE), (10, 3, SHAPE)])
    check("nd_linear_rows_f32", [pa, 8, pb, pc, po, 8, 2, 8, 8, 0, 0], [(0, None, BAD), (2, None, BAD), (4, None, BAD), (1, 4, SHAPE), (5, 4, SHAPE), (7, 2052, SHAPE)])
    w = hu.full((4 * 8 * 4 * 8 + 64,), 0.01)
    pw = w.data_ptr()
    cond = [pi, pa, pw, pb, pw, pb, pw, pb, po, 8, 2, 8, 8]
    cond_bad = [(0, None, BAD), (2, None, BAD), (8, None, BAD), (2, pw + 4, ALIGN), (11, 12, SHAPE), (9, 4, SHAPE)]
    check("nd_cond_step_f32", cond, cond_bad)
    check("nd_cond_table_build_f32", [pa, pw, pb, pw, pb, pc, 4, 8], [(0, None, BAD), (5, None, BAD), (1, pw + 4, ALIGN), (7, 12, SHAPE), (6, 0, SHAPE)])
    check("nd_cond_step_table_f32", cond + [pc, 4], cond_bad + [(13, None, BAD), (14, 0, SHAPE)])
    ptab = hu.full((4 * 8,), 0.25)
    check("nd_cond_step_ptable_f32", cond + [pc, 4, ptab.data_ptr()], cond_bad + [(15, None, BAD), (15, ptab.data_ptr() + 4, ALIGN), (8, po + 4, ALIGN), (12, 6, SHAPE)])
    check("nd_sinusoidal_time_emb_f32", [pi, pa, po, 2, 4], [(0, None, BAD), (1, None, BAD), (2, None, BAD), (4, 0, BAD)])
    check("nd_embedding_rows_f32", [pi, pa, po, 2, 10, 4], [(0, None, BAD), (1, None, BAD), (2, None, BAD), (4, 0, BAD)])
    check("nd_pos_enc_f32", [pa, pb, pc, po, 1, 4, 4, 2], [(0, None, BAD), (1, None, BAD), (2, None, BAD), (3, None, BAD), (7, 0, BAD)])
    for entry in ("nd_nchw_to_nhwc_f32", "nd_nhwc_to_nchw_f32"):
        check(entry, [pa, po, 1, 4, 4, 4], [(0, None, BAD), (1, None, BAD), (3, 0, BAD)])
    check("nd_nchw_to_nhwc_pad_f32", [pa, po, 1, 4, 4, 4, 8], [(0, None, BAD), (1, None, BAD), (6, 3, BAD)])
    check("nd_maxpool2x2_nhwc_f32", [pa, po, 1, 3, 3, 8], [(0, None, BAD), (1, None, BAD), (5, 6, BAD), (0, pa + 4, ALIGN), (1, po + 4, ALIGN)])
    check("nd_philox_normal_f32", [po, C.c_uint64(1), 0, -1, 1, 3, 4], [(0, None, BAD), (0, po + 4, ALIGN), (3, -2, BAD), (6, 3, BAD)])
    # the sampler: state by pointer
    gd = _gd("ddim8_eta1")
    s = _Sampler(gd, 2)
    s.set_step(s.n)                                               # past the end: the valid calls below change nothing
    good = [po, pa, None, 0, C.byref(s.state), 2, C.c_uint64(0), 0, 2, 3, 4]
    bads = [(0, None, BAD), (1, None, BAD), (4, None, BAD), (5, 3, BAD), (0, po + 4, ALIGN), (2, pb + 4, ALIGN), (3, 6, ALIGN), (10, 3, SHAPE)]
    check("nd_sampler_step_ddpm_f32", good, bads)
    check("nd_sampler_step_ddim_f32", good, bads)
    check("nd_sampler_begin_step", [C.byref(s.state)], [(0, None, BAD)])
    for field in ("step", "t_cur", "coef", "time_out"):
        broken = L.SamplerState.from_buffer_copy(s.state)
        setattr(broken, field, None)
        for entry in ("nd_sampler_begin_step", "nd_sampler_advance"):
            assert getattr(lib, entry)(C.byref(broken), st) == BAD, (entry, field)
        assert lib.nd_sampler_step_ddpm_f32(*good[:4], C.byref(broken), *good[5:], st) == BAD, field
    broken = L.SamplerState.from_buffer_copy(s.state)
    broken.t_next = None
    assert lib.nd_sampler_step_ddim_f32(*good[:4], C.byref(broken), *good[5:], st) == BAD
    # the cropped unshuffle: descriptor by pointer
    wp = hu.pack_pw(ctx, U("bad.w", (8, 16)), unshuffle_c=4)
    d = L.Pointwise()
    d.src, d.weight, d.out = hu.src(a, c=16, ld=4, unshuffle=1), wp.data_ptr(), po
    d.B, d.HW, d.W, d.cin, d.cout, d.ldo = 1, 4, 2, 16, 8, 8
    fn = lib.nd_pointwise_gemm_unshuffle_crop_nhwc_f32
    assert fn(C.byref(d), 3, 4, st) == 0, L.load().nd_last_error()
    assert fn(None, 3, 4, st) == BAD and fn(C.byref(d), 0, 4, st) == BAD and fn(C.byref(d), 5, 4, st) == SHAPE and fn(C.byref(d), 3, 5, st) == SHAPE
    d.src.unshuffle = 0
    assert fn(C.byref(d), 3, 4, st) == BAD
    d.src.unshuffle, d.ldo = 1, 4
    assert fn(C.byref(d), 3, 4, st) == SHAPE                        # a stride below cout
    d.ldo, d.weight = 8, None
    assert fn(C.byref(d), 3, 4, st) == BAD
    ctx.sync()
