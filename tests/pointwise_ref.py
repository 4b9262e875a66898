"""References for the 1x1 GEMM and chain kernels (pointwise.hip, pwchain.hip): plain torch on the CPU, in the manner of tests/conv3x3_ref.py.

``operator(inp, dt, gemm)``   the whole nd_pointwise operator in dtype ``dt``: prologue (none, SiLU, LeakyReLU 0.2, GroupNorm-affine + SiLU, LayerNorm(x + vec) with
                              eps 1e-5 and biased variance), the virtual concat, GEMM, bias, activation, then + vec + res0 + res1 + silu((t - M) A + D) -- the order of
                              pw_epilogue's row loop (pointwise.hip: `v = tile + bias`, act, `+= vadd4`, `+= r0`, `+= r1`, `+= nd_silu4((rt - gM) * gA + gD)`).
``chain(inp, dt, gemm)``      two / three stages h = act(W h_prev + bias + res) with CHAIN_RES_INPUT (+ x + v) and CHAIN_RES_INPUT_RAW (+ x), LayerNorm(x + v) or no
                              prologue, and the tail prologue silu(affine(t)) + r0 (+ r1) (pwchain.hip chain_kernel: bias first -- chain_gemm loads it into the accumulator).
``narrow_fold(inp, dt, ...)`` W [p0; p1; silu((t - M) A + D)] + bias (+ res0) on the FOLDED weight (pointwise_narrow_fold_kernel).
``ref64``                     any of them called with torch.float64 and torch's own matmul.

fp32 references -- the same formulas with every product in a legitimate order of the kernel's arithmetic.  Each fp32 multiply-add is ONE rounding (an FMA),
written as fl32(fl64(acc) + fl64(a) * fl64(b)): the product of two fp32 values is exact in fp64.
``gemm32_mfma``    the fp32-MFMA bodies (generic, pipelined, large-tile kernels and the fp32 chain): one sequential chain per output over v_mfma_f32_32x32x2_f32
                   steps, K step 2: group g of eight channels, step k < 4, lane half h supplying channel 8 g + 4 h + k (pointwise.hip `a_off = .. + 4 * half`,
                   `nd_ld4(&As[a_off + g * 8])`, `nd_mfma(av[k], bq[g][k], acc)`; pwchain.hip header: k(j, half) = 8 (j >> 2) + (j & 3) + 4 half) -- the two
                   halves of a step in order.
``gemm32_split``   the split entries: the three-term bf16 split of BOTH operands by split_bf16.h's rule (v1 = bf16(v), v2 = bf16(v - v1), v3 = v - v1 - v2, round to
                   nearest even), per 16-channel K step the six kept products x1 w1, x2 w1, x1 w2, x2 w2, x3 w1, x1 w3 in pointwise_split_kernel's kstep order,
                   each one v_mfma_f32_32x32x16_bf16: its sixteen products are exact in fp32 and are summed here without rounding (fp64), the sum entering the
                   fp32 accumulator with one rounding.  (The rounding inside the instruction's adder tree is not documented; one rounding per instruction is
                   the order with the fewest, and `derived`'s factor 4 covers the others.)
``gemm32_narrow``  the streaming kernels (pointwise_narrow_kernel, pointwise_narrow_fold_kernel): lane part p < 4 owns the channel quads p, p + 4, ... of each source, an
                   fmaf chain per part (`acc = fmaf(x.w, w.w, fmaf(x.z, w.z, fmaf(x.y, w.y, fmaf(x.x, w.x, acc))))`), then (p0 + p1) + (p2 + p3) (the two DPP steps).
"""
import torch
import torch.nn.functional as F

from noisediff_amd import synth

F32, F64 = torch.float32, torch.float64
ACTS = {"none": lambda v: v, "gelu": F.gelu, "silu": F.silu}


def U(name, shape, lo=-1.0, hi=1.0):
    return synth.uniform(29, "pw." + name, shape, lo, hi)


# ---------------------------------------------------------------------------------------------------------------- products

def gemm32_mfma(x, w):
    """x (P, K), w (N, K) fp32 -> (P, N) fp32: see the module docstring.  (The accumulator is held as the fp64 image of its fp32 value between the steps.)"""
    K = x.shape[1]
    x64, w64 = x.double(), w.double().T.contiguous()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=F64)
    for g in range((K + 7) // 8):
        for k in range(4):
            for h in range(2):
                c = 8 * g + 4 * h + k
                if c < K:
                    acc = torch.addcmul(acc, x64[:, c, None], w64[c][None, :]).float().double()
    return acc.float()


def split3(v):
    """split_bf16.h: v == t1 + t2 + t3 exactly, each term a bf16 value (held in fp32)."""
    t1 = v.bfloat16().float()
    r1 = v - t1
    t2 = r1.bfloat16().float()
    t3 = r1 - t2
    assert torch.equal(t3.bfloat16().float(), t3) and torch.equal((t1.double() + t2.double() + t3.double()).float(), v)
    return t1, t2, t3


KEPT = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2))      # (activation term, weight term): pointwise_split_kernel's kstep


def gemm32_split(x, w):
    K = x.shape[1]
    xs, ws = [t.double() for t in split3(x)], [t.double() for t in split3(w)]
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, K, 16):
        for i, j in KEPT:
            acc = (acc.double() + xs[i][:, k0: k0 + 16] @ ws[j][:, k0: k0 + 16].T).float()
    return acc


def gemm32_narrow(x, w, widths=None):
    """``widths``: the channel counts of the sources the kernel strides separately (the fold: c0, c1, c2); the plain narrow kernel strides the concatenation."""
    K = x.shape[1]
    x64, w64 = x.double(), w.double().T.contiguous()
    parts = [torch.zeros(x.shape[0], w.shape[0], dtype=F64) for _ in range(4)]
    base = 0
    for wd in (widths or [K]):
        for q in range(wd // 4):
            for e in range(4):
                c = base + 4 * q + e
                parts[q % 4] = torch.addcmul(parts[q % 4], x64[:, c, None], w64[c][None, :]).float().double()
        base += wd
    p = [t.float() for t in parts]
    return (p[0] + p[1]) + (p[2] + p[3])


def gemm_exact(x, w):
    return x @ w.T


# ---------------------------------------------------------------------------------------------------------------- the operator

def affine_silu(t, mad):
    return F.silu((t - mad[:, None, 0]) * mad[:, None, 1] + mad[:, None, 2])


def layernorm(x, gamma, beta):
    """nn.LayerNorm written out: biased variance, eps 1e-5 (pointwise_kernel's two-pass row statistics)."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + 1e-5) * gamma + beta


def rowstats(inp):
    """(B HW, 2) fp32 {mean, rstd} of x + svec as nd_layernorm_stats_f32 hands them to the kernels: computed in float64, rounded once."""
    x = inp["x"].double() + (inp["svec"].double()[:, None] if "svec" in inp else 0.0)
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    return torch.stack((mean, torch.rsqrt(var + 1e-5)), -1).reshape(-1, 2).float()


def prologue(inp, dt):
    c = lambda name: inp[name].to(dt)
    x = torch.cat((c("x"), c("x2")), -1) if "x2" in inp else c("x")
    pro = inp.get("pro", "none")
    if pro == "silu":
        return F.silu(x)
    if pro == "leaky":
        return F.leaky_relu(x, 0.2)
    if pro == "affine":
        return affine_silu(x, c("mad"))
    if pro == "ln":
        if "svec" in inp:
            x = x + c("svec")[:, None]
        return layernorm(x, c("gamma"), c("beta"))
    assert pro == "none"
    return x


def operator(inp, dt, gemm=gemm_exact):
    c = lambda name: inp[name].to(dt)
    a = prologue(inp, dt)
    B, HW, K = a.shape
    y = gemm(a.reshape(B * HW, K), c("w")).reshape(B, HW, -1)
    if "b" in inp:
        y = y + c("b")
    y = ACTS[inp.get("act", "none")](y)
    if "vec" in inp:
        y = y + c("vec")[:, None]
    if "res0" in inp:
        y = y + c("res0")
    if "res1" in inp:
        y = y + c("res1")
    if "gn_t" in inp:
        y = y + affine_silu(c("gn_t"), c("gn_mad"))
    return y


def narrow_fold(inp, dt, gemm=gemm_exact):
    """``w`` / ``b``: the folded weight (cout, c0 + c1 + c2) and bias, as nd_pack_narrow_fold leaves them."""
    c = lambda name: inp[name].to(dt)
    srcs = [c("x")] + ([c("x2")] if "x2" in inp else []) + [affine_silu(c("t"), c("mad"))]
    a = torch.cat(srcs, -1)
    B, HW, K = a.shape
    y = gemm(a.reshape(B * HW, K), c("w")).reshape(B, HW, -1) + c("b")
    return y + c("res0") if "res0" in inp else y


def chain(inp, dt, gemm=gemm_exact):
    """``ws`` / ``bs``: the stages' weights and biases; ``acts`` / ``res``: per stage, "none" / "gelu" / "silu" and 0 / 1 (+ x + v) / 2 (+ x).  ``tail``: the row is
    silu(affine(x, mad)) + r0 (+ r1).  ``pro``: "none" or "ln" (LayerNorm of x + svec; the residuals see x + svec and x)."""
    c = lambda name: inp[name].to(dt)
    x = torch.cat((c("x"), c("x2")), -1) if "x2" in inp else c("x")
    if inp.get("tail"):
        x = affine_silu(x, c("mad")) + c("r0")
        if "r1" in inp:
            x = x + c("r1")
    xv = x + c("svec")[:, None] if "svec" in inp else x
    h = layernorm(xv, c("gamma"), c("beta")) if inp.get("pro") == "ln" else xv
    B, HW, _ = x.shape
    for i, w in enumerate(inp["ws"]):
        y = gemm(h.reshape(B * HW, -1), w.to(dt)).reshape(B, HW, -1)
        y = inp["bs"][i].to(dt) + y                       # the accumulator starts at the bias
        r = inp.get("res", (0, 0, 0))[i]
        if r == 1:
            y = y + xv
        elif r == 2:
            y = y + (xv - c("svec")[:, None] if "svec" in inp else xv)      # chain_res: `v -= vstash` on the stashed x + v
        h = ACTS[inp.get("acts", ("gelu", "none", "none"))[i]](y)
    return h


def ref64(fn, inp):
    return fn(inp, F64)


def pack_layout(w):
    """nd_pack_pointwise_weight's image of W (cout, cin): [cinP / 4][coutP][4], cinP = cin up to 8, coutP = cout up to 64, zeros in the padding."""
    cout, cin = w.shape
    cinP, coutP = -(-cin // 8) * 8, -(-cout // 64) * 64
    full = torch.zeros(coutP, cinP)
    full[:cout, :cin] = w
    return full.reshape(coutP, cinP // 4, 4).permute(1, 0, 2).contiguous().reshape(-1)
