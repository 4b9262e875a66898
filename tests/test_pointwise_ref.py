"""tests/pointwise_ref.py against torch's own compositions and against itself (CPU): the references the GPU file trusts are checked here first."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R

F32, F64 = torch.float32, torch.float64


def _xw(K, P=24, N=12):
    return R.U(f"ref.x.{K}", (P, K), -1.5, 1.5), R.U(f"ref.w.{K}", (N, K), -0.3, 0.3)


@pytest.mark.parametrize("K", [4, 64, 1024])
def test_fp32_products_against_float64_are_finite_and_ordered(K):
    """Every fp32 product form has a small, non-zero error against float64 that grows with K no faster than K ulps of the largest |x||w| sum (a sequential chain's
    worst case), and the narrow form (four chains of K / 4) is no worse than the single MFMA chain's bound."""
    x, w = _xw(K)
    exact = x.double() @ w.double().T
    mag = float((x.double().abs() @ w.double().abs().T).max())
    errs = {}
    for name, fn in (("mfma", R.gemm32_mfma), ("narrow", R.gemm32_narrow), ("torch", lambda a, b: a @ b.T)) + ((("split", R.gemm32_split),) if K % 16 == 0 else ()):
        y = fn(x, w)
        assert y.dtype == F32 and torch.isfinite(y).all()
        errs[name] = float((y.double() - exact).abs().max())
        assert errs[name] <= K * 2.0 ** -24 * mag, (name, errs[name])
    assert errs["mfma"] > 0 or K == 4
    if K == 1024:
        assert errs["torch"] <= errs["mfma"]          # torch's blocked summation is the more accurate one: not a bound for an MFMA chain


def test_split_emulation_is_no_worse_than_twice_the_plain_chain_at_k_1024():
    """DESIGN: the split is equal in significand to fp32.  An emulation that is worse than 2 x the plain fp32 chain on the same inputs is wrong."""
    x, w = _xw(1024)
    exact = x.double() @ w.double().T
    e_split = float((R.gemm32_split(x, w).double() - exact).abs().max())
    e_plain = float((R.gemm32_mfma(x, w).double() - exact).abs().max())
    assert 0 < e_split <= 2 * e_plain, (e_split, e_plain)


def test_split_terms_are_exact_and_the_dropped_products_are_below_2_to_minus_25():
    v = R.U("ref.split", (4096,), -3.0, 3.0)
    t1, t2, t3 = R.split3(v)
    assert float(t2.abs().max()) <= 2.0 ** -8 * float(v.abs().max()) and float(t3.abs().max()) <= 2.0 ** -16 * float(v.abs().max())
    x, w = _xw(64)
    full = sum(a.double() @ b.double().T for a in R.split3(x) for b in R.split3(w))
    kept = sum(R.split3(x)[i].double() @ R.split3(w)[j].double().T for i, j in R.KEPT)
    assert float((full - x.double() @ w.double().T).abs().max()) < 1e-13          # nine term products: the whole product (fp64 summation order aside)
    assert float((full - kept).abs().max()) <= 3 * 2.0 ** -24 * float((x.double().abs() @ w.double().abs().T).max())


def _operands(B=2, HW=5, cin=12, cout=8):
    return {"x": R.U("op.x", (B, HW, cin), -1.5, 1.5), "w": R.U("op.w", (cout, cin), -0.3, 0.3), "b": R.U("op.b", (cout,)),
            "vec": R.U("op.vec", (B, cout)), "res0": R.U("op.r0", (B, HW, cout)), "res1": R.U("op.r1", (B, HW, cout)),
            "gn_t": R.U("op.t", (B, HW, cout), -2, 2), "gn_mad": R.U("op.mad", (B, 3, cout), 0.5, 1.5),
            "mad": R.U("op.smad", (B, 3, cin), 0.5, 1.5), "gamma": R.U("op.g", (cin,), 0.5, 1.5), "beta": R.U("op.be", (cin,)), "svec": R.U("op.sv", (B, cin))}


@pytest.mark.parametrize("act", ["none", "gelu", "silu"])
@pytest.mark.parametrize("pro", ["none", "silu", "leaky", "affine", "ln"])
def test_operator_reproduces_torch_compositions_in_float64(pro, act):
    o = _operands()
    inp = dict(o, pro=pro, act=act)
    x = o["x"].double()
    d = lambda n: o[n].double()
    if pro == "silu":
        a = F.silu(x)
    elif pro == "leaky":
        a = F.leaky_relu(x, 0.2)
    elif pro == "affine":
        a = F.silu((x - d("mad")[:, None, 0]) * d("mad")[:, None, 1] + d("mad")[:, None, 2])
    elif pro == "ln":
        a = F.layer_norm(x + d("svec")[:, None], (x.shape[-1],), d("gamma"), d("beta"), eps=1e-5)
    else:
        a = x
    y = {"none": lambda v: v, "gelu": F.gelu, "silu": F.silu}[act](F.linear(a, d("w"), d("b")))
    y = y + d("vec")[:, None] + d("res0") + d("res1") + F.silu((d("gn_t") - d("gn_mad")[:, None, 0]) * d("gn_mad")[:, None, 1] + d("gn_mad")[:, None, 2])
    got = R.operator(inp, F64)
    assert got.dtype == F64 and float((got - y).abs().max()) < 1e-13
    # the virtual concat is the concatenation
    if pro in ("none", "silu", "leaky"):
        two = dict(inp, x=o["x"][..., :4].contiguous(), x2=o["x"][..., 4:].contiguous())
        assert torch.equal(R.operator(two, F64), got)
    # every fp32 product form is the same operator
    for fn in (R.gemm32_mfma, R.gemm32_narrow):
        assert float((R.operator(inp, F32, fn).double() - y).abs().max()) < 1e-4


def test_chain_reproduces_mlp_and_attnblock_tail_in_float64():
    B, HW, Cc = 2, 6, 16
    x, v = R.U("ch.x", (B, HW, Cc), -1.5, 1.5), R.U("ch.v", (B, Cc))
    ws = [R.U("ch.w0", (32, Cc), -0.3, 0.3), R.U("ch.w1", (Cc, 32), -0.3, 0.3), R.U("ch.w2", (Cc, Cc), -0.3, 0.3)]
    bs = [R.U("ch.b0", (32,)), R.U("ch.b1", (Cc,)), R.U("ch.b2", (Cc,))]
    g, be = R.U("ch.g", (Cc,), 0.5, 1.5), R.U("ch.be", (Cc,))
    D = [t.double() for t in ws], [t.double() for t in bs]
    mlp = F.linear(F.gelu(F.linear(x.double(), D[0][0], D[1][0])), D[0][1], D[1][1])
    assert float((R.chain({"x": x, "ws": ws[:2], "bs": bs[:2]}, F64) - mlp).abs().max()) < 1e-13
    x1 = x.double() + v.double()[:, None]
    h = F.gelu(F.linear(F.layer_norm(x1, (Cc,), g.double(), be.double(), eps=1e-5), D[0][0], D[1][0]))
    tail = F.linear(F.linear(h, D[0][1], D[1][1]) + x1, D[0][2], D[1][2]) + x.double()
    inp = {"x": x, "svec": v, "gamma": g, "beta": be, "pro": "ln", "ws": ws, "bs": bs, "res": (0, 1, 2)}
    assert float((R.chain(inp, F64) - tail).abs().max()) < 1e-13
    assert float((R.chain(inp, F32, R.gemm32_mfma).double() - tail).abs().max()) < 1e-4
    # the tail prologue
    mad, r0, r1 = R.U("ch.mad", (B, 3, Cc), 0.5, 1.5), R.U("ch.r0", (B, HW, Cc)), R.U("ch.r1", (B, HW, Cc))
    row = F.silu((x.double() - mad.double()[:, None, 0]) * mad.double()[:, None, 1] + mad.double()[:, None, 2]) + r0.double() + r1.double()
    ref = F.linear(F.gelu(F.linear(row, D[0][0], D[1][0])), D[0][1], D[1][1])
    got = R.chain({"x": x, "tail": True, "mad": mad, "r0": r0, "r1": r1, "ws": ws[:2], "bs": bs[:2]}, F64)
    assert float((got - ref).abs().max()) < 1e-13


def test_narrow_fold_and_pack_layout():
    B, HW, d, cout = 2, 7, 8, 4
    inp = {"x": R.U("nf.x", (B, HW, d)), "x2": R.U("nf.x2", (B, HW, d)), "t": R.U("nf.t", (B, HW, d), -2, 2), "mad": R.U("nf.mad", (B, 3, d), 0.5, 1.5),
           "w": R.U("nf.w", (cout, 3 * d), -0.3, 0.3), "b": R.U("nf.b", (cout,)), "res0": R.U("nf.r", (B, HW, cout))}
    D = {k: v.double() for k, v in inp.items()}
    a = torch.cat((D["x"], D["x2"], F.silu((D["t"] - D["mad"][:, None, 0]) * D["mad"][:, None, 1] + D["mad"][:, None, 2])), -1)
    ref = F.linear(a, D["w"], D["b"]) + D["res0"]
    assert float((R.narrow_fold(inp, F64) - ref).abs().max()) < 1e-13
    assert float((R.narrow_fold(inp, F32, lambda x, w: R.gemm32_narrow(x, w, [d, d, d])).double() - ref).abs().max()) < 1e-5
    w = R.U("pk.w", (5, 12))
    p = R.pack_layout(w).reshape(16 // 4, 64, 4)
    assert p.numel() == 16 * 64 and p[2, 3, 1] == w[3, 9] and (p[3] == 0).all() and (p[:, 5:] == 0).all()
