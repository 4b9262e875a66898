"""The checkers of tests/conv3x3_ref.py on the CPU: they admit correct fp32 evaluations of every case of the GPU file's table and reject subtly wrong ones.

Admits: for every case and every entry's bound (the direct kernel's chain, the Winograd formula for m = 2 and m = 4) other legitimate fp32 evaluations of the same
operator stay inside it -- F.conv2d in fp32; for a Winograd bound the same formula with U rounded once from float64 (as the packers form it) and with the
transforms taken columns before rows; for the direct kernel's bound the chain with the taps outside the chunks.
Rejects: eight mutations of a correct output, each at the smallest and the largest case.  The one-pass M2 is taken at those two shapes with the `offset` case's weights
and bias (output mean / std ~ 100): with a mean near 0 a one-pass M2 is a correct evaluation, and the conditioning is what the mutation is about.
"""
import pytest
import torch
import torch.nn.functional as F

import conv3x3_ref as R

KINDS = ("direct", 2, 4)
SMALLEST, LARGEST = "tiny", "second_trip"


def guarded_out(t, pad=4):
    """Host image of the GPU file's output allocation around a result: [1 + B H + 1][W][cout + pad], NaN outside the tensor."""
    B, H, W, Cc = t.shape
    buf = torch.full((B * H + 2, W, Cc + pad), float("nan"))
    buf[1:-1, :, :Cc] = t.reshape(B * H, W, Cc)
    return buf


def check(t, r64, r32, what=""):
    buf = guarded_out(t)
    return R.check_conv(buf[1:-1, :, : t.shape[-1]].reshape(t.shape), buf, r64, r32, what)


@pytest.mark.parametrize("kind", KINDS, ids=str)
@pytest.mark.parametrize("case", list(R.CASES))
def test_other_fp32_evaluations_are_admitted(case, kind):
    inp, r64, r32 = R.references(case, "none", kind)
    others = {"F.conv2d": R.conv2d32(inp)}
    if kind == "direct":
        others["taps outside the chunks"] = R.ref32_direct(inp, taps_outer=True)
    else:
        others["U rounded once from float64"] = R.ref32_winograd(kind, inp, u_from64=True)
        others["columns before rows"] = R.ref32_winograd(kind, inp, cols_first=True)
    for name, t in others.items():
        check(t, r64, r32, f"{case} {kind} {name}")


@pytest.mark.parametrize("kind", (2, 4), ids=str)
def test_the_winograd_formula_in_float64_is_the_convolution(kind):
    inp = R.inputs("ragged")
    err = float((R.ref32_winograd(kind, inp, dtype=torch.float64) - R.ref64(inp)).abs().max())
    assert err < 2.0 ** -40 * float(R.ref64(inp).abs().max())      # float64 rounding of a 40 x 9-term sum: nothing of the formula is approximate


def test_split_ranges_are_admitted_by_the_unsplit_bound_and_differ_from_it():
    inp, r64, r32 = R.references("deep", "none", 4)
    split = R.ref32_winograd(4, inp, ranges=[(i * 64, (i + 1) * 64) for i in range(8)])
    assert not torch.equal(split, r32)
    check(split, r64, r32, "deep, 8 ranges")


# ---------------------------------------------------------------------------------------------------------------- mutations

def correct(case, pro="none", kind="direct"):
    """A correct output (the fp32 reference itself, a copy) with what the mutations need."""
    inp, r64, r32 = R.references(case, pro, kind)
    return inp, r64, r32, r32.clone()


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


@pytest.mark.parametrize("kind", KINDS, ids=str)
@pytest.mark.parametrize("case", [SMALLEST, LARGEST])
def test_output_mutations_are_rejected(case, kind):
    inp, r64, r32, good = correct(case, "none", kind)
    B, H, W, cin, cout = inp["shape"]
    check(good, r64, r32)
    act = R.activated(inp, torch.float32)

    m = good.clone()                                                  # the bias left out of the last channel quad
    m[..., -4:] -= inp["b"][-4:]
    rejected(check, m, r64, r32)

    m = good.clone()                                                  # one tap of one border pixel dropped: tap (1, 1) of pixel (0, W - 1) of the last sample
    m[-1, 0, W - 1] -= inp["w"][:, :, 1, 1] @ act[-1, :, 0, W - 1]
    rejected(check, m, r64, r32)

    m = good.clone()                                                  # the last K chunk's ragged channels dropped (the eight behind the last multiple of 16, or the last eight)
    r = cin % 16 or 8
    m -= F.conv2d(act[:, -r:], inp["w"][:, -r:], None, padding=1).permute(0, 2, 3, 1)
    rejected(check, m, r64, r32)

    m = good.clone()                                                  # one 4 x 4 output tile written one pixel to the right (in memory order: a 4-pixel row spills into the next)
    flat, g = m.reshape(B * H * W, cout), good.reshape(B * H * W, cout)
    for y in range(4):
        flat[y * W + 1: y * W + 5] = g[y * W: y * W + 4]
    rejected(check, m, r64, r32)

    buf = guarded_out(good)                                           # a finite value in one guard column
    buf[1 + H // 2, W - 1, cout + 3] = 0.0
    rejected(R.check_conv, good, buf, r64, r32)
    buf = guarded_out(good)                                           # ... in the guard row behind the tensor
    buf[-1, 0, 0] = 1.0
    rejected(R.check_conv, good, buf, r64, r32)


@pytest.mark.parametrize("kind", KINDS, ids=str)
@pytest.mark.parametrize("case", [SMALLEST, LARGEST])
def test_padding_before_the_activation_is_rejected(case, kind):
    """One border row computed from the tensor padded BEFORE affine + SiLU: silu(D - M A) != 0 instead of 0 around the image."""
    inp, r64, r32, good = correct(case, "affine", kind)
    check(good, r64, r32)
    wrong = F.conv2d(R.activated(inp, torch.float32, pad_first=True), inp["w"], inp["b"]).permute(0, 2, 3, 1)
    m = good.clone()
    m[:, 0] = wrong[:, 0]
    rejected(check, m, r64, r32)


def stats_of(out32, per_slot):
    """Correct fp32 statistics of an fp32 output in the kernels' layout, with their guarded host buffers."""
    s, m2, cnt = R.slot_stats(out32, 16 if per_slot else 8)           # (pooled form: any partition will do -- 8 x 8 tiles)
    return torch.stack((s, m2), -1), cnt.float()


def guarded_flat(t, guard=64):
    buf = torch.full((t.numel() + 2 * guard,), float("nan"))
    buf[guard: guard + t.numel()] = t.reshape(-1)
    return buf


def check_st(st, sc, r64, r32, per_slot, pivot, stb=None, scb=None):
    return R.check_stats(st, sc, guarded_flat(st) if stb is None else stb, guarded_flat(sc) if scb is None else scb, 64, r64, r32, per_slot, "", pivot)


@pytest.mark.parametrize("pivoted", [False, True], ids=["two_pass_bound", "pivoted_bound"])
@pytest.mark.parametrize("per_slot", [True, False], ids=["per_slot", "pooled"])
@pytest.mark.parametrize("case", [SMALLEST, LARGEST])
def test_statistics_mutations_are_rejected(case, per_slot, pivoted):
    """Under both fp32 statistics references: the two-pass one (direct kernel, conv3x3_wino.hip) and the one-pass one about the slot's first pixel (16 x 16 slots:
    the F(4x4) forms, 8 x 16: conv3x3_wino2.hip).  Either admits the other's partials."""
    inp = R.inputs("offset", shape=R.CASES[case])                      # the offset case's weights and bias at this shape: mean / std ~ 100
    r64, r32 = R.ref64(inp), R.ref32_winograd(4, inp)
    B, H, W, cin, cout = inp["shape"]
    pivot = ((16, 16) if per_slot else (8, 16)) if pivoted else None
    st, sc = stats_of(r32, per_slot)
    check_st(st, sc, r64, r32, per_slot, pivot)
    if per_slot:
        ps, pm, pn = R.slot_stats_pivoted(r32, 16, 16)
        check_st(torch.stack((ps, pm), -1), pn.float(), r64, r32, per_slot, pivot)

    tile = 16 if per_slot else 8                                      # M2 taken one-pass without a pivot in fp32: sum v^2 - (sum v)^2 / n
    tx = R.cdiv(W, tile)
    m = st.clone()
    m[..., 1] = R.slot_stats(r32 * r32, tile)[0] - st[..., 0] ** 2 / sc[None, :, None]
    rejected(check_st, m, sc, r64, r32, per_slot, pivot)

    c = sc.clone()                                                    # one slot's count off by one row
    c[-1] -= min(tile, W - (tx - 1) * tile)
    rejected(check_st, st, c, r64, r32, per_slot, pivot)

    stb = guarded_flat(st)                                            # a finite value behind the statistics / in front of slot_count
    stb[-64] = 0.0
    rejected(check_st, st, sc, r64, r32, per_slot, pivot, stb)
    scb = guarded_flat(sc)
    scb[63] = 256.0
    rejected(check_st, st, sc, r64, r32, per_slot, pivot, None, scb)

    m = st.clone()                                                    # one channel's sum of one slot taken over one pixel less
    m[0, 0, 0, 0] -= r32[0, 0, 0, 0]
    rejected(check_st, m, sc, r64, r32, per_slot, pivot)


# ---------------------------------------------------------------------------------------------------------------- F(4x4) packed weights

@pytest.mark.parametrize("cin,cout", [(24, 8), (72, 40), (64, 64)])
def test_the_wino4_layout_helpers_invert_each_other_and_follow_the_header(cin, cout):
    """wino4_unpack(wino4_pack_layout(U)) gives U back with zero padding, and the encode puts every entry where the header's index formula says:
    float 4 l + e of position pair pp of block (c8, cg) holds U[position 2 pp + (e >> 1)] of (cout 16 cg + (l & 15), channel 8 c8 + 2 (l >> 4) + (e & 1))."""
    U = torch.rand(cout, cin, 6, 6, generator=torch.Generator().manual_seed(cin + cout)) + 0.5          # (no zero: padding is told from data)
    packed = R.wino4_pack_layout(U, cin, cout)
    back, pad = R.wino4_unpack(packed, cin, cout)
    assert torch.equal(back, U) and not pad.any()
    assert pad.numel() + U.numel() == packed.numel() == 2 * R.cdiv(R.cdiv(cin, 8), 2) * 4 * R.cdiv(cout, 64) * 18 * 256
    n_cg = 4 * R.cdiv(cout, 64)
    for i in torch.randint(0, packed.numel(), (2000,), generator=torch.Generator().manual_seed(1)).tolist() + [0, packed.numel() - 1]:
        e, l, pp, blk = i % 4, (i // 4) % 64, (i // 256) % 18, i // (18 * 256)
        cg, c8 = blk % n_cg, blk // n_cg
        co, ch, pos = 16 * cg + (l & 15), 8 * c8 + 2 * (l >> 4) + (e & 1), 2 * pp + (e >> 1)
        want = float(U[co, ch, pos // 6, pos % 6]) if co < cout and ch < cin else 0.0
        assert float(packed[i]) == want, (i, co, ch, pos)


def test_wino4_U_in_float64_is_exact_to_rounding():
    """G g G^T with float64 G against the same product in exact rational arithmetic on one filter."""
    from fractions import Fraction as Fr
    G = [[Fr(1, 4), 0, 0], [Fr(-1, 6), Fr(-1, 6), Fr(-1, 6)], [Fr(-1, 6), Fr(1, 6), Fr(-1, 6)], [Fr(1, 24), Fr(1, 12), Fr(1, 6)], [Fr(1, 24), Fr(-1, 12), Fr(1, 6)], [0, 0, 1]]
    g = torch.rand(1, 1, 3, 3, generator=torch.Generator().manual_seed(2)) - 0.5
    U = R.wino4_U(g, torch.float64)[0, 0]
    for xi in range(6):
        for nu in range(6):
            exact = sum(G[xi][r] * Fr(float(g[0, 0, r, s])) * G[nu][s] for r in range(3) for s in range(3))
            assert abs(Fr(float(U[xi, nu])) - exact) <= Fr(1, 2 ** 50) * max(abs(exact), Fr(1, 100))
