"""The conv3x3 kernel family against float64 at its edge shapes: nd_conv3x3_nhwc_f32, nd_conv3x3_wino_nhwc_f32, nd_conv3x3_wino2_nhwc_f32, nd_conv3x3_wino4_nhwc_f32,
nd_conv3x3_wino4_16_nhwc_f32 and the two split-K forms, each through its own packer, called directly through ctypes.

Every bound is util.derived on an fp32 reference of tests/conv3x3_ref.py (the direct kernel's chain, the Winograd formula for m = 2 / 4); no tolerance is a literal.

Buffers (``Guarded``): every source has a pixel stride 8 floats (the second concat source: 16) wider than its channel count with NaN in the unused columns, the output
ldo = cout + 4 and a NaN prefill; each tensor has one NaN image row in front of it and one behind it inside the same allocation; the flat operands (M / A / D, bias,
statistics, slot_count, split-K workspace, the in-kernel map's weights) get 64 NaN floats on each side.  A kernel that multiplies what it should not have read, or stores
outside its region, turns up as NaN.  The scale / shift map and the position embedding have NO pixel stride in nd_src (2 C and 8 floats per pixel, fixed): they
are dense, with the guard rows only.

Refusals are enumerated in ``refusal``: a listed (entry, shape, prologue) must return non-zero with a message and leave the output untouched, an unlisted one that
refuses fails its test.  What the table holds and the line each entry rests on:
  * split-K, any case whose cin is not `splits` ranges of at least two whole 16-channel chunks -- every case of the table but `deep` (cin = 32, 24, 40):
    conv3x3_wino4.hip w4_splitk, "splits=%d must be 2, 4 or 8 and divide cin".  Their numeric checks run in test_split_k at cin = 64, 128 and 512.
  * concat / LeakyReLU-on-the-second-source where cin has no chunk boundary inside: wino2 at cin = 24 (conv3x3_wino2.hip "a 32-channel K chunk must not straddle").
  * the blocked map outside nd_conv3x3_wino4_nhwc_f32 ("blocked map layout is read by nd_conv3x3_wino4_nhwc_f32 only") and there at cin % 16 != 0 ("map_blocked needs");
    the in-kernel map likewise (16 x 32 form only, cin % 16 == 0; the F(2x2) and direct kernels: "unsupported prologue 7").
  * LeakyReLU and map prologues on the 16 x 16 and split-K forms ("plain or GroupNorm-affine + SiLU sources").
  * cout = 2052 on every F(4x4) entry ("cout <= 2048").
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv3x3_ref as R
from hiputil import GUARD, Guarded, nan_like
from noisediff_amd import _lib as L
from noisediff_amd._host import CONV3X3

# name -> (C entry, packer, fp32 reference kind, channels a K chunk holds for a virtual concat's boundary, one statistics slot per 16 x 16 tile, split-K,
#          slot (rows, columns) of a one-pass pivoted statistics epilogue or None for the two-pass one: conv3x3_ref.slot_stats_pivoted)
ENTRIES = {
    "direct": ("nd_conv3x3_nhwc_f32", "nd_pack_conv3x3_weight", "direct", 8, False, False, None),
    "wino": ("nd_conv3x3_wino_nhwc_f32", "nd_pack_conv3x3_wino_weight", 2, 8, False, False, None),
    "wino2": ("nd_conv3x3_wino2_nhwc_f32", "nd_pack_conv3x3_wino_weight", 2, 32, False, False, (8, 16)),
    "wino4": ("nd_conv3x3_wino4_nhwc_f32", "nd_pack_conv3x3_wino4_weight", 4, 16, True, False, (16, 16)),
    "wino4_16": ("nd_conv3x3_wino4_16_nhwc_f32", "nd_pack_conv3x3_wino4_weight", 4, 16, True, False, (16, 16)),
    "wino4_splitk": ("nd_conv3x3_wino4_splitk_nhwc_f32", "nd_pack_conv3x3_wino4_weight", 4, 16, True, True, (16, 16)),
    "wino4_16_splitk": ("nd_conv3x3_wino4_16_splitk_nhwc_f32", "nd_pack_conv3x3_wino4_weight", 4, 16, True, True, (16, 16)),
}
KERNELS = {entry: CONV3X3[entry.replace("_splitk", "")].kernel for entry in ENTRIES}      # what nd_conv3x3_takes is asked about: the split-K entries are their kernel's
MODES = {"none": L.PRO_NONE, "concat": L.PRO_NONE, "upsample": L.PRO_NONE, "affine": L.PRO_AFFINE_SILU, "map": L.PRO_AFFINE_MAP_SILU, "map_blocked": L.PRO_AFFINE_MAP_SILU,
         "genmap": L.PRO_AFFINE_GENMAP_SILU, "leaky": L.PRO_LEAKY, "leaky_second": L.PRO_LEAKY_SECOND}
STATS_PROLOGUES = ("none", "affine", "map", "map_blocked", "genmap", "concat")      # what the sampler puts in front of a convolution whose output a GroupNorm follows


def refusal(entry, shape, pro, c0=0, splits=0):
    """The documented refusals: a fragment of the message the entry must leave, or None where it must compute."""
    B, H, W, cin, cout = shape
    f4 = ENTRIES[entry][2] == 4
    if f4 and cout > 2048:
        return "cout <= 2048"
    if f4 and cin <= 16:
        return "cin > 16"
    if pro in ("concat", "leaky_second") and c0 % ENTRIES[entry][3] and entry in ("wino2", "wino4", "wino4_16", "wino4_splitk", "wino4_16_splitk"):
        return "straddle"
    if pro == "map_blocked":
        if not f4:
            return "blocked map layout"
        if cin % 16:
            return "map_blocked needs"
    if pro == "genmap":
        if not f4:
            return "unsupported prologue"
        if entry != "wino4" or cin % 16:
            return "in-kernel map prologue"
    if entry != "wino4" and f4 and pro in ("map", "map_blocked", "leaky", "leaky_second"):
        return "plain or GroupNorm-affine"
    if ENTRIES[entry][5] and (splits not in (2, 4, 8) or cin % 16 or (cin // 16) % splits or cin // 16 // splits < 2):
        return "must be 2, 4 or 8 and divide cin"
    return None


@pytest.fixture(scope="module")
def ctx():
    import hiputil
    return hiputil.Ctx()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def build_src(inp):
    """nd_src of a prologue's operands; returns it with the Guarded buffers that keep its pointers alive."""
    pro, cin = inp["pro"], inp["shape"][3]
    s, keep = L.Src(), []
    g0 = Guarded(nhwc(inp["x"]), 8)
    s.p0, s.c0, s.ld0 = g0.ptr, inp["x"].shape[1], g0.ld
    keep.append(g0)
    if "x2" in inp:
        g1 = Guarded(nhwc(inp["x2"]), 16)                                 # another pixel stride than the first source's
        s.p1, s.c1, s.ld1 = g1.ptr, inp["x2"].shape[1], g1.ld
        keep.append(g1)
    s.mode, s.upsample = MODES[pro], int(pro == "upsample")
    if "M" in inp:
        mad = Guarded(torch.stack((inp["M"], inp["A"], inp["D"]), 1))
        s.mad = mad.ptr
        keep.append(mad)
    if pro == "map":
        mp = Guarded(nhwc(torch.cat((inp["sc"], inp["sh"]), 1)), 0)
    elif pro == "map_blocked":                                            # [B][H][W][C / 16][scale 16 | shift 16]; a ragged last block where the entry must refuse anyway
        B, H, W = inp["sc"].shape[0], inp["sc"].shape[2], inp["sc"].shape[3]
        if cin % 16 == 0:
            sc, sh = nhwc(inp["sc"]).reshape(B, H, W, cin // 16, 16), nhwc(inp["sh"]).reshape(B, H, W, cin // 16, 16)
            mp = Guarded(torch.stack((sc, sh), 4).reshape(B, H, W, 2 * cin), 0)
        else:
            mp = Guarded(nhwc(torch.cat((inp["sc"], inp["sh"]), 1)), 0)
        s.map_blocked = 1
    elif pro == "genmap":
        mp = Guarded(nhwc(inp["pe"]), 0)
        gw, gb = Guarded(inp["gw"]), Guarded(inp["gb"])
        s.gamma, s.beta = gw.ptr, gb.ptr
        keep += [gw, gb]
    else:
        mp = None
    if mp is not None:
        s.map = mp.ptr
        keep.append(mp)
    s._refs = keep
    return s


_packed = {}


def packed(ctx, entry, inp):
    import hiputil as hu
    key = (ENTRIES[entry][1], inp["case"], inp["shape"])
    if key not in _packed:
        if len(_packed) > 6:
            _packed.clear()
        cout, cin = inp["w"].shape[:2]
        wd = hu.dev(inp["w"])
        wp = hu.full((getattr(ctx.lib, ENTRIES[entry][1] + "_floats")(cin, cout),))
        L.call(ENTRIES[entry][1], wd.data_ptr(), wp.data_ptr(), cin, cout, ctx.stream)
        ctx.sync()
        _packed[key] = wp
    return _packed[key]


def stat_slots(ctx, entry, shape):
    B, H, W, cin, cout = shape
    if entry == "direct":
        return ctx.lib.nd_conv3x3_stat_slots(H, W, cout, B)
    return ctx.lib.nd_conv3x3_wino4_stat_slots(H, W) if ENTRIES[entry][4] else ctx.lib.nd_conv3x3_wino_stat_slots(H, W)


def launch(ctx, entry, inp, stats, splits=0):
    """One call of an entry on guarded buffers -> (return code, message, output Guarded, statistics Guarded, slot_count Guarded, workspace Guarded)."""
    B, H, W, cin, cout = inp["shape"]
    d = L.Conv3x3()
    d.src = src = build_src(inp)
    wp, bias, out = packed(ctx, entry, inp), Guarded(inp["b"]), nan_like((B, H, W, cout), 4)
    d.weight, d.bias, d.out = wp.data_ptr(), bias.ptr, out.ptr
    d.B, d.H, d.W, d.cin, d.cout, d.ldo = B, H, W, cin, cout, out.ld
    st = sc = ws = None
    if stats:
        slots = stat_slots(ctx, entry, inp["shape"])
        st, sc = nan_like((B, slots, cout, 2)), nan_like((slots,))
        d.stats, d.slot_count = st.ptr, sc.ptr
    fn = getattr(ctx.lib, ENTRIES[entry][0])
    if ENTRIES[entry][5]:
        n = ctx.lib.nd_conv3x3_wino4_splitk_workspace_floats(B, H, W, cout, max(splits, 1))
        ws = nan_like((n,))
        rc = fn(C.byref(d), ws.ptr, splits, ctx.stream)
    else:
        rc = fn(C.byref(d), ctx.stream)
    msg = ctx.lib.nd_last_error().decode() if rc else ""
    try:
        ctx.sync()
    except L.HipError as e:
        rc, msg = 1, str(e)
    if rc > 0:          # a HIP error, not a refusal (those are negative): the device may have faulted -- nothing more runs on it from this file
        pytest.exit(f"{entry} {inp['case']} {inp['pro']}: HIP error {rc}: {msg}", returncode=3)
    # The library's own answer for this entry and descriptor agrees with what the entry did: every pointer of this file is valid and aligned, so a refusal here
    # is a refusal of the shape.  (A split-K entry called with splits <= 1 refuses; the question at splits <= 1 is about the plain entry and is not asked.)
    if not ENTRIES[entry][5] or splits > 1:
        takes = ctx.lib.nd_conv3x3_takes(KERNELS[entry], C.byref(d), splits if ENTRIES[entry][5] else 1)
        assert takes == (rc == 0), f"{entry} {inp['case']} {inp['pro']}: nd_conv3x3_takes says {takes}, the entry returned {rc} '{msg}'"
        assert not rc or ctx.lib.nd_last_error().decode() == msg, "nd_conv3x3_takes wrote to nd_last_error"
    del src
    return rc, msg, out, st, sc, ws


def concat_c0(entry, cin):
    """First-source channels of a virtual concat: the entry's first K-chunk boundary, or -- where cin has none inside -- 16 (refused by the 32-channel kernels)."""
    u = ENTRIES[entry][3]
    return u if u < cin else 16


def run_and_check(ctx, entry, case, pro, splits=0, shape=None, stats_too=None):
    """Numeric check of one (entry, case, prologue) with and without statistics, or its enumerated refusal."""
    shp = shape or (R.UPSAMPLE_TWIN[case] if pro == "upsample" else R.CASES[case])
    cin = shp[3]
    c0 = concat_c0(entry, cin) if pro in ("concat", "leaky_second") else 0
    why = refusal(entry, shp, pro, c0, splits)
    if why is not None:
        inp = R.inputs(case, pro, c0, shape)
        rc, msg, out, *_ = launch(ctx, entry, inp, False, splits)
        assert rc != 0 and why in msg, f"{entry} {case} {pro}: expected a refusal with '{why}', got rc {rc} '{msg}'"
        assert torch.isnan(out.host()).all(), f"{entry} {case} {pro}: a refused call wrote to the output"
        return "refused"
    kind, per_slot = ENTRIES[entry][2], ENTRIES[entry][4]
    ranges = [(i * cin // splits, (i + 1) * cin // splits) for i in range(splits)] if splits else None
    inp, r64, r32 = R.references(case, pro, kind, c0, ranges, shape)
    what = f"{entry} {case} {pro}" + (f" splits={splits}" if splits else "")
    for stats in ((False, True) if (pro in STATS_PROLOGUES if stats_too is None else stats_too) else (False,)):
        rc, msg, out, st, sc, ws = launch(ctx, entry, inp, stats, splits)
        assert rc == 0, f"{what}: refused ({rc}: {msg}) but not listed in `refusal`"
        buf = out.host()
        R.check_conv(out.tensor(buf), buf, r64, r32, what + (" +stats" if stats else ""))
        if ws is not None:
            wsb = ws.host()
            R.only_nan_outside(wsb, ws.region, what + " workspace")
        if stats:
            stb, scb = st.host(), sc.host()
            R.check_stats(st.tensor(stb), sc.tensor(scb), stb, scb, GUARD, r64, r32, per_slot, what, ENTRIES[entry][6])
    return "computed"


# ---------------------------------------------------------------------------------------------------------------- the cases, plain sources

def items(entry, shape):
    """Workgroup items of a shape from each kernel's documented tile, and the workgroups per CU it keeps resident."""
    B, H, W, cin, cout = shape
    cd = R.cdiv
    if entry == "wino4":
        return B * cd(H, 16) * cd(W, 32) * cd(cout, 64), 1          # 16 x 32 regions x 64 couts, one workgroup per CU
    if entry == "wino4_16":
        return B * cd(H, 16) * cd(W, 16) * cd(cout, 64), 2          # 16 x 16 regions, two per CU
    if entry in ("wino", "wino2"):                                  # 16 x 16 tiles x 64 couts; wino2: one workgroup per CU, wino: 256 registers, two waves per SIMD
        return B * cd(H, 16) * cd(W, 16) * cd(cout, 64), 1 if entry == "wino2" else 2
    return None                                                     # (the split-K forms refuse the case's cin)


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_plain_source_every_case(ctx, entry, case):
    """Every entry on every case, with and without statistics; the split-K entries with splits = 2 (refused wherever cin is not 2 x at least two chunks: listed)."""
    shape = R.CASES[case]
    if case == "second_trip":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if entry == "direct":
            # its tiling: choose_tiling takes (16, 2, 2) -- 8 x 16 pixels x 128 couts -- only for cout % 128 == 0; cout = 180 runs (16, 2, 1): 8 x 16 pixels x 64 couts
            B, H, W, cin, cout = shape
            assert ctx.lib.nd_conv3x3_tiling_id(B, H, W, cout) == 1621
            n, per_cu = B * R.cdiv(H, 8) * R.cdiv(W, 16) * R.cdiv(cout, 64), 4
        elif items(entry, shape):
            n, per_cu = items(entry, shape)
        else:
            n = per_cu = None
        if n is not None:
            assert n > cus * per_cu, f"{entry}: {n} items do not exceed {cus} CUs x {per_cu}: no persistent workgroup takes a second trip on this part"
    splits = 2 if ENTRIES[entry][5] else 0
    did = run_and_check(ctx, entry, case, "none", splits)
    # only the split-K forms refuse cases of the table (their cin); `tiny` may be refused by a Winograd entry, and none does: everything else has computed
    assert did == "computed" or ENTRIES[entry][5], f"{entry} refused {case}"


@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][2] == 4])
def test_cout_above_the_lds_bias_vector_is_refused(ctx, entry):
    B, H, W, cin, cout = R.CASES["all_bias"]
    assert run_and_check(ctx, entry, "all_bias", "none", 2 if ENTRIES[entry][5] else 0, shape=(B, H, W, cin, 2052)) == "refused"


# ---------------------------------------------------------------------------------------------------------------- prologues and addressing

@pytest.mark.parametrize("pro", [p for p in R.PROLOGUES if p != "none"])
@pytest.mark.parametrize("case", ["one_over", "ragged", "deep"])
@pytest.mark.parametrize("entry", [e for e in ENTRIES if not ENTRIES[e][5]])
def test_prologues_and_addressing(ctx, entry, case, pro):
    """Affine + SiLU, the per-pixel map (planar, blocked, formed in the kernel), LeakyReLU (whole input / second source), virtual concat on the entry's chunk boundary
    with different pixel strides, nearest-x2 upsample on the even-sized twins -- or the enumerated refusal."""
    run_and_check(ctx, entry, case, pro)


@pytest.mark.parametrize("entry", ["wino2", "wino4", "wino4_16"])
def test_concat_off_the_chunk_boundary_is_refused(ctx, entry):
    inp = R.inputs("ragged", "concat", 8)
    rc, msg, out, *_ = launch(ctx, entry, inp, False)
    assert rc != 0 and "straddle" in msg
    assert torch.isnan(out.host()).all()


def test_map_with_upsample_is_refused_on_wino2(ctx):
    """conv3x3_wino2.hip: "map prologue with upsample is not supported here"."""
    inp = dict(R.inputs("ragged", "map", shape=R.UPSAMPLE_TWIN["ragged"]))
    inp["x"] = inp["x"][:, :, ::2, ::2].contiguous()                      # the half-size source behind a full-size map
    B, H, W, cin, cout = inp["shape"]
    d = L.Conv3x3()
    s = build_src(inp)
    s.upsample = 1
    d.src = s
    out = nan_like((B, H, W, cout), 4)
    d.weight, d.out = packed(ctx, "wino2", inp).data_ptr(), out.ptr
    d.B, d.H, d.W, d.cin, d.cout, d.ldo = B, H, W, cin, cout, out.ld
    assert ctx.lib.nd_conv3x3_wino2_nhwc_f32(C.byref(d), ctx.stream) != 0
    assert b"map prologue with upsample" in ctx.lib.nd_last_error()
    ctx.sync()
    assert torch.isnan(out.host()).all()


# ---------------------------------------------------------------------------------------------------------------- split-K

SPLITK = {"c64_s2": (64, 2), "c128_s4": (128, 4), "deep_s2": (512, 2), "deep_s4": (512, 4), "deep_s8": (512, 8)}


@pytest.mark.parametrize("pro", ["none", "affine"])
@pytest.mark.parametrize("cfg", list(SPLITK))
@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][5]])
def test_split_k(ctx, entry, cfg, pro):
    """Explicit split counts: two chunks per range (the minimum) at cin = 64, four ranges at 128, 2 / 4 / 8 at `deep`; (2, 19, 37) pixels x 68 couts otherwise.  With and
    without statistics (the reduction's own statistics kernel), plain and affine + SiLU; the NaN-prefilled workspace is exactly the partial tensors.  fp32 reference:
    the F(4x4) formula per K range, the ranges added in order."""
    cin, splits = SPLITK[cfg]
    if cfg.startswith("deep"):
        assert run_and_check(ctx, entry, "deep", pro, splits, stats_too=True) == "computed"
    else:
        assert run_and_check(ctx, entry, "ragged", pro, splits, shape=(2, 19, 37, cin, 68), stats_too=True) == "computed"


@pytest.mark.parametrize("splits", [0, 3, 4, 8, 16])
@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][5]])
def test_split_counts_that_do_not_divide_the_chunks_are_refused(ctx, entry, splits):
    """cin = 64 is four chunks: only splits = 2 leaves two per range."""
    assert run_and_check(ctx, entry, "ragged", "none", splits, shape=(2, 19, 37, 64, 68)) == "refused"
