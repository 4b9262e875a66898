"""References, restated plans and the checker for the weight-gradient kernels (conv3x3_wgrad.hip, linear_wgrad.hip): plain torch on the CPU, no GPU, no library.

``ref64``                  dW, db in float64: torch.nn.grad.conv2d_weight(padding=1) on the activated, concatenated input; the linear case g.T @ x.
``ref32_nine_tap``         the same sum in fp32 as chains in wgrad_kernel's order: split slot s walks the tiles s, s + S, .. of the 16 x 8 tiling, a tile's pixel pairs row by
                           row (the two halves of a v_mfma_f32_32x32x2_f32 in order), the S partials added in slot order (wgrad_reduce_kernel); the bias through its four
                           pixel quarters ((q0 + q1) + q2) + q3, then in slot order.  Not conv2d_weight in fp32: torch's blocked sum is more accurate than an MFMA chain and a
                           bound taken from it would reject a correct kernel (conv3x3_ref.py).
``ref32_linear``           linear_wgrad_kernel's chain: slot s walks the 128-token chunks s, s + S, ..; the slots meet as linear_wgrad_reduce_kernel adds them: eight stripes
                           (s = k, k + 8, ..), then the stripes in stripe order.
``ref32_winograd_domain``  the Winograd-domain formula of the kernel's header in fp32: V = B^T d B and D = A dY A^T per 4 x 4 tile (rows, then columns; the matrices are
                           conv3x3_ref.WINO[4]), M[pos] accumulated over the tiles in tile-group order per split, the splits added in split order, dW = G^T M G (G^T M first,
                           each entry a chain from 0).  The bias takes the kernel's route: position (1, 1) of D per tile, lane half h adds (tile h + tile 2 + h) of each group
                           to its chain, the halves meet, the splits in split order.
``nine_tap_plan`` / ``wino_plan`` / ``linear_plan``   Python restatements of plan(), ww_plan() and lw_plan() with what follows from them: S, trips, interior tiles, groups
                           per workgroup, wide or not, which finisher runs, bias workgroups, reduce blocks, workspace floats.  The references take their order from them,
                           tests/test_wgrad_ref.py proves from them what each case reaches and checks them against the library's host-only answers.
``check_wgrad``            a pure function of host tensors: util.derived for dW and for db against the reference of the form that ran, every guard float still NaN.

Tensors are NHWC ([B][H][W][C], tokens [N][C]) as the kernels read them; dW comes out OIHW as the kernels write it.  ``inputs`` / ``references`` build and cache the operands
and references of a row so that the CPU and the GPU test files share them and compute each once; callers never modify them.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from conv3x3_ref import WINO, _chain_threads, cdiv
from noisediff_amd import synth
from util import derived

F32, F64 = torch.float32, torch.float64
SLOPE = 0.2
PINS = (1, 2, 3)                        # nd_conv3x3_wgrad_form: nine taps, Winograd domain on four waves, on eight waves wherever cout % 64 == 0 (else four)

# (B, H, W, cin, cout): the smallest shapes that reach each code path -- tests/test_wgrad_ref.py::test_every_case_reaches_what_its_line_says proves each line from the plans
CASES = {
    "one": (1, 1, 1, 4, 4),                  # one pixel; a quad of a 64-block
    "tiny": (2, 3, 5, 4, 68),                # image smaller than a tile, odd sizes; cin = 4 (LSID conv1_1); one quad over a cout block
    "ragged": (2, 19, 37, 40, 20),           # ragged tiles in y and x; part blocks on both sides; S = 18 (reduce: two 8-batches + remainder)
    "interior": (1, 17, 33, 64, 64),         # the smallest shape with an interior tile (1 of 9)
    "second_trip": (2, 41, 130, 128, 192),   # nine taps: S = 85 < 108 tiles; 56 interior tiles; workgroups that walk a border and an interior tile in one loop
    "reduce_trip": (1, 3, 3, 384, 320),      # nine taps: more reduce blocks needed than the cap of 4096
    "w_one": (1, 4, 16, 16, 16),             # Winograd domain: one group; half-empty 32-blocks; S = 1, reduce only
    "w_sum": (3, 8, 48, 48, 112),            # S = 18; the sum + reduce finisher; 48 = 32 + 16; 112 = 3 x 32 + 16; a form-3 pin falls to four waves
    "w_wide": (2, 8, 32, 96, 64),            # eight waves under pin 3; sum + reduce
    "w_bias2": (1, 8, 32, 64, 400),          # the finish kernel with two bias workgroups (cout > 384)
    "w_uneven": (1, 28, 16, 256, 512),       # four waves: 7 groups over S = 2 (3 and 4 per workgroup); finish kernel
    "w8_uneven": (1, 28, 16, 512, 512),      # the same on eight waves
    "w_reduce_trip": (1, 4, 16, 1024, 1024), # wgrad_wino_reduce_kernel needs 4100 blocks against 4096; three bias workgroups' worth of cout; 151 MB workspace
}

# One call of an entry.  ``lk``: the first input channel that goes through LeakyReLU(0.2) before the sum (0: all, cin: none); ``c0``: channels of the first source (0: one
# source); x0 / x1 / y: (pixel stride, channel offset) of a source / of dY inside a wider tensor whose other channels are NaN, None: dense.
Row = collections.namedtuple("Row", "id entry shape lk c0 x0 x1 y", defaults=(0, None, None, None))
LinRow = collections.namedtuple("LinRow", "id entry shape x y", defaults=(None, None))          # shape = (N, cin, cout)


def _conv_rows():
    rows = []
    for case, shp in CASES.items():            # the plain entry is given the activated copy: one reference per case, and the leaky entry's twin
        rows += [Row(f"plain.{case}", "plain", shp, 0), Row(f"leaky.{case}", "leaky", shp, 0)]
    it = CASES["interior"]
    rows += [Row("plain.interior.slice", "plain", it, 0, 0, (96, 16), None, (80, 12)), Row("leaky.interior.slice", "leaky", it, 0, 0, (96, 16), None, (80, 12))]
    # beyond the table: the loop that mixes border and interior tiles on strided operands; the Winograd-domain forms' half-empty and whole blocks next to NaN gap channels
    rows += [Row("plain.second_trip.slice", "plain", CASES["second_trip"], 0, 0, (160, 16), None, (208, 12)),
             Row("plain.w_sum.slice", "plain", CASES["w_sum"], 0, 0, (64, 8), None, (128, 12)), Row("leaky.w_sum.slice", "leaky", CASES["w_sum"], 0, 0, (64, 8), None, (128, 12)),
             Row("plain.w_wide.slice", "plain", CASES["w_wide"], 0, 0, (112, 4), None, (80, 8))]
    B, H, W, _, cout = CASES["w_sum"]
    rows += [Row("cat.w_sum.32_32", "cat", (B, H, W, 64, cout), 64, 32, (48, 8), (40, 4), None),
             Row("cat.w_sum.96_32", "cat", (B, H, W, 128, cout), 128, 96, (112, 4), None, (128, 16)),
             Row("cat_leaky_second.w_sum.32_64", "cat_leaky_second", (B, H, W, 96, cout), 32, 32, (48, 8), (72, 4), None),
             # the twins of the two-source rows: the plain entry on the materialised concatenation
             Row("plain.cat.w_sum.32_32", "plain", (B, H, W, 64, cout), 64), Row("plain.cat.w_sum.96_32", "plain", (B, H, W, 128, cout), 128),
             Row("plain.cat_leaky_second.w_sum.32_64", "plain", (B, H, W, 96, cout), 32)]
    B, H, W, cin, cout = CASES["ragged"]
    rows += [Row("cat_leaky_second.ragged.36_4", "cat_leaky_second", (B, H, W, cin, cout), 36, 36, (44, 4), (8, 4), (24, 0))]
    return {r.id: r for r in rows}


def _lin_rows():
    rows = []
    for tag, shp in (("one", (1, 4, 4)), ("one_over", (129, 36, 20)), ("second_trip", (16641, 128, 128))):
        rows += [LinRow(f"linear.{tag}", "linear", shp), LinRow(f"linear_leaky.{tag}", "linear_leaky", shp)]
    rows += [LinRow("linear.slice", "linear", (300, 64, 64), (96, 16), (80, 12)), LinRow("linear_leaky.slice", "linear_leaky", (300, 64, 64), (96, 16), (80, 12))]
    return {r.id: r for r in rows}


ROWS, LIN_ROWS = _conv_rows(), _lin_rows()


# ---------------------------------------------------------------------------------------------------------------- the plans, restated

WG_TILE_W, WG_TILE_H, WG_CB, WG_TARGET, WG_REDUCE_CAP = 16, 8, 64, 512, 4096             # conv3x3_wgrad.hip: WG_TILE, TILE_H, CB, WGRAD_TARGET_WGS, the reduce grid's cap
WW_CB, W8_CO, WW_TARGET, WW_SUM_CAP, WW_REDUCE_CAP, WW_FINISH_MIN, WW_BIAS_WG = 32, 64, 256, 8192, 4096, 512, 384
LW_PK, LW_CB, LW_TARGET, LW_REDUCE_CAP = 128, 64, 512, 8192                               # linear_wgrad.hip


def nine_tap_plan(B, H, W, cin, cout):
    """plan() of conv3x3_wgrad.hip and what wgrad_run_t / wgrad_kernel / wgrad_reduce_kernel make of it."""
    n_co, n_ci = cdiv(cout, WG_CB), cdiv(cin, WG_CB)
    tiles_x, tiles_y = cdiv(W, WG_TILE_W), cdiv(H, WG_TILE_H)
    n_tiles = B * tiles_x * tiles_y
    S = min(max(WG_TARGET // (n_co * n_ci), 1), n_tiles)
    lists = [list(range(s, n_tiles, S)) for s in range(S)]

    def is_interior(tile):                   # `interior` of wgrad_kernel for a workgroup of whole channel blocks (fast_ok); tile = (b tiles_y + ty) tiles_x + tx
        tx, ty = tile % tiles_x, (tile // tiles_x) % tiles_y
        y0, x0 = ty * WG_TILE_H, tx * WG_TILE_W
        return y0 >= 1 and y0 + WG_TILE_H + 1 <= H and x0 >= 1 and x0 + WG_TILE_W + 1 <= W

    fast_blocks = (cout // WG_CB) * (cin // WG_CB)                  # (64 couts x 64 cins) blocks with co0 + 64 <= cout and ci0 + 64 <= cin
    interior = [t for t in range(n_tiles) if is_interior(t)] if fast_blocks else []
    mixed = [s for s, l in enumerate(lists) if 0 < sum(t in set(interior) for t in l) < len(l)]
    reduce_needed = cdiv(n_co * WG_CB * (9 * n_ci * WG_CB + 1), 256)
    return dict(n_co=n_co, n_ci=n_ci, tiles_x=tiles_x, tiles_y=tiles_y, n_tiles=n_tiles, S=S, lists=lists, trips=max(len(l) for l in lists),
                fast_blocks=fast_blocks, interior=interior, mixed_slots=mixed, reduce_needed=reduce_needed, reduce_trips=cdiv(reduce_needed, WG_REDUCE_CAP),
                workspace=S * n_co * WG_CB * (9 * n_ci * WG_CB + 1))


def wino_takes(pin, B, H, W, cin, cout):
    """ww_takes(): the Winograd-domain forms' shapes (the 1 GiB-per-sample limits of ww_runs are out of a test's reach)."""
    return pin != 1 and H % 4 == 0 and W % 16 == 0 and cin % 16 == 0 and cout % 16 == 0 and B * H * W < (1 << 30)


def wino_plan(pin, B, H, W, cin, cout):
    """ww_plan() under a pin of the form (0: by the shape) and the finisher wgrad_run_t launches behind it; None where the nine-tap form runs."""
    if not wino_takes(pin, B, H, W, cin, cout):
        return None
    wide = pin != 2 and cout % W8_CO == 0 and cin % WW_CB == 0 and (pin == 3 or B * (H // 4) * (W // 16) * (cin // WW_CB) * (cout // WW_CB) >= 20000)
    n_co, n_ci = (cout // W8_CO if wide else cdiv(cout, WW_CB)), cdiv(cin, WW_CB)
    coP, ciP = n_co * (W8_CO if wide else WW_CB), n_ci * WW_CB
    gx, gy = W // 16, H // 4
    n_groups, blocks = B * gx * gy, n_co * n_ci
    best, S = -1, 1
    for c in range(1, min(n_groups, 4 * WW_TARGET) + 1):
        rounds = cdiv(blocks * c, WW_TARGET)
        cost = rounds * (cdiv(n_groups, c) + 14)
        if best < 0 or cost < best:
            best, S = cost, c
        if rounds > 8:
            break
    ranges = [(s * n_groups // S, (s + 1) * n_groups // S) for s in range(S)]
    n_main = cout * (ciP // 32)
    finisher = "reduce" if S == 1 else "finish" if n_main >= WW_FINISH_MIN else "sum+reduce"
    return dict(wide=wide, form=3 if wide else 2, n_co=n_co, n_ci=n_ci, coP=coP, ciP=ciP, gx=gx, gy=gy, n_groups=n_groups, S=S, ranges=ranges,
                groups_per_wg=sorted({hi - lo for lo, hi in ranges}), finisher=finisher, bias_wgs=cdiv(cout, WW_BIAS_WG) if finisher == "finish" else 0,
                finish_wgs=n_main if finisher == "finish" else 0, reduce_needed=cdiv(cout * (cin + 1), 256) if finisher != "finish" else 0,
                sum_needed=cdiv(36 * coP * ciP + coP, 256) if finisher == "sum+reduce" else 0, workspace=S * coP * (36 * ciP + 1))


def form_that_runs(pin, B, H, W, cin, cout):
    """nd_conv3x3_wgrad_plan restated: 1 = nine taps, 2 = Winograd domain on four waves, 3 = on eight."""
    p = wino_plan(pin, B, H, W, cin, cout)
    return p["form"] if p else 1


def workspace_floats(pin, B, H, W, cin, cout):
    """nd_conv3x3_wgrad_workspace_floats restated: the nine-tap layout, or the Winograd-domain one where it is larger."""
    p = wino_plan(pin, B, H, W, cin, cout)
    return max(nine_tap_plan(B, H, W, cin, cout)["workspace"], p["workspace"] if p else 0)


def linear_plan(N, cin, cout):
    """lw_plan() of linear_wgrad.hip."""
    n_co, n_ci, chunks = cdiv(cout, LW_CB), cdiv(cin, LW_CB), cdiv(N, LW_PK)
    S = min(max(LW_TARGET // (n_co * n_ci), 1), chunks)
    lists = [list(range(s, chunks, S)) for s in range(S)]
    return dict(n_co=n_co, n_ci=n_ci, chunks=chunks, S=S, lists=lists, trips=max(len(l) for l in lists), workspace=S * n_co * LW_CB * (n_ci * LW_CB + 1),
                reduce_needed=cdiv(n_co * LW_CB * (n_ci * LW_CB + 1), 32))


# ---------------------------------------------------------------------------------------------------------------- operands

def leaky(x):
    """The activated copy as the kernels form it on load: max(x, 0.2 x) in the dtype of ``x``."""
    return torch.maximum(x, x * SLOPE)


@functools.lru_cache(maxsize=None)
def _draw(kind, shape):
    tag = "x".join(map(str, shape))
    lo, hi = (-1.5, 1.0) if kind == "x" else (-1.0, 1.0)               # x over (-1.5, 1.0): both branches of LeakyReLU occur
    return synth.uniform(29, f"wg.{kind}.{tag}", shape, lo, hi)


def inputs(row):
    """(x raw, x as the sum sees it, dY) of a row, fp32 NHWC / tokens.  Rows of one shape share their draws: a twin sees the same numbers."""
    if isinstance(row, LinRow):
        N, cin, cout = row.shape
        x, dy = _draw("x", (N, cin)), _draw("dy", (N, cout))
        return x, (leaky(x) if row.entry == "linear_leaky" else x), dy
    B, H, W, cin, cout = row.shape
    x, dy = _draw("x", (B, H, W, cin)), _draw("dy", (B, H, W, cout))
    return x, activated(x, row.lk), dy


def activated(x, lk):
    """Channels lk .. of ``x`` through LeakyReLU(0.2), in the dtype of ``x``."""
    return torch.cat((x[..., :lk], leaky(x[..., lk:])), -1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- float64

def ref64(xa, dy):
    """(dW [cout][cin][3][3], db [cout]) in float64 of the activated, concatenated NHWC input ``xa`` and NHWC ``dy``; tokens [N][C]: (dy.T @ xa, db)."""
    xa, dy = xa.double(), dy.double()
    if xa.dim() == 2:
        return dy.T @ xa, dy.sum(0)
    cin, cout = xa.shape[-1], dy.shape[-1]
    dw = torch.nn.grad.conv2d_weight(xa.permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.permute(0, 3, 1, 2), padding=1)
    return dw.contiguous(), dy.sum((0, 1, 2))


# ---------------------------------------------------------------------------------------------------------------- fp32 chains

def _chain(dyT, xT, idx, lists):
    """acc[s][t](co, ci) += dyT[tile][p][co] * xT[tile][idx[p][t]][ci], sequentially over the tiles of ``lists[s]`` and the pixels p of a tile: one multiply-add chain
    per element, all slots at once.  dyT [tiles][P][cout], xT [tiles][Px][cin], idx [P][taps].  A slot with fewer tiles than the longest adds zeros."""
    S, trips, T = len(lists), max(len(l) for l in lists), dyT.shape[0]
    dyT, xT = torch.cat((dyT, torch.zeros_like(dyT[:1]))), torch.cat((xT, torch.zeros_like(xT[:1])))
    order = torch.tensor([[l[t] if t < len(l) else T for l in lists] for t in range(trips)])
    acc = torch.zeros(S, idx.shape[1], dyT.shape[2], xT.shape[2], dtype=dyT.dtype)
    with _chain_threads(acc):
        for t in range(trips):
            d, xx = dyT[order[t]], xT[order[t]]
            for p in range(d.shape[1]):
                if bool(d[:, p].any()):                                  # (a pixel outside the image in every slot: the kernel adds 0 x)
                    acc.addcmul_(d[:, p, None, :, None], xx[:, idx[p]][:, :, None, :])
    return acc


def _quarter_bias(dyT, lists):
    """wsb [S][cout]: thread (cout, quarter q) chains the pixels 32 q .. 32 q + 31 of every tile of its slot (carried across the tiles), then ((q0 + q1) + q2) + q3."""
    S, trips, T = len(lists), max(len(l) for l in lists), dyT.shape[0]
    dq = torch.cat((dyT, torch.zeros_like(dyT[:1]))).reshape(T + 1, 4, dyT.shape[1] // 4, dyT.shape[2])
    bs = torch.zeros(S, 4, dyT.shape[2], dtype=dyT.dtype)
    for t in range(trips):
        d = dq[torch.tensor([l[t] if t < len(l) else T for l in lists])]
        for r in range(d.shape[2]):
            bs += d[:, :, r]
    return ((bs[:, 0] + bs[:, 1]) + bs[:, 2]) + bs[:, 3]


def add_in_order(parts, order=None):
    """The partials [S][..] added one by one from 0 in ``order`` (default: slot order) -- wgrad_reduce_kernel's loop, wgrad_wino_sum_kernel's and sum_splits'."""
    total = torch.zeros_like(parts[0])
    for s in (range(parts.shape[0]) if order is None else order):
        total = total + parts[s]
    return total


def add_in_stripes(parts):
    """linear_wgrad_reduce_kernel: stripe k adds the slots k, k + 8, .. in order, the eight stripes then meet in stripe order."""
    total = None
    for k in range(8):
        stripe = add_in_order(parts[k::8]) if k < parts.shape[0] else torch.zeros_like(parts[0])
        total = stripe if total is None else total + stripe
    return total


def nine_tap_tiles(xa, dy):
    """The operands as wgrad_kernel stages them: dY tiles [tiles][128 pixels][cout] and X halos [tiles][10 x 18 pixels][cin], zeros outside the image, and the halo index of
    (pixel, tap).  Tile = (b tiles_y + ty) tiles_x + tx."""
    B, H, W, cin = xa.shape
    cout = dy.shape[-1]
    ty, tx = cdiv(H, WG_TILE_H), cdiv(W, WG_TILE_W)
    Hp, Wp = ty * WG_TILE_H, tx * WG_TILE_W
    dyT = F.pad(dy, (0, 0, 0, Wp - W, 0, Hp - H)).reshape(B, ty, WG_TILE_H, tx, WG_TILE_W, cout).permute(0, 1, 3, 2, 4, 5).reshape(B * ty * tx, WG_TILE_H * WG_TILE_W, cout)
    xp = F.pad(xa, (0, 0, 1, Wp - W + 1, 1, Hp - H + 1))
    xT = xp.unfold(1, WG_TILE_H + 2, WG_TILE_H).unfold(2, WG_TILE_W + 2, WG_TILE_W).permute(0, 1, 2, 4, 5, 3).reshape(B * ty * tx, (WG_TILE_H + 2) * (WG_TILE_W + 2), cin)
    p, t = torch.arange(WG_TILE_H * WG_TILE_W)[:, None], torch.arange(9)[None, :]
    idx = (p // WG_TILE_W + t // 3) * (WG_TILE_W + 2) + p % WG_TILE_W + t % 3
    return dyT.contiguous(), xT.contiguous(), idx


def nine_tap_partials(xa, dy, lists=None):
    """(ws [S][9][cout][cin], wsb [S][cout]) as wgrad_kernel leaves them; ``lists``: the tiles of every slot (default: the plan's)."""
    B, H, W, cin = xa.shape
    dyT, xT, idx = nine_tap_tiles(xa, dy)
    lists = lists or nine_tap_plan(B, H, W, cin, dy.shape[-1])["lists"]
    return _chain(dyT, xT, idx, lists), _quarter_bias(dyT, lists)


def taps_to_oihw(m):
    return m.permute(1, 2, 0).reshape(m.shape[1], m.shape[2], 3, 3).contiguous()


def ref32_nine_tap(xa, dy, lists=None, order=None):
    """(dW OIHW, db) in fp32 in the nine-tap kernel's order.  ``order``: the slots added in another order (admit tests)."""
    ws, wsb = nine_tap_partials(xa.float(), dy.float(), lists)
    return taps_to_oihw(add_in_order(ws, order)), add_in_order(wsb, order)


def ref32_linear(xa, dy):
    """(dW [cout][cin], db) in fp32 in linear_wgrad_kernel's order."""
    N, cin = xa.shape
    plan = linear_plan(N, cin, dy.shape[-1])
    pad = plan["chunks"] * LW_PK - N
    dyT, xT = F.pad(dy.float(), (0, 0, 0, pad)).reshape(plan["chunks"], LW_PK, -1), F.pad(xa.float(), (0, 0, 0, pad)).reshape(plan["chunks"], LW_PK, cin)
    ws = _chain(dyT, xT, torch.arange(LW_PK)[:, None], plan["lists"])
    return add_in_stripes(ws[:, 0]), add_in_stripes(_quarter_bias(dyT, plan["lists"]))


def wino_matrices(dtype, absolute=False):
    BT, G, AT = (torch.tensor(t, dtype=dtype) for t in WINO[4])
    return (BT.abs(), G.abs(), AT.abs()) if absolute else (BT, G, AT)


def wino_partials(xa, dy, plan, mats=None, ranges=None):
    """(ws [S][36][cout][cin], wsb [S][cout]) as the Winograd-domain kernels leave them, in the dtype of ``xa``.  ``ranges``: the tile groups [lo, hi) of every split
    (default: the plan's); ``mats``: (B^T, G, A^T) (default: conv3x3_ref.WINO[4] in that dtype)."""
    BT, G, AT = mats or wino_matrices(xa.dtype)
    B, H, W, cin = xa.shape
    cout = dy.shape[-1]
    d = F.pad(xa, (0, 0, 1, 1, 1, 1)).unfold(1, 6, 4).unfold(2, 6, 4)                               # [B][H / 4][W / 4][cin][6][6]
    V = torch.einsum("byxciq,jq->byxcij", torch.einsum("ip,byxcpq->byxciq", BT, d), BT)             # rows (ww_bt3 down a column), then columns (ww_bt6)
    y = dy.unfold(1, 4, 4).unfold(2, 4, 4)                                                          # [B][H / 4][W / 4][cout][4][4]
    D = torch.einsum("byxciq,qj->byxcij", torch.einsum("pi,byxcpq->byxciq", AT, y), AT)             # A = (A^T)^T: 6 x 4
    Vt = V.reshape(-1, cin, 36).permute(0, 2, 1).contiguous()                                       # tile = (b H / 4 + ty) W / 4 + tx: four in a row are one group
    Dt = D.reshape(-1, cout, 36).permute(0, 2, 1).contiguous()
    ranges = ranges or plan["ranges"]
    lists = [list(range(4 * lo, 4 * hi)) for lo, hi in ranges]                                      # K = two tiles per MFMA, the lane halves in order: tile order
    S, steps, T = len(lists), max(len(l) for l in lists), Dt.shape[0]
    Dz, Vz = torch.cat((Dt, torch.zeros_like(Dt[:1]))), torch.cat((Vt, torch.zeros_like(Vt[:1])))
    ws = torch.zeros(S, 36, cout, cin, dtype=xa.dtype)
    bs = torch.zeros(S, 2, cout, dtype=xa.dtype)
    with _chain_threads(ws):
        for t in range(steps):
            o = torch.tensor([l[t] if t < len(l) else T for l in lists])
            ws.addcmul_(Dz[o][:, :, :, None], Vz[o][:, :, None, :])
            if t % 4 == 0:                                                                           # a group: lane half h holds D[7] of the tiles h and 2 + h
                g = torch.stack([Dz[torch.tensor([l[t + k] if t + k < len(l) else T for l in lists])][:, 7] for k in range(4)], 1)      # [S][4][cout]
                bs += g[:, 0:2] + g[:, 2:4]
    return ws, bs[:, 0] + bs[:, 1]


def wino_back(M, G):
    """dW OIHW = G^T M G of M [36][cout][cin]: R = G^T M, each entry a chain over i from 0, then R G over jj (wgrad_wino_reduce_kernel, wgrad_wino_finish_kernel)."""
    g = G.tolist()
    R = [[None] * 6 for _ in range(3)]
    for r in range(3):
        for jj in range(6):
            v = torch.zeros_like(M[0])
            for i in range(6):
                if g[i][r]:
                    v = v + g[i][r] * M[i * 6 + jj]
            R[r][jj] = v
    out = torch.zeros(M.shape[1], M.shape[2], 3, 3, dtype=M.dtype)
    for r in range(3):
        for c in range(3):
            v = torch.zeros_like(M[0])
            for jj in range(6):
                if g[jj][c]:
                    v = v + R[r][jj] * g[jj][c]
            out[:, :, r, c] = v
    return out


def ref32_winograd_domain(xa, dy, plan, dtype=F32, order=None, ranges=None, absolute=False):
    """(dW OIHW, db) by the Winograd-domain formula in ``dtype`` in the kernels' order, for a ``plan`` of wino_plan.  float64: the formula itself (exact up to rounding);
    ``absolute``: every matrix and operand by its absolute value -- the sum of the magnitudes of all terms, which scales an a-priori rounding bound."""
    xa, dy = xa.to(dtype), dy.to(dtype)
    mats = wino_matrices(dtype, absolute)
    ws, wsb = wino_partials(xa.abs() if absolute else xa, dy.abs() if absolute else dy, plan, mats, ranges)
    return wino_back(add_in_order(ws, order), mats[1]), add_in_order(wsb, order)


# ---------------------------------------------------------------------------------------------------------------- references of a row, cached

@functools.lru_cache(maxsize=16)
def _conv_references(shape, lk, form, wide_pin, split_c0):
    B, H, W, cin, cout = shape
    x = _draw("x", (B, H, W, cin))
    xa, dy = activated(x, lk), _draw("dy", (B, H, W, cout))
    dw64, db64 = ref64(xa, dy)
    if form == 1 and split_c0:               # nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32's nine-tap route: one gradient per source into its columns, the bias with the first
        a, b = ref32_nine_tap(xa[..., :split_c0].contiguous(), dy), ref32_nine_tap(xa[..., split_c0:].contiguous(), dy)
        dw32, db32 = torch.cat((a[0], b[0]), 1), a[1]
    elif form == 1:
        dw32, db32 = ref32_nine_tap(xa, dy)
    else:
        dw32, db32 = ref32_winograd_domain(xa, dy, wino_plan(wide_pin, B, H, W, cin, cout))
    return dict(dw64=dw64, db64=db64, dw32=dw32, db32=db32)


def references(row, form):
    """{dw64, db64, dw32, db32} of a row for the form that ran (1 / 2 / 3; a linear row has one).  Cached: computed once, shared, never modified by a caller."""
    if isinstance(row, LinRow):
        return _lin_references(row.shape, row.entry == "linear_leaky")
    two_gradients = row.entry == "cat_leaky_second" and form == 1
    return _conv_references(row.shape, row.lk, form, form, row.c0 if two_gradients else 0)


@functools.lru_cache(maxsize=16)
def _lin_references(shape, lk):
    N, cin, cout = shape
    x, dy = _draw("x", (N, cin)), _draw("dy", (N, cout))
    xa = leaky(x) if lk else x
    dw64, db64 = ref64(xa, dy)
    dw32, db32 = ref32_linear(xa, dy)
    return dict(dw64=dw64, db64=db64, dw32=dw32, db32=db32)


# ---------------------------------------------------------------------------------------------------------------- the checker

def check_wgrad(got_dw, got_db, refs, guards, what=""):
    """``got_dw`` / ``got_db`` (None: no bias gradient was asked for): host copies of what the entry wrote; ``refs``: ``references`` of the form that ran; ``guards``:
    {name: host tensor of the floats around a buffer the entry was given}.  Bound: util.derived for dW and for db; every guard float still NaN.  No tolerance of its own."""
    for name, g in guards.items():
        bad = int((~torch.isnan(g)).sum())
        assert bad == 0, f"{what}: {bad} guard floats of {name} were written"
    derived(got_dw, refs["dw64"], refs["dw32"], what + " dW")
    if got_db is not None:
        derived(got_db, refs["db64"], refs["db32"], what + " db")
    return True
