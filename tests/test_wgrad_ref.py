"""tests/wgrad_ref.py on the CPU: the references agree with float64 and with each other, the restated plans say that every case reaches what its table line claims and
agree with the library's host-only answers, and check_wgrad admits correct fp32 evaluations and rejects subtly wrong ones.

A-priori bounds (nothing here is taken from what a kernel or a reference achieves): an fp32 chain of n multiply-adds is within n 2^-24 of the sum of the magnitudes of its
terms (Higham, gamma_n; first order), element by element.  For the nine-tap and the linear chains that sum is ref64 of (|x|, |dY|) and n the chain's length (pixels per slot +
slots); for the Winograd-domain formula it is the same formula evaluated in float64 with every matrix and operand replaced by its absolute value, and n the tiles per split +
the splits + 40 for the three transforms (B^T d B and A dY A^T: at most 2 x 5 additions each; G^T M G: 2 x 6).  In float64 the Winograd-domain formula IS the sum.
The library questions need the built library and no GPU, as the library tests of tests/test_host.py.
"""
import pytest
import torch

import wgrad_ref as R
from noisediff_amd import _lib as L

U32 = 2.0 ** -24
FORMS_OF = {case: sorted({R.form_that_runs(pin, *shp) for pin in R.PINS}) for case, shp in R.CASES.items()}


def operands(row):
    x, xa, dy = R.inputs(row)
    return xa, dy


def magnitude_sum(row, form):
    """(dW, db) with every term replaced by its magnitude, float64, by the formula of ``form``."""
    xa, dy = operands(row)
    if form == 1 or isinstance(row, R.LinRow):
        return R.ref64(xa.abs(), dy.abs())
    return R.ref32_winograd_domain(xa, dy, R.wino_plan(form, *row.shape), dtype=torch.float64, absolute=True)


def chain_lengths(row, form):
    """(n of a dW chain, n of a db chain): multiply-adds (additions) that meet in one output element."""
    if isinstance(row, R.LinRow):
        p = R.linear_plan(*row.shape)
        return p["trips"] * R.LW_PK + R.cdiv(p["S"], 8) + 8, p["trips"] * R.LW_PK // 4 + 4 + R.cdiv(p["S"], 8) + 8
    if form == 1:
        p = R.nine_tap_plan(*row.shape)
        return p["trips"] * 128 + p["S"], p["trips"] * 32 + 4 + p["S"]
    p = R.wino_plan(form, *row.shape)
    tiles = 4 * max(p["groups_per_wg"])
    return tiles + p["S"] + 40, tiles + p["S"] + 10


def within(got, ref64, mag, n, what):
    excess = float(((got.double() - ref64).abs() - n * U32 * mag).max())
    assert excess <= 0, f"{what}: an element is {excess:.3e} beyond {n} x 2^-24 x the sum of its terms' magnitudes"


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_fp32_references_agree_with_float64_and_with_each_other(case):
    row = R.ROWS["plain." + case]
    refs = {form: R.references(row, form) for form in FORMS_OF[case]}
    bounds = {}
    for form, r in refs.items():
        (mw, mb), (nw, nb) = magnitude_sum(row, form), chain_lengths(row, form)
        within(r["dw32"], r["dw64"], mw, nw, f"{case} form {form} dW")
        within(r["db32"], r["db64"], mb, nb, f"{case} form {form} db")
        bounds[form] = nw * U32 * mw
    for form in refs:                        # two independent restatements of one sum
        if form != 1:
            diff = (refs[form]["dw32"].double() - refs[1]["dw32"].double()).abs()
            assert bool((diff <= bounds[form] + bounds[1]).all()), f"{case}: the nine-tap and the form-{form} reference differ by {float(diff.max()):.3e}"


@pytest.mark.parametrize("id", list(R.LIN_ROWS))
def test_the_linear_reference_agrees_with_float64(id):
    row = R.LIN_ROWS[id]
    r = R.references(row, 0)
    (mw, mb), (nw, nb) = magnitude_sum(row, 0), chain_lengths(row, 0)
    within(r["dw32"], r["dw64"], mw, nw, id + " dW")
    within(r["db32"], r["db64"], mb, nb, id + " db")


@pytest.mark.parametrize("case", ["w_one", "w_sum", "w_wide"])
def test_the_winograd_domain_formula_in_float64_is_the_sum(case):
    row = R.ROWS["plain." + case]
    xa, dy = operands(row)
    dw64, db64 = R.ref64(xa, dy)
    for pin in (2, 3):
        dw, db = R.ref32_winograd_domain(xa, dy, R.wino_plan(pin, *row.shape), dtype=torch.float64)
        assert float((dw - dw64).abs().max()) < 2.0 ** -40 * float(dw64.abs().max()) and float((db - db64).abs().max()) < 2.0 ** -40 * float(db64.abs().max())


# ---------------------------------------------------------------------------------------------------------------- what each case reaches

def test_every_case_reaches_what_its_line_says():
    nt = {case: R.nine_tap_plan(*shp) for case, shp in R.CASES.items()}
    wp = {(case, pin): R.wino_plan(pin, *shp) for case, shp in R.CASES.items() for pin in R.PINS}
    for case in ("one", "tiny", "ragged", "interior", "second_trip", "reduce_trip"):          # nine taps under every pin
        assert FORMS_OF[case] == [1], case
    for case in ("w_one", "w_sum", "w_wide", "w_bias2", "w_uneven", "w8_uneven", "w_reduce_trip"):
        assert wp[case, 1] is None and wp[case, 2]["form"] == 2, case

    p = nt["one"]                            # one pixel; a quad of a 64-block
    assert (p["n_tiles"], p["S"], p["trips"], p["n_co"], p["n_ci"], p["fast_blocks"]) == (1, 1, 1, 1, 1, 0)
    p = nt["tiny"]                           # smaller than a tile; one quad over a cout block
    assert (p["tiles_x"], p["tiles_y"], p["n_co"], p["n_ci"], p["S"]) == (1, 1, 2, 1, 2) and R.CASES["tiny"][4] == 64 + 4
    p = nt["ragged"]                         # ragged in y and x, part blocks, S = 18: wgrad_reduce_kernel takes two batches of eight slots and two single ones
    B, H, W, cin, cout = R.CASES["ragged"]
    assert H % 8 and W % 16 and cin % 64 and cout % 64 and (p["S"], p["trips"]) == (18, 1) and p["S"] // 8 == 2 and p["S"] % 8 == 2 and not p["interior"]
    p = nt["interior"]                       # one interior tile of nine; one row or one column less and there is none
    B, H, W, cin, cout = R.CASES["interior"]
    assert (p["n_tiles"], len(p["interior"]), p["fast_blocks"], p["trips"]) == (9, 1, 1, 1)
    assert not R.nine_tap_plan(B, H - 1, W, cin, cout)["interior"] and not R.nine_tap_plan(B, H, W - 1, cin, cout)["interior"]
    p = nt["second_trip"]                    # the tile loop's second trip; interior and border tiles in one workgroup's loop; whole blocks only
    B, H, W, cin, cout = R.CASES["second_trip"]
    assert (p["S"], p["n_tiles"], p["trips"], len(p["interior"])) == (85, 108, 2, 56) and p["fast_blocks"] == p["n_co"] * p["n_ci"] == 6
    assert len(p["mixed_slots"]) >= 1 and sum(len(l) == 2 for l in p["lists"]) == 108 - 85
    both_interior = [s for s, l in enumerate(p["lists"]) if len(l) == 2 and all(t in p["interior"] for t in l)]
    assert both_interior, "no workgroup stages two interior tiles in a row"
    p = nt["reduce_trip"]                    # wgrad_reduce_kernel's grid-stride loop
    assert p["reduce_needed"] > R.WG_REDUCE_CAP and p["reduce_trips"] == 2 and p["S"] == 1

    p = wp["w_one", 2]                       # one group, half-empty blocks, no split: the reduce kernel alone
    assert (p["n_groups"], p["S"], p["finisher"], p["coP"], p["ciP"]) == (1, 1, "reduce", 32, 32) and wp["w_one", 3]["form"] == 2
    p = wp["w_sum", 2]
    assert (p["S"], p["finisher"], p["ciP"], p["coP"]) == (18, "sum+reduce", 64, 128) and R.CASES["w_sum"][3:] == (32 + 16, 3 * 32 + 16)
    assert wp["w_sum", 3]["form"] == 2       # cout % 64 != 0: a form-3 pin falls to four waves
    p = wp["w_wide", 3]
    assert p["form"] == 3 and p["finisher"] == "sum+reduce" and p["S"] > 1 and wp["w_wide", 2]["form"] == 2
    p = wp["w_bias2", 2]
    assert (p["finisher"], p["bias_wgs"]) == ("finish", 2) and p["S"] > 1 and wp["w_bias2", 3]["form"] == 2
    p = wp["w_uneven", 2]                    # k and k + 1 groups per workgroup, k >= 3: the two-phase loop's body and both of its exits
    assert (p["n_groups"], p["S"], p["groups_per_wg"], p["finisher"], p["bias_wgs"]) == (7, 2, [3, 4], "finish", 2)
    p = wp["w8_uneven", 3]
    assert (p["form"], p["n_groups"], p["S"], p["groups_per_wg"], p["finisher"]) == (3, 7, 2, [3, 4], "finish")
    for pin in (2, 3):                       # wgrad_wino_reduce_kernel's grid-stride loop, on both forms
        p = wp["w_reduce_trip", pin]
        assert p["form"] == pin and p["finisher"] == "reduce" and p["reduce_needed"] == 4100 > R.WW_REDUCE_CAP and R.cdiv(R.CASES["w_reduce_trip"][4], R.WW_BIAS_WG) == 3
        assert 150e6 < 4 * p["workspace"] < 152e6

    lp = {id: R.linear_plan(*row.shape) for id, row in R.LIN_ROWS.items()}
    assert (lp["linear.one_over"]["chunks"], lp["linear.one_over"]["S"]) == (2, 2) and R.LIN_ROWS["linear.one_over"].shape[0] == R.LW_PK + 1
    p = lp["linear.second_trip"]
    assert (p["S"], p["chunks"], p["trips"]) == (128, 131, 2) and p["S"] > 64          # (the reduce kernel's 64-slot batches and its tail)

    # the two-source rows: which route each takes under each pin
    for id, forms in (("cat.w_sum.32_32", [None, 2, 2]), ("cat.w_sum.96_32", [None, 2, 2]), ("cat_leaky_second.w_sum.32_64", [1, 2, 2]), ("cat_leaky_second.ragged.36_4", [1, 1, 1])):
        row = R.ROWS[id]
        B, H, W, cin, cout = row.shape
        c0, c1 = row.c0, cin - row.c0
        got = []
        for pin in R.PINS:
            cat_takes = c0 % 32 == 0 and c1 % 32 == 0 and R.wino_takes(pin, B, H, W, cin, cout)
            got.append(R.form_that_runs(pin, B, H, W, cin, cout) if cat_takes else None if row.entry == "cat" else 1)
        assert got == forms, (id, got)          # (cout = 112: a form-3 pin falls to four waves)


# ---------------------------------------------------------------------------------------------------------------- the plans against the library

EXTRA_SHAPES = [(2, 48, 32, 64, 128), (4, 64, 64, 32, 32), (1, 16, 16, 512, 256), (3, 40, 48, 96, 64), (3, 64, 256, 32, 64), (2, 8, 32, 80, 112), (1, 256, 256, 32, 32),
                (79, 64, 64, 64, 64), (78, 64, 64, 64, 64), (4, 128, 128, 192, 128), (1, 9, 11, 32, 64), (2, 16, 32, 62, 64), (16, 32, 32, 384, 512)]


def test_the_restated_plans_equal_the_librarys_answers():
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(-1)
    try:
        shapes = list(R.CASES.values()) + [r.shape for r in R.ROWS.values()] + EXTRA_SHAPES
        for pin in (0, 1, 2, 3):
            lib.nd_conv3x3_wgrad_form(pin)
            for shp in shapes:
                if shp[3] % 4 or shp[4] % 4:                           # (62 channels: the entry refuses; the question answers 1)
                    assert lib.nd_conv3x3_wgrad_plan(*shp) == 1
                    continue
                nine, wp = R.nine_tap_plan(*shp), R.wino_plan(pin, *shp)
                assert nine["workspace"] == nine["S"] * nine["n_co"] * 64 * (9 * nine["n_ci"] * 64 + 1)
                want = nine["workspace"] if pin == 1 or wp is None else max(nine["workspace"], wp["S"] * wp["coP"] * (36 * wp["ciP"] + 1))
                assert int(lib.nd_conv3x3_wgrad_workspace_floats(*shp)) == want == R.workspace_floats(pin, *shp), (pin, shp)
                assert lib.nd_conv3x3_wgrad_plan(*shp) == R.form_that_runs(pin, *shp), (pin, shp)
    finally:
        lib.nd_conv3x3_wgrad_form(was)
    for shp in [r.shape for r in R.LIN_ROWS.values()] + [(4096 * 16, 64, 64), (1000, 1024, 256), (127, 4, 132)]:
        assert int(lib.nd_linear_wgrad_workspace_floats(*shp)) == R.linear_plan(*shp)["workspace"], shp


# ---------------------------------------------------------------------------------------------------------------- check_wgrad: admits and rejects

NAN_GUARD = {"dw": torch.full((128,), float("nan")), "db": torch.full((128,), float("nan")), "workspace": torch.full((128,), float("nan"))}
MUTATED = [("plain.ragged", 1), ("plain.w_sum", 2)]


def evaluate(row, form, xa, dy, slots=None, order=None):
    """(dW, db) in fp32 by the reference of ``form``; ``slots``: the tiles of every nine-tap slot / the tile groups [lo, hi) of every Winograd-domain split."""
    if form == 1:
        return R.ref32_nine_tap(xa, dy, slots, order)
    return R.ref32_winograd_domain(xa, dy, R.wino_plan(form, *row.shape), order=order, ranges=slots)


def slots_of(row, form):
    return [list(l) for l in R.nine_tap_plan(*row.shape)["lists"]] if form == 1 else list(R.wino_plan(form, *row.shape)["ranges"])


def rejected(*a):
    with pytest.raises(AssertionError):
        R.check_wgrad(*a)


@pytest.mark.parametrize("id,form", MUTATED)
def test_correct_evaluations_are_admitted(id, form):
    row = R.ROWS[id]
    refs = R.references(row, form)
    xa, dy = operands(row)
    R.check_wgrad(refs["dw32"].clone(), refs["db32"].clone(), refs, NAN_GUARD, id)
    R.check_wgrad(refs["dw32"].clone(), None, refs, NAN_GUARD, id)
    S = len(slots_of(row, form))
    dw, db = evaluate(row, form, xa, dy, order=range(S - 1, -1, -1))       # the slots added in reverse order: another legitimate order
    assert not torch.equal(dw, refs["dw32"])
    R.check_wgrad(dw, db, refs, NAN_GUARD, id + " reversed")


@pytest.mark.parametrize("id,form", MUTATED)
def test_single_source_mutations_are_rejected(id, form):
    row = R.ROWS[id]
    refs = R.references(row, form)
    xa, dy = operands(row)
    good_w, good_b = refs["dw32"], refs["db32"]

    m = good_w.clone()                                                # one border term kept: replicate padding above pixel (0, 0) of sample 0 (tap (0, 1)) instead of zero
    m[:, :, 0, 1] += torch.outer(dy[0, 0, 0], xa[0, 0, 0])
    rejected(m, good_b, refs, NAN_GUARD)

    rejected(good_w.transpose(2, 3).contiguous(), good_b, refs, NAN_GUARD)          # taps transposed: r and s swapped

    slots = slots_of(row, form)                                       # one split slot left out
    slots[len(slots) // 2] = [] if form == 1 else (slots[len(slots) // 2][0],) * 2
    rejected(*evaluate(row, form, xa, dy, slots), refs, NAN_GUARD)

    slots = slots_of(row, form)                                       # one tile (tile group) counted twice
    if form == 1:
        slots[1] = slots[1] + slots[1][:1]
    else:
        slots.append(slots[1])
    rejected(*evaluate(row, form, xa, dy, slots), refs, NAN_GUARD)

    rejected(*evaluate(row, form, xa.bfloat16().float(), dy), refs, NAN_GUARD)      # x rounded to bfloat16 before the sum

    m = good_b - (dy[0, 2:4, :16].sum((0, 1)) if form == 1 else dy[0, :4, :4].sum((0, 1)))       # db over one pixel quarter of one tile (one 4 x 4 tile) fewer
    rejected(good_w, m, refs, NAN_GUARD)

    for name in NAN_GUARD:                                            # a guard float overwritten
        g = {k: v.clone() for k, v in NAN_GUARD.items()}
        g[name][64 if name == "dw" else 63] = 0.0
        rejected(good_w, good_b, refs, g)

    m = good_w.clone()                                                # (and an element never written)
    m[-1, -1, 2, 2] = float("nan")
    rejected(m, good_b, refs, NAN_GUARD)


@pytest.mark.parametrize("id,form", [("cat_leaky_second.ragged.36_4", 1), ("cat_leaky_second.w_sum.32_64", 2)])
def test_two_source_mutations_are_rejected(id, form):
    row = R.ROWS[id]
    refs = R.references(row, form)
    x, xa, dy = R.inputs(row)
    c0, cin = row.c0, row.shape[3]
    R.check_wgrad(refs["dw32"].clone(), refs["db32"].clone(), refs, NAN_GUARD, id)

    wrong = torch.cat((R.leaky(x[..., :c0]), x[..., c0:]), -1)       # LeakyReLU applied to the wrong source
    if form == 1:
        a, b = R.ref32_nine_tap(wrong[..., :c0].contiguous(), dy), R.ref32_nine_tap(wrong[..., c0:].contiguous(), dy)
        rejected(torch.cat((a[0], b[0]), 1), a[1], refs, NAN_GUARD)
    else:
        rejected(*evaluate(row, form, wrong, dy), refs, NAN_GUARD)

    m = refs["dw32"].clone()                                          # the second source's columns written at dw_ci0 = 0 (their own columns as they should be)
    m[:, : cin - c0] = refs["dw32"][:, c0:]
    rejected(m, refs["db32"], refs, NAN_GUARD)

    if form == 1:                                                     # the bias gradient taken with the second gradient as well: its partials added twice
        rejected(refs["dw32"], refs["db32"] * 2, refs, NAN_GUARD)


@pytest.mark.parametrize("id", ["linear.one_over", "linear_leaky.second_trip"])
def test_linear_mutations_are_rejected(id):
    row = R.LIN_ROWS[id]
    refs = R.references(row, 0)
    x, xa, dy = R.inputs(row)
    R.check_wgrad(refs["dw32"].clone(), refs["db32"].clone(), refs, NAN_GUARD, id)
    rejected(refs["dw32"] - torch.outer(dy[-1], xa[-1]), refs["db32"], refs, NAN_GUARD)            # the token over the last whole chunk left out
    rejected(refs["dw32"], refs["db32"] - dy[-1], refs, NAN_GUARD)
    rejected(refs["dw32"].T.contiguous() if refs["dw32"].shape[0] == refs["dw32"].shape[1] else refs["dw32"].flip(0), refs["db32"], refs, NAN_GUARD)
    rejected(*R.ref32_linear(xa.bfloat16().float(), dy), refs, NAN_GUARD)
    if row.entry == "linear_leaky":
        rejected(*R.ref32_linear(x, dy), refs, NAN_GUARD)                                          # the activation left out
