"""The weight-gradient kernels against float64 at their edge shapes: nd_conv3x3_wgrad_nhwc_f32, nd_conv3x3_wgrad_leaky_nhwc_f32, nd_conv3x3_wgrad_cat_nhwc_f32,
nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32 under each pin of nd_conv3x3_wgrad_form (1, 2, 3), nd_linear_wgrad_f32 and nd_linear_wgrad_leaky_f32, called on raw pointers.

Every bound is util.derived on the fp32 reference of tests/wgrad_ref.py for the form that ran (the nine-tap chain, the Winograd-domain formula with the plan's split, the
linear chain); which form ran is the library's own answer (nd_conv3x3_wgrad_plan / nd_conv3x3_wgrad_cat_takes under the pin), which must equal the restated plan's.  A pin
that does not take a shape runs the form the library names and is checked against that form's reference.  What each case of the table reaches is proved from the restated
plans in tests/test_wgrad_ref.py; the nd_convt2x2 gradient and the 7x7 stem gradient have edge tables of their own (test_lsid_kernels.py, test_train_gpu.py).

Buffers: dw, db and the workspace -- exactly the floats the library's question returns -- each sit in a NaN-filled allocation with 64 guard floats on both sides, 16-byte
aligned; an operand sits in an allocation with one NaN image row (one NaN token) in front and behind, a strided one at a 16-byte-aligned channel offset of a wider tensor whose
other channels are NaN.  Every entry is called twice without a bias gradient and once with one: the same bits, a NULL dbias left untouched, every result finite, every guard
still NaN.  Twins, bit for bit under the same pin: a leaky entry and the plain entry on the activated copy, a slice and its dense copy, a two-source entry and the plain entry
on the materialised concatenation (Winograd-domain route) or two plain nine-tap gradients written into their columns (nine-tap route).

Not reached at test size: tensors of 2 GiB and more, which switch the nine-tap interior path off (a.fast), and the 1 GiB-per-sample limit of the Winograd-domain forms
(ww_runs).  Both stay covered by the questions of tests/test_host.py only.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hiputil as hu
import wgrad_ref as R
from hiputil import GUARD
from noisediff_amd import _lib as L

ENTRY = {"plain": "nd_conv3x3_wgrad_nhwc_f32", "leaky": "nd_conv3x3_wgrad_leaky_nhwc_f32", "cat": "nd_conv3x3_wgrad_cat_nhwc_f32",
         "cat_leaky_second": "nd_conv3x3_wgrad_cat_leaky_second_nhwc_f32", "linear": "nd_linear_wgrad_f32", "linear_leaky": "nd_linear_wgrad_leaky_f32"}


@pytest.fixture(scope="module")
def ctx():
    return hu.Ctx()


@pytest.fixture
def wgrad_form():
    """Pins a form of the 3x3 weight gradients for a test and restores the product's choice (by the shape) afterwards."""
    lib = L.load()
    was = lib.nd_conv3x3_wgrad_form(-1)
    yield lib.nd_conv3x3_wgrad_form
    lib.nd_conv3x3_wgrad_form(was)


class Operand:
    """A device allocation around channels off .. off + C - 1 of a [pixels][ld] tensor: NaN in every other channel and in ``guard`` pixels in front and behind."""

    def __init__(self, t, where=None, guard=1):
        Cc = t.shape[-1]
        self.ld, off = where or (Cc, 0)
        assert self.ld % 4 == 0 and off % 4 == 0 and off + Cc <= self.ld
        host = torch.full((t.numel() // Cc + 2 * guard, self.ld), float("nan"))
        host[guard: -guard, off: off + Cc] = t.reshape(-1, Cc)
        self.dev = hu.dev(host)
        self.ptr = self.dev.data_ptr() + 4 * (guard * self.ld + off)
        assert self.ptr % 16 == 0


class Out:
    """``n`` NaN floats for an entry to write, GUARD NaN floats on each side."""

    def __init__(self, n):
        self.dev = hu.full((n + 2 * GUARD,))
        self.ptr = self.dev.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def value(self):
        return self.dev[GUARD: -GUARD].cpu()

    def guards(self):
        return torch.cat((self.dev[:GUARD], self.dev[-GUARD:])).cpu()


def finish(ctx, rc, what):
    """Waits for the call; a HIP error (not a refusal: those are negative) may mean a faulted device -- nothing more runs on it from this file."""
    msg = ctx.lib.nd_last_error().decode() if rc else ""
    try:
        ctx.sync()
    except L.HipError as e:
        rc, msg = 1, str(e)
    if rc > 0:
        pytest.exit(f"{what}: HIP error {rc}: {msg}", returncode=3)
    return rc, msg


def launch(ctx, entry, shape, xs, y, n_ws, c0=0, what=""):
    """The call pattern of this file on guarded buffers: twice without a bias gradient, once with one.  -> (rc, message, dW host, db host, {guard name: host floats})."""
    lin = entry.startswith("linear")
    cin, cout = shape[-2:]
    ws = Out(n_ws)
    fn = getattr(ctx.lib, ENTRY[entry])
    outs, guards = [], {}
    for i, with_bias in enumerate((False, False, True)):
        dw, db = Out(cout * cin * (1 if lin else 9)), Out(cout)
        dbp = db.ptr if with_bias else None
        if lin or entry in ("plain", "leaky"):
            rc = fn(xs[0].ptr, xs[0].ld, y.ptr, y.ld, dw.ptr, dbp, ws.ptr, *shape, ctx.stream)
        else:
            B, H, W = shape[:3]
            rc = fn(xs[0].ptr, xs[0].ld, c0, xs[1].ptr, xs[1].ld, cin - c0, y.ptr, y.ld, dw.ptr, dbp, ws.ptr, B, H, W, cout, ctx.stream)
        rc, msg = finish(ctx, rc, what)
        outs.append((dw.value(), db.value()))
        guards.update({f"dw (call {i})": dw.guards(), f"db (call {i})": db.guards()})
        if rc:
            break
    guards["workspace"] = ws.guards()
    if rc:
        return rc, msg, outs[0][0], outs[0][1], guards
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0]), f"{what}: dW differs between calls (with / without the bias gradient)"
    assert bool(outs[0][1].isnan().all()) and bool(outs[1][1].isnan().all()), f"{what}: a NULL dbias was written"
    return 0, "", outs[2][0].reshape((cout, cin) if lin else (cout, cin, 3, 3)), outs[2][1], guards


def conv_operands(row, x):
    """The sources and dY of a row on the device: ``x`` is what the entry reads (raw for the entries that activate on load)."""
    B, H, W, cin, cout = row.shape
    dy = R.inputs(row)[2]
    if row.entry in ("plain", "leaky"):
        xs = [Operand(x, row.x0, W)]
    else:
        xs = [Operand(x[..., : row.c0].contiguous(), row.x0, W), Operand(x[..., row.c0:].contiguous(), row.x1, W)]
    return xs, Operand(dy, row.y, W)


def route(ctx, row):
    """The form the entry runs under the pin in force, by the library's own answers: 1 / 2 / 3, None where the entry refuses.  It must be the restated plan's."""
    lib = ctx.lib
    B, H, W, cin, cout = row.shape
    pin = lib.nd_conv3x3_wgrad_form(-1)
    form = lib.nd_conv3x3_wgrad_plan(B, H, W, cin, cout)
    assert form == R.form_that_runs(pin, B, H, W, cin, cout), (row.id, pin, form)
    if row.entry in ("plain", "leaky"):
        return form
    ld = lambda where, c: where[0] if where else c
    takes = lib.nd_conv3x3_wgrad_cat_takes(B, H, W, row.c0, cin - row.c0, cout, ld(row.x0, row.c0), ld(row.x1, cin - row.c0), ld(row.y, cout))
    assert bool(takes) == (row.c0 % 32 == 0 and (cin - row.c0) % 32 == 0 and form != 1), (row.id, pin, takes)
    return form if takes else None if row.entry == "cat" else 1


def workspace(ctx, row):
    B, H, W, cin, cout = row.shape
    if row.entry in ("plain", "leaky"):
        n = int(ctx.lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, cin, cout))
        assert n == R.workspace_floats(ctx.lib.nd_conv3x3_wgrad_form(-1), B, H, W, cin, cout)
        return n
    return int(ctx.lib.nd_conv3x3_wgrad_cat_workspace_floats(B, H, W, row.c0, cin - row.c0, cout))


_results = {}


def result(ctx, id, pin):
    """(form, dW, db) of a row under a pin: computed and checked once (a twin asks for it again)."""
    if (id, pin) in _results:
        return _results[id, pin]
    row = R.ROWS[id]
    x, xa, dy = R.inputs(row)
    form = route(ctx, row)
    what = f"{id} pin {pin}"
    xs, y = conv_operands(row, xa if row.entry == "plain" else x)
    rc, msg, dw, db, guards = launch(ctx, row.entry, row.shape, xs, y, workspace(ctx, row), row.c0, what)
    if form is None:
        assert rc < 0 and "Winograd-domain form" in msg, f"{what}: expected the refusal of two sources outside the Winograd-domain form, got {rc} '{msg}'"
        assert bool(dw.isnan().all()) and all(bool(g.isnan().all()) for g in guards.values()), f"{what}: a refused call wrote"
        out = (None, None, None)
    else:
        assert rc == 0, f"{what}: refused ({rc}: {msg})"
        R.check_wgrad(dw, db, R.references(row, form), guards, what)
        out = (form, dw, db)
    if len(_results) >= 4:
        _results.pop(next(iter(_results)))
    _results[id, pin] = out
    return out


def two_nine_tap_gradients(ctx, row, wgrad_form):
    """nd_conv3x3_wgrad_nhwc_f32 in its nine-tap form on each source of a row (the second one activated), dense: -> dW with each gradient in its columns, db of the first."""
    B, H, W, cin, cout = row.shape
    x, xa, dy = R.inputs(row)
    was = wgrad_form(1)
    parts = []
    for lo, hi in ((0, row.c0), (row.c0, cin)):
        shape = (B, H, W, hi - lo, cout)
        n_ws = int(ctx.lib.nd_conv3x3_wgrad_workspace_floats(*shape))
        rc, msg, dw, db, guards = launch(ctx, "plain", shape, [Operand(xa[..., lo:hi].contiguous(), None, W)], Operand(dy, None, W), n_ws, what=f"{row.id} source {lo}:{hi}")
        assert rc == 0, msg
        parts.append((dw, db))
    wgrad_form(was)
    return torch.cat((parts[0][0], parts[1][0]), 1), parts[0][1]


def twin_of(id):
    if id.startswith("leaky."):
        return "plain." + id[len("leaky."):]
    if id.endswith(".slice"):
        return id[: -len(".slice")]
    if id.startswith("cat"):
        return "plain." + id
    return None


# twins next to each other: the plain row, then the leaky one; a slice after its dense copy
CONV_RUNS = [(id, pin) for pin in R.PINS for id in R.ROWS]


@pytest.mark.parametrize("id,pin", CONV_RUNS, ids=[f"{id}-pin{pin}" for id, pin in CONV_RUNS])
def test_conv3x3_wgrad_entry_on_every_row_under_every_pin(ctx, wgrad_form, id, pin):
    row = R.ROWS[id]
    wgrad_form(pin)
    form, dw, db = result(ctx, id, pin)
    if form is None:                         # nd_conv3x3_wgrad_cat_nhwc_f32 where no Winograd-domain form takes the shape: refused, nothing written (asserted in `result`)
        assert row.entry == "cat" and pin == 1
        return
    if row.entry == "cat_leaky_second" and form == 1:
        tw, tb = two_nine_tap_gradients(ctx, row, wgrad_form)
    elif twin_of(id):
        tform, tw, tb = result(ctx, twin_of(id), pin)
        assert tform == form, f"{id}: ran form {form}, its twin {twin_of(id)} form {tform}"
    else:
        return
    assert torch.equal(dw, tw) and torch.equal(db, tb), f"{id} pin {pin}: not the bits of its twin"


@pytest.mark.parametrize("id", list(R.LIN_ROWS))
def test_linear_wgrad_entry_on_every_row(ctx, id):
    row = R.LIN_ROWS[id]
    x, xa, dy = R.inputs(row)
    n_ws = int(ctx.lib.nd_linear_wgrad_workspace_floats(*row.shape))
    assert n_ws == R.linear_plan(*row.shape)["workspace"]
    rc, msg, dw, db, guards = launch(ctx, row.entry, row.shape, [Operand(x, row.x)], Operand(dy, row.y), n_ws, what=id)
    assert rc == 0, msg
    R.check_wgrad(dw, db, R.references(row, 0), guards, id)
    # twin: the plain entry on the dense (activated) copy
    if row.entry == "linear_leaky" or row.x:
        rc, msg, tw, tb, _ = launch(ctx, "linear", row.shape, [Operand(xa)], Operand(dy), n_ws, what=id + " twin")
        assert rc == 0 and torch.equal(dw, tw) and torch.equal(db, tb), f"{id}: not the bits of the plain entry on the dense activated copy"


# ---------------------------------------------------------------------------------------------------------------- refusals

def _refused(ctx, entry, shape, xs, y, n_ws, why, c0=0):
    rc, msg, dw, db, guards = launch(ctx, entry, shape, xs, y, n_ws, c0, f"refusal ({why})")
    assert rc < 0 and why in msg, f"expected a refusal with '{why}', got {rc} '{msg}'"
    assert bool(dw.isnan().all()) and bool(db.isnan().all()) and all(bool(g.isnan().all()) for g in guards.values()), f"refusal ({why}): something was written"


def test_refusals_leave_dw_untouched(ctx, wgrad_form):
    """One refusal from each ND_DESC_REQUIRE of wgrad_shape and wgrad_cat_shape and one from lw_run; both sides of each limit: tests/test_host.py."""
    wgrad_form(2)
    row = R.ROWS["cat.w_sum.32_32"]
    B, H, W, cin, cout = row.shape
    x, xa, dy = R.inputs(row)
    n_ws = int(ctx.lib.nd_conv3x3_wgrad_workspace_floats(B, H, W, cin, cout))
    dense, y = [Operand(x, None, W)], Operand(dy, None, W)
    _refused(ctx, "plain", (0, H, W, cin, cout), dense, y, n_ws, "non-positive size")
    _refused(ctx, "plain", (B, H, W, cin - 2, cout), dense, y, n_ws, "must be multiples of 4")
    halves = lambda c0: [Operand(x[..., :c0].contiguous(), None, W), Operand(x[..., c0:].contiguous(), None, W)]
    _refused(ctx, "cat", row.shape, halves(16), y, n_ws, "whole 32-channel blocks", c0=16)
    rag = R.ROWS["cat_leaky_second.ragged.36_4"]                       # two 32-channel sources at a shape no Winograd-domain form takes (H % 4, W % 16)
    B, H, W, _, cout = rag.shape
    xr, dyr = R._draw("x", (B, H, W, 64)), R.inputs(rag)[2]
    n_ws = int(ctx.lib.nd_conv3x3_wgrad_cat_workspace_floats(B, H, W, 32, 32, cout))
    _refused(ctx, "cat", (B, H, W, 64, cout), [Operand(xr[..., :32].contiguous(), (48, 8), W), Operand(xr[..., 32:].contiguous(), None, W)], Operand(dyr, None, W), n_ws,
             "Winograd-domain form", c0=32)
    lrow = R.LIN_ROWS["linear.one_over"]
    N, cin, cout = lrow.shape
    x, xa, dy = R.inputs(lrow)
    xo = Operand(x)
    xo.ld = cin - 4                                                     # a token stride below cin
    _refused(ctx, "linear", lrow.shape, [xo], Operand(dy), int(ctx.lib.nd_linear_wgrad_workspace_floats(N, cin, cout)), "token strides")
