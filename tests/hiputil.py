"""Helpers to call the C ABI directly from tests (torch only as a device-memory allocator)."""
import ctypes as C

import torch

from noisediff_amd import _lib as L
from noisediff_amd._host import CONV3X3

DEV = torch.device("cuda", 0)


class Ctx:
    def __init__(self):
        self.lib = L.load()
        self.stream = C.c_void_p()
        L.call("nd_stream_create", C.byref(self.stream))

    def sync(self):
        L.call("nd_stream_sync", self.stream)


def _settle(t):
    # torch's copies / fills run on torch's stream; the library runs on its own non-blocking stream
    torch.cuda.synchronize(DEV)
    return t


def dev(t):
    return _settle(t.to(DEV).contiguous())


def full(shape, value=float("nan")):
    return _settle(torch.full(shape, value, device=DEV))


GUARD = 64


class Guarded:
    """A device allocation around a host tensor: NaN everywhere but the tensor.  NHWC images ([B][H][W][C], ``pad`` unused columns per pixel): [1 + B H + 1][W][C + pad];
    anything else flat with GUARD floats on each side.  ``ptr`` addresses the tensor's first element (16-byte aligned: strides are multiples of 4 floats)."""

    def __init__(self, t, pad=None):
        self.shape = tuple(t.shape)
        if pad is None:
            host = torch.full((t.numel() + 2 * GUARD,), float("nan"))
            host[GUARD: GUARD + t.numel()] = t.reshape(-1)
            self.region, first = (slice(GUARD, GUARD + t.numel()),), GUARD
        else:
            B, H, W, Cc = t.shape
            self.ld = Cc + pad
            host = torch.full((B * H + 2, W, self.ld), float("nan"))
            host[1:-1, :, :Cc] = t.reshape(B * H, W, Cc)
            self.region, first = (slice(1, -1), slice(None), slice(0, Cc)), W * self.ld
        self.dev = dev(host)
        self.ptr = self.dev.data_ptr() + 4 * first
        assert self.ptr % 16 == 0

    def host(self):
        return self.dev.cpu()

    def tensor(self, buf=None):
        return (self.host() if buf is None else buf)[self.region].reshape(self.shape)


def nan_like(shape, pad=None):
    return Guarded(torch.full(shape, float("nan")), pad)


def nhwc(t):           # NCHW cpu -> NHWC gpu
    return _settle(t.permute(0, 2, 3, 1).contiguous().to(DEV))


def nchw(t):           # NHWC gpu -> NCHW cpu
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def src(t, t2=None, mode=L.PRO_NONE, **kw):
    # the struct only holds raw pointers: the builder keeps the tensors alive on it (a freed block would be recycled by
    # torch's caching allocator for the next allocation, e.g. the NaN-filled output buffer)
    return L.src(t, t2, mode, **kw)


def pack_conv3(ctx, w):
    cout, cin = w.shape[:2]
    n = ctx.lib.nd_pack_conv3x3_weight_floats(cin, cout)
    wd, out = dev(w), torch.empty(n, device=DEV)
    L.call("nd_pack_conv3x3_weight", wd.data_ptr(), out.data_ptr(), cin, cout, ctx.stream)
    ctx.sync()
    return out


def pack_pw(ctx, w, unshuffle_c=0):
    w = w.reshape(w.shape[0], -1)
    cout, cin = w.shape
    n = ctx.lib.nd_pack_pointwise_weight_floats(cin, cout)
    wd, out = dev(w), torch.empty(n, device=DEV)
    L.call("nd_pack_pointwise_weight", wd.data_ptr(), out.data_ptr(), cin, cout, unshuffle_c, ctx.stream)
    ctx.sync()
    return out


def conv3x3(ctx, s, wp, bias, B, H, W, cin, cout, stats=False, kind="direct"):
    out = full((B, H, W, cout))
    k = CONV3X3[kind]
    st = sc = None
    slots = 0
    if stats:
        slots = k.stat_slots(ctx.lib, B, H, W, cout)
        st = full((B, slots, cout, 2))
        sc = full((slots,))
    d = L.conv3x3(s, wp, bias, out, B, H, W, cin, cout, stats=st, slot_count=sc)
    L.call(k.entry, C.byref(d), ctx.stream)
    ctx.sync()
    return out, st, sc, slots


def pointwise(ctx, s, wp, bias, B, HW, W, cin, cout, act=0, res0=None, res1=None, vec=None, gn_t=None, gn_mad=None, entry="nd_pointwise_gemm_nhwc_f32"):
    out = full((B, HW, cout))
    d = L.pointwise(s, wp, bias, out, B, HW, W, cin, cout, act=act, res0=res0, res1=res1, vec=vec, gn_t=gn_t, gn_mad=gn_mad)
    L.call(entry, C.byref(d), ctx.stream)
    ctx.sync()
    return out


def gn_finalize(ctx, st, sc, slots, gamma, beta, ss, B, Cc, groups):
    mad = full((B, 3, Cc))
    L.call("nd_groupnorm_finalize_f32", st.data_ptr(), sc.data_ptr(), slots, gamma.data_ptr(), beta.data_ptr(),
           None if ss is None else ss.data_ptr(), 0 if ss is None else ss.shape[-1], mad.data_ptr(), B, Cc, groups, 1e-5, ctx.stream)
    ctx.sync()
    return mad
