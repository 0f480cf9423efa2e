"""Runs the cases of tests/conv_refs.py through the C ABI on the GPU (tests/test_gpu_conv_exact.py, tests/test_gpu_conv_values.py): weight packing, buffers
poisoned around and inside, the launch under the case's fvit_tune knobs, the route name, and the guards read back.

Poison: every output buffer is NaN-prefilled and sits between two NaN guard rows of pixels that must still be NaN afterwards; every input map sits
between two NaN guard rows; the pad channels of a channel-padded map are NaN on the dense routes (which must never read them).  Stem images that are a
crop lie inside a NaN-filled larger tensor."""
import contextlib
import ctypes

import torch

from fastervit_amd import _lib, hat_runtime
from fastervit_amd.conv_runtime import frag_pack_conv128
from tests import conv_refs as R
from tests.util import tuned

CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A (B, H, W, C) map on the device between two NaN guard rows of W * C elements."""

    def __init__(self, shape, dtype, fill=None):
        B, H, W, C = shape
        self.row, n = W * C, B * H * W * C
        self.buf = torch.full((n + 2 * self.row,), NAN, dtype=dtype, device="cuda")
        self.map = self.buf[self.row:self.row + n].view(B, H, W, C)
        if fill is not None:
            self.map.copy_(fill.to(dtype))

    def ptr(self):
        return self.map.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.row]).all() and torch.isnan(self.buf[-self.row:]).all())


def pack_weights(c, inp, dt):
    """(classic rows, dense rows or None, fragment stream or None) of a case's weight planes, on the device."""
    planes = [p.permute(0, 2, 3, 1).contiguous().to(dt) for p in inp.w]                        # (Co, 3, 3, Ci)
    classic = torch.cat([p.reshape(c.Co, -1) for p in planes], dim=1).contiguous().cuda()
    dense = frag = None
    if c.cv < c.Ci:
        kd = _lib.lib().fvit_conv3x3_dense_k(c.cv)
        rows = torch.zeros(c.Co, c.terms, kd, dtype=dt)
        for t, p in enumerate(planes):
            rows[:, t, :9 * c.cv] = p[..., :c.cv].reshape(c.Co, 9 * c.cv)
        dense = rows.reshape(c.Co, -1).contiguous().cuda()
    if c.route == R.BAND:
        frag = frag_pack_conv128(classic.reshape(128, 1152))
    return classic, dense, frag


def knobs(c):
    """The case's fvit_tune settings for the body (tests.util.tuned), nothing where the defaults already give its route."""
    return tuned(**dict(c.knobs)) if c.knobs else contextlib.nullcontext()


class ConvRun:
    """One case's device state; ``run`` launches one epilogue (inside ``knobs(c)``) and returns the output planes as CPU float64 tensors."""

    def __init__(self, c, inp, dt):
        self.c, self.inp, self.dt = c, inp, dt
        self.classic, self.dense, self.frag = pack_weights(c, inp, dt)
        x = inp.x.clone()
        if "dense" in c.route:
            x[..., c.cv:] = NAN
        self.x = Guarded(x.shape, dt, x)
        self.x_lo = None
        if inp.x_lo is not None:
            xl = inp.x_lo.clone()
            if "dense" in c.route:
                xl[..., c.cv:] = NAN
            self.x_lo = Guarded(xl.shape, dt, xl)
        self.bias = inp.bias.cuda()
        self.zeros = torch.zeros(256, dtype=dt, device="cuda")
        self.oshape = (c.B, R.out_size(c.H, c.stride), R.out_size(c.W, c.stride), c.Co)

    def run(self, act, res=False, in_place=False):
        """res: False, "hi" (the residual plane alone) or True (+ residual_lo where the case has one)."""
        c, inp, dt, lib = self.c, self.inp, self.dt, _lib.lib()
        r_hi = Guarded(self.oshape, dt, inp.res) if res else None
        r_lo = Guarded(self.oshape, dt, inp.res_lo) if res is True and inp.res_lo is not None else None
        out = out_lo = out_f32 = None
        if c.out == "f32":
            out_f32 = Guarded(self.oshape, torch.float32)
        else:
            out = r_hi if in_place else Guarded(self.oshape, dt)
            if c.out == "lo":
                out_lo = r_lo if in_place and r_lo is not None else Guarded(self.oshape, dt)
        p = lambda g: g.ptr() if g is not None else None            # noqa: E731
        w = _lib.FvitConvWeights(self.classic.data_ptr() if self.classic is not None else None, self.dense.data_ptr() if self.dense is not None else None,
                                 self.frag.data_ptr() if self.frag is not None else None, c.terms, c.cv)
        call = _lib.FvitConvCall(in_=p(self.x), in_lo=p(self.x_lo), bias=self.bias.data_ptr(), residual=p(r_hi), residual_lo=p(r_lo), out=p(out),
                                 out_lo=p(out_lo), out_f32=p(out_f32), zeros=self.zeros.data_ptr(), B=c.B, Hi=c.H, Wi=c.W, Cin=c.Ci, Cout=c.Co,
                                 stride=c.stride, act=act, px=1 if "px" in c.route else 0)
        name = lib.fvit_conv3x3_route_name(lib.fvit_conv3x3_route(CODE[dt], w, call)).decode()
        assert name == c.route, (name, lib.fvit_last_error())
        _lib.check(lib.fvit_conv3x3(CODE[dt], w, call, stream()), "fvit_conv3x3")
        torch.cuda.synchronize()
        for g in (self.x, self.x_lo, r_hi, r_lo, out, out_lo, out_f32):
            assert g is None or g.guards_intact()
        got = {k: g.map.cpu().to(R.F64) for k, g in (("hi", out), ("lo", out_lo), ("f32", out_f32)) if g is not None}
        if res and not in_place:                           # an out-of-place launch leaves the residual as it was
            assert torch.equal(r_hi.map.cpu().float(), inp.res)
        return got


def stem_tensor(c, raw):
    """The caller's image tensor of a stem case on the device, in the case's format; logical shape (B, 3, H, W)."""
    fmt, t = c.fmt, raw.to(R.FORMAT_DTYPE[c.fmt])
    if fmt == "crop":
        big = torch.full((c.B, 3, c.H + 3, c.W + 5), NAN, device="cuda")
        view = big[:, :, 1:1 + c.H, 2:2 + c.W]
        view.copy_(t)
        return view
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if fmt.endswith("nhwc") else t.contiguous()


def _stem_w1(planes, dt):
    out = []
    for p in planes:
        wk = torch.zeros(64, 32)
        wk[:, :27] = p.permute(0, 2, 3, 1).reshape(64, 27)
        out.append(wk.to(dt).contiguous().cuda())
    return out


def run_stem(c, inp, dt):
    """Launches a stem case; the (B, Ho, Wo, 64) output as CPU float64."""
    lib = _lib.lib()
    x = stem_tensor(c, inp.raw)
    view = hat_runtime._map_view(x)
    w1 = _stem_w1(inp.w1, dt)
    b1 = inp.b1.cuda()
    H1, W1 = R.out_size(c.H, 2), R.out_size(c.W, 2)
    with knobs(c):
        if c.kernel == "stem_fused":
            out = Guarded((c.B, R.out_size(H1, 2), R.out_size(W1, 2), 64), dt)
            w2, b2 = inp.w2.permute(0, 2, 3, 1).contiguous().to(dt).cuda(), inp.b2.cuda()
            _lib.check(lib.fvit_stem_fused(CODE[dt], ctypes.byref(view), w1[0].data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.ptr(),
                                           c.B, c.H, c.W, stream()), "stem_fused")
        elif c.kernel == "stem_conv_px":
            out = Guarded((c.B, H1, W1, 64), dt)
            _lib.check(lib.fvit_stem_conv3x3s2_px(CODE[dt], ctypes.byref(view), w1[0].data_ptr(), w1[1].data_ptr(), b1.data_ptr(), out.ptr(), c.B, c.H, c.W,
                                                  stream()), "stem_conv_px")
        else:
            out = Guarded((c.B, H1, W1, 64), dt)
            _lib.check(lib.fvit_stem_conv3x3s2(CODE[dt], ctypes.byref(view), w1[0].data_ptr(), b1.data_ptr(), out.ptr(), c.B, c.H, c.W, stream()), "stem_conv")
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.map.cpu().to(R.F64)
