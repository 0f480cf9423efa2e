"""The conv driver on an MI355X: one case per route through ``fvit_conv3x3`` with every image of the weights present, at the shapes that separate
the route rules (tests/test_conv_route_cpu.py), against F.conv2d in fp64 on the 16-bit-rounded operands (+ bias, activation, residual), and
bitwise against the entry point from before the driver that names the same kernel -- the wrapper and the struct path are one launch.

Tolerances are those of the existing conv tests: 16-bit routes 5e-3 (fp16) / 3e-2 (bf16) x max(|ref|max, 1) (tests/test_gpu_kernels.py); <ln>
routes one unit in the last place of the exact LayerNorm of the plain route's map (tests/test_gpu_level_glue_fusion.py); two-term-map routes
2e-6 x max(|ref|max, 1) on hi + lo (tests/test_gpu_px.py)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from fastervit_amd import _lib
from fastervit_amd.conv_runtime import frag_pack_conv128
from tests.util import tuned

pytestmark = pytest.mark.gpu
B = 2
F16, BF16 = (torch.float16, _lib.FVIT_F16, 5e-3, 2.0 ** -10), (torch.bfloat16, _lib.FVIT_BF16, 3e-2, 2.0 ** -7)
# (route, Cin, cin_valid, Cout, H = W, stride, act, residual)
PLAIN = [("conv3x3_c64_halo_kernel", 64, 64, 64, 16, 1, 2, False), ("conv3x3_c128_band_kernel", 128, 128, 128, 14, 1, 0, True),
         ("conv3x3_kernel<2,2,4,patch>", 128, 128, 128, 32, 1, 1, True), ("conv3x3_kernel<2,2,4>", 64, 64, 128, 16, 2, 0, False),
         ("conv3x3_kernel<2,2,4,dense>", 128, 104, 128, 14, 1, 2, True), ("conv3x3_kernel<2,2,2>", 128, 128, 64, 16, 1, 2, False),
         ("conv3x3_kernel<2,2,2,dense>", 64, 40, 64, 16, 1, 0, True), ("conv3x3_kernel<4,1,4>", 128, 128, 64, 16, 1, 1, True)]
LN = [("conv3x3_c64_halo_kernel<ln>", 64, 16), ("conv3x3_c128_band_kernel<ln>", 128, 14)]
PX = [("conv3x3_kernel<2,2,4,px,patch>", 128, 128, 128, 16), ("conv3x3_kernel<2,2,4,px>", 128, 128, 128, 14),
      ("conv3x3_kernel<2,2,4,px,dense>", 128, 104, 128, 14), ("conv3x3_kernel<2,2,2,px>", 64, 64, 64, 16), ("conv3x3_kernel<2,2,2,px,dense>", 64, 40, 64, 16)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _split(t, dt):
    hi = t.to(dt)
    return hi, (t - hi.float()).to(dt)


def _pack(w, cv, dt, terms):
    """fp32 (Co, Ci, 3, 3) weight with zero pad channels -> (classic rows, dense rows or None, fragment stream or None, the value the kernels see)."""
    Co, Ci = w.shape[:2]
    planes = [p.permute(0, 2, 3, 1).contiguous() for p in _split(w, dt)[:terms]]   # (Co, 3, 3, Ci)
    classic = torch.cat([p.reshape(Co, -1) for p in planes], dim=1).contiguous().cuda()
    dense = None
    if cv < Ci:
        kd = _lib.lib().fvit_conv3x3_dense_k(cv)
        rows = torch.zeros(Co, terms, kd, dtype=dt)
        for t, p in enumerate(planes):
            rows[:, t, :9 * cv] = p[..., :cv].reshape(Co, 9 * cv)
        dense = rows.reshape(Co, -1).contiguous().cuda()
    frag = frag_pack_conv128(classic.reshape(128, 1152)) if (Co, Ci, terms, cv) == (128, 128, 1, 128) else None
    return classic, dense, frag, sum(p.double() for p in planes).permute(0, 3, 1, 2)


def _case(seed, Ci, cv, Co, hw, stride, dt, terms):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, hw, hw, Ci, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (9 * cv) ** 0.5
    x[..., cv:] = 0
    w[:, cv:] = 0
    ho = (hw - 1) // stride + 1
    return g, x, _pack(w, cv, dt, terms), torch.randn(Co, generator=g), torch.randn(B, ho, ho, Co, generator=g), torch.zeros(256, dtype=dt, device="cuda")


def _run(code, images, terms, cv, want, **call):
    lib = _lib.lib()
    w = _lib.FvitConvWeights(_ptr(images[0]), _ptr(images[1]), _ptr(images[2]), terms, cv)
    c = _lib.FvitConvCall(**{k: (_ptr(v) if torch.is_tensor(v) else v) for k, v in call.items()})
    assert lib.fvit_conv3x3_route_name(lib.fvit_conv3x3_route(code, w, c)).decode() == want, lib.fvit_last_error()
    _lib.check(lib.fvit_conv3x3(code, w, c, _stream()), "fvit_conv3x3")


@pytest.mark.parametrize("dt,code,tol,ulp", [F16, BF16])
@pytest.mark.parametrize("route,Ci,cv,Co,hw,stride,act,res", PLAIN)
def test_16_bit_routes(route, Ci, cv, Co, hw, stride, act, res, dt, code, tol, ulp):
    lib = _lib.lib()
    terms = 2 if route == "conv3x3_kernel<2,2,2>" else 1   # one case with two-term weights on 16-bit maps
    g, x, (classic, dense, frag, wv), bias, r, zeros = _case(Ci + Co + hw, Ci, cv, Co, hw, stride, dt, terms)
    x, bias, r = x.to(dt).cuda(), bias.cuda(), r.to(dt).cuda()
    out, old = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    res_p = _ptr(r) if res else None
    with tuned(conv64_variant=1) if route == "conv3x3_kernel<4,1,4>" else contextlib.nullcontext():
        _run(code, (classic, dense, frag), terms, cv, route, in_=x, bias=bias, residual=r if res else None, out=out, zeros=zeros, B=B, Hi=hw, Wi=hw,
             Cin=Ci, Cout=Co, stride=stride, act=act)
        if frag is not None and hw <= 30:
            rc = lib.fvit_conv3x3_c128_band(code, x.data_ptr(), frag.data_ptr(), bias.data_ptr(), res_p, old.data_ptr(), B, hw, hw, act, zeros.data_ptr(), _stream())
        else:
            rc = lib.fvit_conv3x3_nhwc_dense(code, x.data_ptr(), (dense if "dense" in route else classic).data_ptr(), bias.data_ptr(), res_p, old.data_ptr(),
                                             B, hw, hw, Ci, cv if "dense" in route else Ci, Co, stride, act, terms, zeros.data_ptr(), _stream())
        _lib.check(rc, "the entry point from before the driver")
    torch.cuda.synchronize()
    ref = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), wv, bias.double().cpu(), stride, 1)
    ref = [lambda t: t, torch.relu, F.gelu][act](ref).permute(0, 2, 3, 1)
    if res:
        ref = ref + r.double().cpu()
    err, bound = (out.double().cpu() - ref).abs().max().item(), tol * max(ref.abs().max().item(), 1.0)
    print(f"{route} {dt}: max-abs {err:.2e} (bound {bound:.1e})")
    assert torch.isfinite(out.float()).all() and err < bound
    assert torch.equal(out, old)


@pytest.mark.parametrize("dt,code,tol,ulp", [F16, BF16])
@pytest.mark.parametrize("route,C,hw", LN)
def test_ln_routes(route, C, hw, dt, code, tol, ulp):
    lib = _lib.lib()
    g, x, images, bias, r, zeros = _case(C + hw, C, C, C, hw, 1, dt, 1)
    x, bias, r = x.to(dt).cuda(), bias.cuda(), r.to(dt).cuda()
    lw, lb, eps = (1.0 + 0.5 * torch.randn(C, generator=g)).cuda(), (0.5 * torch.randn(C, generator=g)).cuda(), 1e-6
    plain, fused, old = torch.full_like(r, float("nan")), r.clone(), r.clone()   # <ln>: in place on the residual, as the plan runs it
    call = dict(in_=x, bias=bias, residual=r, out=plain, zeros=zeros, B=B, Hi=hw, Wi=hw, Cin=C, Cout=C, stride=1, act=0)
    _run(code, images[:3], 1, C, route[:-4], **call)
    _run(code, images[:3], 1, C, route, **dict(call, residual=fused, out=fused, ln_w=lw, ln_b=lb, ln_eps=eps))
    fn, wt = (lib.fvit_conv3x3_c64_ln2d, images[0]) if C == 64 else (lib.fvit_conv3x3_c128_band_ln2d, images[2])
    _lib.check(fn(code, x.data_ptr(), wt.data_ptr(), bias.data_ptr(), old.data_ptr(), old.data_ptr(), lw.data_ptr(), lb.data_ptr(), eps, B, hw, hw,
                  zeros.data_ptr(), _stream()), "the entry point from before the driver")
    torch.cuda.synchronize()
    exact = F.layer_norm(plain.double().cpu(), (C,), lw.double().cpu(), lb.double().cpu(), eps)
    worst = ((fused.double().cpu() - exact).abs() / (ulp * exact.abs() + 1e-5)).max().item()
    print(f"{route} {dt}: worst error / bound {worst:.3f}")
    assert torch.isfinite(fused.float()).all() and worst <= 1.0
    assert torch.equal(fused, old)
    # a route without the epilogue refuses the LayerNorm2d parameters instead of dropping them
    with tuned(conv_halo=0, conv_band=0):
        w = _lib.FvitConvWeights(_ptr(images[0]), None, _ptr(images[2]), 1, C)
        c = _lib.FvitConvCall(**{k: (_ptr(v) if torch.is_tensor(v) else v) for k, v in dict(call, residual=old, out=old, ln_w=lw, ln_b=lb, ln_eps=eps).items()})
        assert lib.fvit_conv3x3(code, w, c, _stream()) == -1 and b"LayerNorm2d" in lib.fvit_last_error()
    torch.cuda.synchronize()
    assert torch.equal(fused, old)


@pytest.mark.parametrize("route,Ci,cv,Co,hw", PX)
def test_two_term_map_routes(route, Ci, cv, Co, hw):
    lib = _lib.lib()
    dt, code = torch.float16, _lib.FVIT_F16
    g, x, (classic, dense, _, wv), bias, r, zeros = _case(Ci + Co + hw + 1, Ci, cv, Co, hw, 1, dt, 2)
    (xh, xl), (rh, rl), bias = [t.cuda() for t in _split(x, dt)], [t.cuda() for t in _split(r * 3, dt)], bias.cuda()
    oh, ol, old_h, old_l = rh.clone(), rl.clone(), rh.clone(), rl.clone()   # in place over the residual planes
    _run(code, (classic, dense, None), 2, cv, route, in_=xh, in_lo=xl, bias=bias, residual=oh, residual_lo=ol, out=oh, out_lo=ol, zeros=zeros, B=B, Hi=hw, Wi=hw,
         Cin=Ci, Cout=Co, stride=1, act=0)
    _lib.check(lib.fvit_conv3x3_nhwc_px_dense(code, xh.data_ptr(), xl.data_ptr(), (dense if "dense" in route else classic).data_ptr(), bias.data_ptr(),
                                              old_h.data_ptr(), old_l.data_ptr(), old_h.data_ptr(), old_l.data_ptr(), None, B, hw, hw, Ci,
                                              cv if "dense" in route else Ci, Co, 1, 0, 2, zeros.data_ptr(), _stream()), "the entry point from before the driver")
    torch.cuda.synchronize()
    ref = F.conv2d((xh.double() + xl.double()).cpu().permute(0, 3, 1, 2), wv, bias.double().cpu(), 1, 1).permute(0, 2, 3, 1) + (rh.double() + rl.double()).cpu()
    got = oh.double().cpu() + ol.double().cpu()
    err, bound = (got - ref).abs().max().item(), 2e-6 * max(ref.abs().max().item(), 1.0)
    print(f"{route}: max-abs {err:.2e} (bound {bound:.1e})")
    assert torch.isfinite(got).all() and err < bound
    assert torch.equal(oh, old_h) and torch.equal(ol, old_l)
