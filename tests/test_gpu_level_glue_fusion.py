"""The level-glue fusions of the 16-bit deploy plan on an MI355X: LayerNorm2d in the epilogue of the conv / window_reverse that produces a level's last
map, and the global average pool taken straight from the token rows of a one-window last level.

Each fused kernel is compared with the EXACT result: LayerNorm (fp64, torch CPU) of the 16-bit map that the existing route -- the same conv / reverse
kernel without the fusion -- produces on the same inputs.  Both roundings are correct to half a unit in the last place of the map type and the fp32
statistics add about 1e-6, so the bound is one such unit: |got - exact| <= 2^-10 |exact| + 1e-5 (fp16), 2^-7 |exact| + 1e-5 (bf16).  The existing
two-kernel route (map, then ``fvit_layernorm2d_cl``) is held to the same bound in the same test, which shows the bound is reachable.  The pool writes
fp32: 1e-5 relative."""
import pytest
import torch
import torch.nn.functional as F

from fastervit_amd import _lib, hat_runtime
from tests.util import build_product_model, case_input, load_golden, max_abs

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float16, _lib.FVIT_F16, 2.0 ** -10), (torch.bfloat16, _lib.FVIT_BF16, 2.0 ** -7)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ln_params(C, g):
    return (1.0 + 0.5 * torch.randn(C, generator=g)).cuda(), (0.5 * torch.randn(C, generator=g)).cuda()


def _exact_ln(map_nhwc, w, b, eps):
    """fp64 LayerNorm over the last dimension of a 16-bit [..., C] map."""
    return F.layer_norm(map_nhwc.double().cpu(), (map_nhwc.shape[-1],), w.double().cpu(), b.double().cpu(), eps)


def _within_one_unit(got, exact, ulp, what):
    err = (got.double().cpu() - exact).abs()
    bound = ulp * exact.abs() + 1e-5
    worst = (err / bound).max().item()
    print(f"{what}: max |got - exact| {err.max().item():.3e}, worst error / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0, what


def _two_kernel_ln(code, plain, w, b, eps):
    """The existing route's second kernel: fvit_layernorm2d_cl on the dense [B][H][W][C] map ``plain``."""
    out = torch.empty_like(plain)
    C = plain.shape[-1]
    _lib.check(_lib.lib().fvit_layernorm2d_cl(code, plain.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), eps, plain.numel() // C, C, C,
                                              _stream()), "fvit_layernorm2d_cl")
    return out


@pytest.mark.parametrize("dt,code,ulp", DTYPES)
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (20, 56, 56)])   # partial 8 x 16 tiles both ways; 560 tiles on 512 workgroups (the deferred store crosses iterations)
def test_halo_conv_ln2d(dt, code, ulp, B, H, W):
    lib = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H)
    x = torch.randn(B, H, W, 64, generator=g).to(dt).cuda()
    r = torch.randn(B, H, W, 64, generator=g).to(dt).cuda()
    wk = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dt).cuda()
    bias = torch.randn(64, generator=g).cuda()
    lw, lb = _ln_params(64, g)
    eps = 1e-6
    zeros = torch.zeros(256, dtype=dt, device="cuda")
    plain = torch.full_like(x, float("nan"))
    _lib.check(lib.fvit_conv3x3_nhwc(code, x.data_ptr(), wk.data_ptr(), bias.data_ptr(), r.data_ptr(), plain.data_ptr(), B, H, W, 64, 64, 1, 0,
                                     zeros.data_ptr(), _stream()), "conv3x3")
    fused = r.clone()   # in place on the residual, as the plan runs it
    _lib.check(lib.fvit_conv3x3_c64_ln2d(code, x.data_ptr(), wk.data_ptr(), bias.data_ptr(), fused.data_ptr(), fused.data_ptr(), lw.data_ptr(),
                                         lb.data_ptr(), eps, B, H, W, zeros.data_ptr(), _stream()), "conv3x3_c64_ln2d")
    two = _two_kernel_ln(code, plain, lw, lb, eps)
    torch.cuda.synchronize()
    exact = _exact_ln(plain, lw, lb, eps)
    _within_one_unit(fused, exact, ulp, f"halo conv + LayerNorm2d {B}x{H}x{W}")
    _within_one_unit(two, exact, ulp, f"halo conv, then LayerNorm2d {B}x{H}x{W}")
    again = r.clone()
    _lib.check(lib.fvit_conv3x3_c64_ln2d(code, x.data_ptr(), wk.data_ptr(), bias.data_ptr(), again.data_ptr(), again.data_ptr(), lw.data_ptr(),
                                         lb.data_ptr(), eps, B, H, W, zeros.data_ptr(), _stream()), "conv3x3_c64_ln2d")
    torch.cuda.synchronize()
    assert torch.equal(again, fused)
    assert lib.fvit_conv3x3_c64_ln2d(code, x.data_ptr(), wk.data_ptr(), bias.data_ptr(), None, fused.data_ptr(), lw.data_ptr(), lb.data_ptr(), eps,
                                     B, H, W, zeros.data_ptr(), _stream()) != 0   # no residual: not this kernel's epilogue


@pytest.mark.parametrize("dt,code,ulp", DTYPES)
@pytest.mark.parametrize("B,H,W", [(2, 28, 28), (3, 20, 20)])   # four full bands; row bands that do not divide H
def test_band_conv_ln2d(dt, code, ulp, B, H, W):
    from fastervit_amd.conv_runtime import frag_pack_conv128
    lib = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H)
    x = torch.randn(B, H, W, 128, generator=g).to(dt).cuda()
    r = torch.randn(B, H, W, 128, generator=g).to(dt).cuda()
    wk = (torch.randn(128, 3, 3, 128, generator=g) / (9 * 128) ** 0.5).to(dt).cuda()
    wf = frag_pack_conv128(wk.reshape(128, 1152))
    bias = torch.randn(128, generator=g).cuda()
    lw, lb = _ln_params(128, g)
    eps = 1e-6
    zeros = torch.zeros(256, dtype=dt, device="cuda")
    plain = torch.full_like(x, float("nan"))
    _lib.check(lib.fvit_conv3x3_c128_band(code, x.data_ptr(), wf.data_ptr(), bias.data_ptr(), r.data_ptr(), plain.data_ptr(), B, H, W, 0,
                                          zeros.data_ptr(), _stream()), "conv3x3_c128_band")
    fused = r.clone()
    _lib.check(lib.fvit_conv3x3_c128_band_ln2d(code, x.data_ptr(), wf.data_ptr(), bias.data_ptr(), fused.data_ptr(), fused.data_ptr(), lw.data_ptr(),
                                               lb.data_ptr(), eps, B, H, W, zeros.data_ptr(), _stream()), "conv3x3_c128_band_ln2d")
    two = _two_kernel_ln(code, plain, lw, lb, eps)
    torch.cuda.synchronize()
    exact = _exact_ln(plain, lw, lb, eps)
    _within_one_unit(fused, exact, ulp, f"band conv + LayerNorm2d {B}x{H}x{W}")
    _within_one_unit(two, exact, ulp, f"band conv, then LayerNorm2d {B}x{H}x{W}")
    assert lib.fvit_conv3x3_c128_band_ln2d(code, x.data_ptr(), wf.data_ptr(), bias.data_ptr(), fused.data_ptr(), fused.data_ptr(), lw.data_ptr(),
                                           lb.data_ptr(), eps, B, H, 31, zeros.data_ptr(), _stream()) != 0   # wider than the band kernel takes


@pytest.fixture(scope="module")
def level2():
    """Level 2 of faster_vit_0_224: 14 x 14 x 256, 7 x 7 windows with 2 x 2 carrier rows per window, propagation into the reverse."""
    model, _ = build_product_model("fvit0_224", "cuda")
    return model.levels[2]


@pytest.mark.parametrize("dt,ulp", [(d, u) for d, _, u in DTYPES])
@pytest.mark.parametrize("strided", [False, True])
def test_reverse_ln2d(level2, dt, ulp, strided):
    g = torch.Generator(device="cpu").manual_seed(7)
    C = 256
    x = torch.randn(2, C, 14, 14, generator=g).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    lw, lb = _ln_params(C, g)
    eps = 1e-6
    with torch.no_grad():
        plain = hat_runtime.stage_forward(level2, x)
        if strided:   # the first C channels of a wider map; the pad channels are not touched
            wide = torch.full((2, C + 64, 14, 14), 3.0, dtype=dt, device="cuda").contiguous(memory_format=torch.channels_last)
            fused = wide[:, :C]
        else:
            fused = torch.empty_like(x)
        assert hat_runtime.ln2d_tail_supported(x, fused)
        hat_runtime.stage_forward(level2, x, out=fused, ln2d=(lw, lb, eps))
        two = _two_kernel_ln(hat_runtime._DT[dt], plain.permute(0, 2, 3, 1).contiguous(), lw, lb, eps)
    torch.cuda.synchronize()
    exact = _exact_ln(plain.permute(0, 2, 3, 1), lw, lb, eps)
    _within_one_unit(fused.permute(0, 2, 3, 1), exact, ulp, f"reverse + LayerNorm2d (strided={strided})")
    _within_one_unit(two, exact, ulp, "reverse, then LayerNorm2d")
    if strided:
        assert (wide[:, C:] == 3.0).all()


@pytest.mark.parametrize("dt,code", [(d, c) for d, c, _ in DTYPES])
def test_rows_avgpool(dt, code):
    lib = _lib.lib()
    B, S, C = 3, 49, 512
    g = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randn(B, S, C, generator=g) + 2.0).cuda()   # means away from zero: the bound is relative per element
    feat = torch.full((B, C), float("nan"), device="cuda")
    _lib.check(lib.fvit_rows_avgpool(code, x.data_ptr(), feat.data_ptr(), B, S, C, _stream()), "fvit_rows_avgpool")
    # the existing route: the rows rounded into a 7 x 7 map (one window: row index == pixel index), then fvit_global_avgpool_cl
    m = x.to(dt)
    two = torch.empty_like(feat)
    _lib.check(lib.fvit_global_avgpool_cl(code, m.data_ptr(), two.data_ptr(), B, S, C, _stream()), "fvit_global_avgpool_cl")
    torch.cuda.synchronize()
    exact = m.double().cpu().mean(dim=1)
    for got, what in ((feat, "pool from the rows"), (two, "map, then pool")):
        rel = ((got.double().cpu() - exact).abs() / exact.abs()).max().item()
        print(f"{what}: max relative error {rel:.3e}")
        assert rel <= 1e-5, what
    assert torch.equal(feat, two)   # the same sums in the same order
    assert lib.fvit_rows_avgpool(_lib.FVIT_F32, x.data_ptr(), feat.data_ptr(), B, S, C, _stream()) != 0


def test_model_fused_routes_vs_unfused_plan():
    """faster_vit_0_224, batch 4, deploy plan: the fused routes against the same plan with them switched off, both against the reference's logits
    (the 1e-3 of the parity tests), and the fused plan bitwise repeatable."""
    gold = torch.from_numpy(load_golden("fvit0_224")["logits"][:4])
    model, _ = build_product_model("fvit0_224", "cuda")
    x = case_input("fvit0_224")[:4].cuda()
    model.switch_to_deploy(torch.float16)
    plan = model.__dict__["_deploy_plan"]
    assert plan.fuse_conv_ln2d == {64: True, 128: True} and plan.fuse_reverse_ln2d and plan.fuse_pool
    with torch.no_grad():
        model(x)   # packs the weights, sizes the workspaces
        _lib.prof_enable(True)
        try:
            fused = model(x).float().cpu()
            names = {r["name"] for r in _lib.prof_records()}
        finally:
            _lib.prof_enable(False)
        fused2 = model(x).float().cpu()
        plan.fuse_conv_ln2d, plan.fuse_reverse_ln2d, plan.fuse_pool = {64: False, 128: False}, False, False
        plain = model(x).float().cpu()
    # the fused kernels ran, and nothing fell back to the passes they replace
    assert {"conv3x3_c64_halo_kernel<ln>", "conv3x3_c128_band_kernel<ln>", "map_rows_ln_cl_kernel", "rows_avgpool_kernel"} <= names, names
    e_fused, e_plain = max_abs(fused, gold), max_abs(plain, gold)
    print(f"logits max-abs: fused vs unfused plan {max_abs(fused, plain):.3e}; vs reference: fused {e_fused:.3e}, unfused {e_plain:.3e}")
    assert e_fused < 1e-3 and e_plain < 1e-3
    assert torch.equal(fused, fused2)

