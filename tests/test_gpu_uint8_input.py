"""uint8 images on the GPU (needs an MI355X): the three stem kernels' uint8 instances, fvit_image_normalize_u8, and every public
entry point that takes an image.

The contract is ``f(u8) == f(table[u8])``, bit for bit, where table is the fp32 normalisation of tests/test_input_norm_cpu.py and the float image is
in the SAME memory layout.  Two kinds of kernel test:

* exact: bytes in {0, 1, 2}, scale = (1, -1, 2), shift = -scale, so that every normalised value is an integer in {-2 .. 2}, different per channel, and
  a raw 0 is NOT a normalised 0 (a kernel that pads before it normalises is wrong by whole integers); integer weights and bias of
  tests/conv_refs.stem_int_inputs; every sum asserted <= INT_LIMIT on the CPU; the result EQUALS the float64 reference;
* same bits: ImageNet constants, random bytes with 0 and 255 forced into corners and borders; the uint8 entry point EQUALS the float entry point on
  the table image (general gather against general gather, HWC gather against the fp32 NHWC3 gather), guards intact, a second call the same bits.

Formats: planar; channels-last (the decoder's HWC); a planar crop inside a larger tensor filled with 255 that starts at an odd address; a
channels-last crop.  Sizes: tests/conv_refs.STEM_IMAGES (+ 2 x 67 x 131 on 8 workgroups for the fused kernel): W * 3 mod 4 = 3, 0, 2, 3, 1."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, hat_runtime
from fastervit_amd.inference import evaluate
from tests import conv_launch as L
from tests import conv_refs as R
from tests.backbone_cases import BACKBONE_CASES, make_mask
from tests.cases import CASES, SEED
from tests.synth import synth_state_dict
from tests.test_input_norm_cpu import MEAN, STD, table
from tests.util import tuned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = ["planar", "hwc", "planar_crop", "hwc_crop"]
DTYPES = R.OPERAND_DTYPES
INT_SCALE, INT_SHIFT = (1.0, -1.0, 2.0), (-1.0, 1.0, -2.0)
FUSED_BIG = (2, 67, 131)


def _kernel_cases():
    out = []
    for kernel in ("stem_conv", "stem_conv_px", "stem_fused"):
        for shape in R.STEM_IMAGES + ([FUSED_BIG] if kernel == "stem_fused" else []):
            for fmt in FORMATS:
                for n3 in ((0, 1) if kernel == "stem_fused" else (None,)):
                    knobs = () if n3 is None else ((("stem_fused_grid", 8),) if shape == FUSED_BIG else ()) + (("stem_nhwc3", n3),)
                    out.append((kernel, shape, fmt, knobs))
    return out


KERNEL_CASES = _kernel_cases()


def _kid(c):
    kernel, (B, H, W), fmt, knobs = c
    return f"{kernel}-{B}x{H}x{W}-{fmt}" + "".join(f"-{k.replace('stem_', '')}{v}" for k, v in knobs)


def norm_array(scale, shift):
    return (ctypes.c_float * (2 * len(scale)))(*scale, *shift)


def lookup(tab: np.ndarray, u8: torch.Tensor) -> torch.Tensor:
    """table[u8]: the fp32 image (B, C, H, W) a uint8 image stands for (CPU)."""
    t = torch.from_numpy(tab)
    return torch.stack([t[c][u8[:, c].long()] for c in range(u8.shape[1])], dim=1)


def place(t: torch.Tensor, fmt: str) -> torch.Tensor:
    """The CPU image (B, C, H, W) on the device in one of FORMATS; the surroundings of a crop hold 255 (uint8) or NaN (float)."""
    B, C, H, W = t.shape
    fill = 255 if t.dtype == torch.uint8 else float("nan")
    if fmt == "planar":
        return t.to(DEV).contiguous()
    if fmt == "hwc":
        return t.to(DEV).contiguous(memory_format=torch.channels_last) if C > 1 else t.to(DEV).contiguous()
    x0 = 2 if W % 2 else 3                                                  # 1 + (W + 5) + x0 is odd: the view starts at an odd element
    if fmt == "planar_crop":
        buf = torch.full((B * C * (H + 3) * (W + 5) + 1,), fill, dtype=t.dtype, device=DEV)
        view = buf[1:].view(B, C, H + 3, W + 5)[:, :, 1:1 + H, x0:x0 + W]
        if t.dtype == torch.uint8:
            assert view.data_ptr() % 2 == 1
    else:
        buf = torch.full((B, H + 3, W + 5, C), fill, dtype=t.dtype, device=DEV)
        view = buf[:, 1:1 + H, x0:x0 + W, :].permute(0, 3, 1, 2)
    view.copy_(t.to(DEV))
    return view


def launch(kernel, x, dt, w, knobs=(), norm=None):
    """One stem launch through the C ABI (the uint8 entry point for a uint8 image); the Guarded output."""
    lib, (B, _, H, W) = _lib.lib(), x.shape
    u8 = x.dtype == torch.uint8
    view = hat_runtime._image_view(x)
    H1, W1 = R.out_size(H, 2), R.out_size(W, 2)
    tail = (norm,) if u8 else ()
    with tuned(**dict(knobs)) if knobs else contextlib.nullcontext():
        if kernel == "stem_fused":
            out = L.Guarded((B, R.out_size(H1, 2), R.out_size(W1, 2), 64), dt)
            fn = lib.fvit_stem_fused_u8 if u8 else lib.fvit_stem_fused
            rc = fn(L.CODE[dt], ctypes.byref(view), w["w1"][0].data_ptr(), w["b1"].data_ptr(), w["w2"].data_ptr(), w["b2"].data_ptr(), out.ptr(), B, H, W,
                    L.stream(), *tail)
        elif kernel == "stem_conv_px":
            out = L.Guarded((B, H1, W1, 64), dt)
            fn = lib.fvit_stem_conv3x3s2_px_u8 if u8 else lib.fvit_stem_conv3x3s2_px
            rc = fn(L.CODE[dt], ctypes.byref(view), w["w1"][0].data_ptr(), w["w1"][1].data_ptr(), w["b1"].data_ptr(), out.ptr(), B, H, W, L.stream(), *tail)
        else:
            out = L.Guarded((B, H1, W1, 64), dt)
            fn = lib.fvit_stem_conv3x3s2_u8 if u8 else lib.fvit_stem_conv3x3s2
            rc = fn(L.CODE[dt], ctypes.byref(view), w["w1"][0].data_ptr(), w["b1"].data_ptr(), out.ptr(), B, H, W, L.stream(), *tail)
        _lib.check(rc, kernel)
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out


def device_weights(inp, dt):
    return dict(w1=L._stem_w1(inp.w1, dt), b1=inp.b1.to(DEV), w2=inp.w2.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV), b2=inp.b2.to(DEV))


def _case(kernel, shape):
    return R.StemCase(kernel, *shape, "f32_nchw", ())


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(kernel, shape):
    """(uint8 image, StemInputs on its normalised values, float64 reference): computed once per kernel and size, shared by formats and dtypes."""
    c = _case(kernel, shape)
    base = R.stem_int_inputs(c)                                             # the integer weights and biases of the float tests (and their own checks)
    g = R.gen(R._seed(c) + 40)
    u8 = torch.randint(0, 3, (c.B, 3, c.H, c.W), generator=g, dtype=torch.uint8)
    u8[:, :, 0, 0], u8[:, :, -1, -1], u8[:, :, 0, -1], u8[:, :, -1, 0] = 0, 0, 0, 0   # raw zeros where the padding is: they normalise to -scale
    img = lookup(table(INT_SCALE, INT_SHIFT), u8)
    assert torch.equal(img, img.round()) and sorted(img.unique().tolist()) == [-2.0, -1.0, 0.0, 1.0, 2.0]
    assert all(img[:, ch, 0, 0].abs().min().item() > 0 for ch in range(3))
    inp = R.StemInputs(img, torch.float16, base.w1, base.b1, base.w2, base.b2)
    c1 = inp.conv1()
    mid = R.conv3x3.finish(R.conv3x3.presum(c1, R.F64), c1, 1, False, R.F64)
    R._assert_int(R.conv3x3.presum(c1, R.F64), "conv1 sum")
    R._assert_int(mid, "conv1 output")
    if kernel == "stem_fused":
        R._assert_int(R.conv3x3.presum(R.Inputs(mid, [inp.w2], inp.b2, 2), R.F64), "conv2 sum")
        R._assert_int(R.stem_fused.exact(inp), "conv2 output")
    return u8, inp, R.stem_ref(c).exact(inp)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_kid)
def test_uint8_stem_equals_the_integer_reference(case, dt):
    kernel, shape, fmt, knobs = case
    u8, inp, ref = exact_case(kernel, shape)
    out = launch(kernel, place(u8, fmt), dt, device_weights(inp, dt), knobs, norm_array(INT_SCALE, INT_SHIFT))
    assert torch.equal(out.map.cpu().to(R.F64), ref)


# ---- 2. the float kernel's bits ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_case(kernel, shape):
    c = _case(kernel, shape)
    g = R.gen(R._seed(c) + 41)
    u8 = torch.randint(0, 256, (c.B, 3, c.H, c.W), generator=g, dtype=torch.uint8)
    u8[:, :, 0, :], u8[:, :, -1, :] = 0, 255
    u8[:, :, 1:-1, 0], u8[:, :, 1:-1, -1] = 255, 0
    u8[0, :, 0, 0], u8[0, :, 0, -1], u8[0, :, -1, 0], u8[0, :, -1, -1] = 255, 0, 255, 0
    u8[1, :, 0, 0], u8[1, :, 0, -1], u8[1, :, -1, 0], u8[1, :, -1, -1] = 0, 255, 0, 255
    scale, shift = hat_runtime.input_norm_constants(MEAN, STD, 3)
    return u8, lookup(table(scale, shift), u8), norm_array(scale, shift)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=_kid)
def test_uint8_stem_has_the_float_kernels_bits(case, dt):
    kernel, shape, fmt, knobs = case
    u8, img, norm = value_case(kernel, shape)
    w = device_weights(R.stem_value_inputs(_case(kernel, shape), dt), dt)
    xu = place(u8, fmt)
    got = launch(kernel, xu, dt, w, knobs, norm)
    want = launch(kernel, place(img, fmt), dt, w, knobs)                      # the float entry point, same layout, same knobs
    assert not torch.isnan(want.map.float()).any()
    assert torch.equal(got.map, want.map)
    assert torch.equal(launch(kernel, xu, dt, w, knobs, norm).map, got.map)   # a repeated call


# ---- 3. fvit_image_normalize_u8 ----------------------------------------------------------------------------------------------------------------
NORM_CONSTANTS = {1: ((0.4,), (0.3,)), 3: (MEAN, STD), 4: ((0.1, 0.2, 0.3, 0.4), (0.5, 0.6, 0.7, 0.8))}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("chans", [1, 3, 4])
@pytest.mark.parametrize("shape", [(2, 7, 5), (3, 30, 22), (1, 51, 37)], ids=lambda s: "x".join(map(str, s)))
def test_image_normalize_u8_equals_the_table(shape, chans, fmt, masked):
    B, H, W = shape
    g = R.gen(5000 + 7 * H + chans)
    u8 = torch.randint(0, 256, (B, chans, H, W), generator=g, dtype=torch.uint8)
    u8[:, :, 0, 0], u8[:, :, -1, -1] = 0, 255
    scale, shift = hat_runtime.input_norm_constants(*NORM_CONSTANTS[chans], chans)
    want = lookup(table(scale, shift), u8)
    mask = None
    if masked:
        mask = torch.rand(B, H, W, generator=g) < 0.3
        mask[:, -1, :] = True
        want = want * (~mask)[:, None].float()                                # masked pixels exactly 0 (no -0, no NaN: the values are finite)
        want[mask[:, None].expand_as(want)] = 0.0
    x = place(u8, fmt)
    cl = fmt.startswith("hwc") and chans > 1
    # the output between two NaN guard rows; channels-last input -> channels-last output
    out = L.Guarded((B, H, W, chans) if cl else (B, chans, H, W), torch.float32)
    dst = out.map.permute(0, 3, 1, 2) if cl else out.map
    got = hat_runtime.normalize_u8(x, norm_array(scale, shift), mask.to(DEV) if masked else None, out=dst)
    torch.cuda.synchronize()
    assert got is dst and out.guards_intact()
    assert torch.equal(dst.cpu(), want) and not torch.signbit(dst.cpu()[want == 0]).any()
    # without ``out``: a new tensor in the input's memory format
    fresh = hat_runtime.normalize_u8(x, norm_array(scale, shift), mask.to(DEV) if masked else None)
    assert torch.equal(fresh.cpu(), want)
    assert fresh.is_contiguous(memory_format=torch.channels_last) if cl else fresh.is_contiguous()


# ---- 4. models ---------------------------------------------------------------------------------------------------------------------------------
_SMALL64 = dict(depths=[1, 1, 2, 1], num_heads=[1, 1, 2, 4], dim=32, in_dim=64)
MODELS = {
    "fvit0_fused_stem": dict(entry="faster_vit_0_224", kwargs={}, family="init", precise=False, symbol="fvit_stem_fused_u8"),
    # dim = 32 is carried as 64 padded channels, so this stem fits the fused kernel too: the plan's switch (FVIT_NO_FUSED_STEM) selects the branch under test
    "in64_stem_conv": dict(entry="faster_vit_0_224", kwargs=_SMALL64, family="stress", precise=False, symbol="fvit_stem_conv3x3s2_u8", fused_stem=False),
    "in64_precise_px": dict(entry="faster_vit_0_224", kwargs=_SMALL64, family="stress", precise=True, symbol="fvit_stem_conv3x3s2_px_u8"),
    "tiny_in16_unfused": dict(entry=CASES["tiny_d40"]["entry"], kwargs=CASES["tiny_d40"]["kwargs"], family="stress", precise=False,
                              symbol="fvit_image_normalize_u8"),
}


def _model(spec):
    m = fastervit_amd.create_model(spec["entry"], **spec["kwargs"]).eval()
    m.load_state_dict(synth_state_dict(m.state_dict(), SEED, spec["family"]), strict=True)
    return m.to(DEV).requires_grad_(False)


def _deploy(m, spec):
    if spec["precise"]:
        m.set_hat_operand_dtype("f16x3")
    m.switch_to_deploy()
    m.__dict__["_deploy_plan"].precise = spec["precise"]
    m.__dict__["_deploy_plan"].fused_stem = spec.get("fused_stem", True)
    return m


def _images(batch=2, hw=(224, 224), seed=0):
    g = R.gen(777 + seed)
    u8 = torch.randint(0, 256, (batch, 3, *hw), generator=g, dtype=torch.uint8)
    u8[:, :, 0, :], u8[:, :, :, -1] = 0, 255
    scale, shift = hat_runtime.input_norm_constants(MEAN, STD, 3)
    return u8, lookup(table(scale, shift), u8)


@contextlib.contextmanager
def _repeatable_module_mode():
    """Module mode runs the conv side on MIOpen's fp32 convolutions, whose default algorithms are not bit-repeatable run to run (measured here: the same
    float image twice through faster_vit_0_224 differs by 9e-5 at the logits, through its level-2 Downsample conv by 4e-7; tests/test_gpu_determinism.py).
    With the deterministic algorithms requested, as tests/test_gpu_backbone_backward.py does, f(x) == f(x) holds and f(u8) == f(table[u8]) can be asked."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = det


@contextlib.contextmanager
def _count_calls(symbol):
    """Counts the calls of one entry point of the loaded library (the route a forward took)."""
    lib, n = _lib.lib(), [0]
    fn = getattr(lib, symbol)

    def counted(*a):
        n[0] += 1
        return fn(*a)
    setattr(lib, symbol, counted)
    try:
        yield n
    finally:
        setattr(lib, symbol, fn)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_on_uint8_equals_model_on_the_table_image(name):
    spec = MODELS[name]
    model = _model(spec)
    u8, img = _images()
    with torch.no_grad():
        for fmt in ("planar", "hwc"):
            xu, xf = place(u8, fmt), place(img, fmt)
            if not spec["precise"]:                                           # module mode: one normalisation pass, then the float path
                with _repeatable_module_mode():
                    with _count_calls("fvit_image_normalize_u8") as n:
                        got = model(xu)
                    assert n[0] == 1 and torch.equal(got, model(xf))
        _deploy(model, spec)
        for fmt in ("planar", "hwc"):
            xu, xf = place(u8, fmt), place(img, fmt)
            with _count_calls(spec["symbol"]) as n:
                got = model(xu)
            assert n[0] == 1, f"{name}: the deployed forward did not take {spec['symbol']}"
            want = model(xf)
            assert torch.isfinite(want).all() and torch.equal(got, want)


def test_runners_evaluate_and_constants_on_uint8():
    spec = MODELS["fvit0_fused_stem"]
    model = _deploy(_model(spec), spec)
    u8, img = _images()
    u8b, imgb = _images(seed=1)
    xu, xf = u8.to(DEV), img.to(DEV)
    with torch.no_grad():
        eager = model(xu).clone()
        assert torch.equal(eager, model(xf))
        eager1 = model(xu[:1]).clone()
        # a uint8 runner: uint8 static input, the eager bits at full and at short batch, other dtypes refused by name
        runner = model.compile_inference(xu)
        assert runner.static_x.dtype == torch.uint8
        assert torch.equal(runner(xu), eager)
        assert torch.equal(runner(xu[:1]), eager1)
        assert int(runner.static_x[1:].max()) == 0                            # short-batch padding is zero bytes
        with pytest.raises(RuntimeError, match=r"uint8.*float32"):
            runner(xf)
        # a float runner fed uint8: one normalisation pass into its static buffer
        frunner = model.compile_inference(xf)
        want = frunner(xf).clone()
        with _count_calls("fvit_image_normalize_u8") as n:
            got = frunner(xu).clone()
        assert n[0] == 1 and torch.equal(got, want) and torch.equal(got, eager)
        short = frunner(xu[:1]).clone()
        assert torch.equal(short, frunner(xf[:1]))
        # evaluate over a uint8 loader
        tgt = torch.tensor([1, 2])
        ev_u = evaluate(model, [(u8, tgt), (u8b, tgt)], DEV)
        last_u = ev_u[3].clone()
        ev_f = evaluate(model, [(img, tgt), (imgb, tgt)], DEV)
        assert ev_u[:3] == ev_f[:3] and ev_u[0] == 4 and torch.equal(last_u, ev_f[3])
        ev_r = evaluate(model, [(u8, tgt), (u8b, tgt)], DEV, runner=runner)
        assert ev_r[:3] == ev_f[:3] and torch.equal(ev_r[3], ev_f[3])
        # other constants: the next eager call uses them; the compiled runner keeps its own until recompile()
        mean2, std2 = (0.5, 0.4, 0.3), (0.25, 0.2, 0.3)
        model.set_input_norm(mean2, std2)
        other = model(xu).clone()
        assert not torch.equal(other, eager)
        assert torch.equal(other, model(lookup(table(*hat_runtime.input_norm_constants(mean2, std2, 3)), u8).to(DEV)))
        assert torch.equal(runner(xu), eager)
        runner.recompile()
        assert torch.equal(runner(xu), other)


# ---- 5. the detection backbone -----------------------------------------------------------------------------------------------------------------
class _Nested:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask


def test_backbone_on_uint8():
    case = BACKBONE_CASES["bb_tiny_odd"]
    m = fastervit_amd.build_fastervit(case["name"], **case["kwargs"])
    m.load_state_dict(synth_state_dict(m.state_dict(), SEED, case["family"]), strict=True)
    m = m.eval().to(DEV).requires_grad_(False)
    u8, img = _images(hw=case["hw"], seed=2)
    mask = make_mask(case["mask"], 2, *case["hw"])
    assert mask.any() and not mask.all()
    xu, xf, mk = u8.to(DEV), img.to(DEV), mask.to(DEV)
    padded = torch.where(mk[:, None], torch.zeros_like(xf), xf)              # a float NestedTensor's padded pixels are 0
    with torch.no_grad():
        for deployed in (False, True):
            if deployed:
                m.switch_to_deploy()
            with contextlib.nullcontext() if deployed else _repeatable_module_mode():
                got, want = m.forward_features(xu), m.forward_features(xf)
                gn, wn = m(_Nested(xu, mk)), m(_Nested(padded, mk))
            assert len(got) == len(want) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))
            assert sorted(gn) == sorted(wn) == [0, 1, 2]
            for k in gn:
                assert torch.equal(gn[k].tensors, wn[k].tensors) and torch.equal(gn[k].mask, wn[k].mask)
            assert not torch.equal(gn[0].tensors, got[0])                     # the mask mattered
