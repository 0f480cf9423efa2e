"""References, inputs and case tables for the 3x3 conv and stem kernels of csrc/fvit_conv_*.hip and csrc/fvit_stem.hip, shared by tests/test_conv_refs_cpu.py (the proof that the
references and the bar are fair and have teeth, no GPU), tests/test_gpu_conv_exact.py (integer inputs, exact equality) and
tests/test_gpu_conv_values.py (random inputs against the bar).  Plain PyTorch on the CPU, nothing else.

Maps are channels-last fp32 tensors (B, H, W, C) holding the values the kernel receives: already representable in the 16-bit operand type.  Weights
are (Cout, Cin, 3, 3) planes ``[hi]`` or ``[hi, lo]``, bias fp32.  ``conv3x3`` has, over the SAME inputs:

    exact(inp, act, res)     float64:  act(conv(x, hi + lo) + conv(x_lo, hi) + bias) + residual (+ residual_lo).  The lo.lo product is not part of the
                             contract (include/fvit_hip.h, FvitConvCall); the residual is added after the activation, in the wide type.
    plain32(inp, act, res)   the same with F.conv2d in float32.
    chunk32(inp, act, res)   an independent float32 evaluation: unfold, K permuted, accumulated in steps of 32 (the MFMA K step) by matmul.

act: 0 none, 1 ReLU, 2 erf-GELU.  A channel-padded map (cin_valid < Cin) contracts over its first cin_valid channels only.

The bar of every value comparison, per output element (``conv_bound``; u_T, sub_T, the factor 8 and ``bound`` itself are tests/backward_primitive_refs.py's):

    bound[i] = u_T * |exact[i]| + sub_T + 8 * e32 + 2^-24 * max|exact|  (+ G for act 2 on the 16-bit routes)        e32 = max_i |plain32[i] - exact[i]|

G is the largest absolute error of gelu_fast (the coefficients of csrc/fvit_common.h:180-194 transcribed below, evaluated in float64) against float64
erf-GELU on a grid of 1.6e6 points over [-GELU_RANGE, GELU_RANGE]; the value builders assert that no pre-activation value leaves that range.
Measured: G = 3.80e-5 (the header documents 5.4e-5 for the fp32 evaluation; scripts/fit_gelu.py is the derivation).

``stem_fused`` (both PatchEmbed convs in one kernel) narrows ONCE: ReLU(conv1 + b1) is rounded to the map type before conv2 -- phase A's LDS store,
the ``(T)y`` of stem_fused_kernel (csrc/fvit_stem.hip) in the contiguous-run gather of fp32 channels-last images and in the strided gather; phase B
accumulates in fp32 and rounds the result once (the ``(T)fmaxf`` of its epilogue).  ``exact`` is the float64 chain with that rounding.  A conv1 value within an fp32 rounding error of a
rounding boundary may legitimately land on the other side, so, as tests/fused_block_refs.py does for its chains, the bar's e32 term becomes

    F * e16          e16 = max_i |plain32[i] - exact[i]|,  plain32 = the float32 chain rounded at the same point

F (``STEM_F``) is twice the worst ratio max|variant - exact| / e16 over the other legitimate evaluations of the chain (``STEM_VARIANTS``: chunk32 for
both convs; conv1 in float64 and conv2 in float32; conv1 in float32 and conv2 in float64), measured on the CPU over all stem_fused value cases and
both map types by tests/test_conv_refs_cpu.py, plus 2 % and rounded up to one decimal.  Measured worst ratios: chunk32 1.684 (2 x 67 x 131, fp16: it
flips other boundary values than plain32 does), mid64 1.000, mid32 1.001  ->  F = 3.5.  e16 itself is 2.0e-7 .. 4.5e-7 where no conv1 value changed
sides in the float32 chain (the 7 x 5 images, most bf16 cases) and 5.9e-5 .. 2.5e-4 where one did: a kernel that flips a value in a case of the
first kind would exceed this bar at outputs near zero.  None of the cases here does (profiles/conv_exact_and_value_tests.log).

No term of any bar comes from kernel output.

The integer cases (``int_inputs``, ``stem_int_inputs``): x, residual and the lo planes in {-1, 0, 1}, bias in {-2 .. 2}, weights in {-1, 0, 1} with a
quarter of the entries non-zero; the lo weight image, a two-term input's in_lo and residual_lo are independent integer maps.  Every partial and final
sum is an integer of magnitude <= 256: exact in fp32, fp16 and bf16 for any summation order, so a kernel's output must EQUAL the integer reference.
Each builder asserts the <= 256 condition over the pre-activation sums and the final values."""
import collections
import functools

import torch
import torch.nn.functional as F

from tests.backward_primitive_refs import F32, F64, SUB_T, U_T, bound, gen, rounded, worst_ratio  # noqa: F401  (re-exported to the tests)

OPERAND_DTYPES = [torch.float16, torch.bfloat16]
INT_LIMIT = 256
GELU_RANGE = 8.0
GELU_DOCUMENTED = 5.4e-5
# csrc/fvit_common.h:183-191, highest power of u = z^2 first; every literal is an fp32 constant there
GELU_FAST_Q = (4.075095461e-08, -1.945139275e-06, 4.106515917e-05, -5.110726343e-04, 4.235583358e-03, -2.510324307e-02, 1.110798195e-01,
               -3.753151596e-01, 1.128268480e+00)
STEM_F = 3.5


def _f32(v: float) -> float:
    return torch.tensor(v, dtype=F32).item()


# ------------------------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------------------------
def gelu_erf(t):
    return 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))


def gelu_fast64(t, q=GELU_FAST_Q):
    """gelu_fast of csrc/fvit_common.h with its fp32 constants, every operation in float64 (the polynomial's own error, no rounding)."""
    t = t.to(F64)
    z = (t * _f32(0.70710678118654752)).clamp(-3.0, 3.0)
    u = z * z
    acc = torch.full_like(u, _f32(q[0]))
    for c in q[1:]:
        acc = acc * u + _f32(c)
    hx = 0.5 * t
    return hx * (z * acc) + hx


@functools.lru_cache(maxsize=None)
def gelu_fast_error() -> float:
    """G: max |gelu_fast - erf-GELU| over the grid, float64."""
    grid = torch.linspace(-GELU_RANGE, GELU_RANGE, 1_600_001, dtype=F64)
    return (gelu_fast64(grid) - gelu_erf(grid)).abs().max().item()


def activate(t, act, gelu=gelu_erf):
    return [lambda v: v, torch.relu, gelu][act](t)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# three statements of the 3x3 convolution, pad 1: x (B, H, W, C), w (Co, C, 3, 3) -> (B, Ho, Wo, Co)
# ------------------------------------------------------------------------------------------------------------------------------------------------
def out_size(n: int, stride: int) -> int:
    return (n - 1) // stride + 1


def conv_plain(x, w, stride, dtype):
    return F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), None, stride, 1).permute(0, 2, 3, 1)


def conv_chunk(x, w, stride, dtype=F32, step=32):
    """unfold, then the K = 9 C columns in a fixed permuted order, ``step`` at a time: acc += cols[idx] . w[idx]."""
    B, H, W, C = x.shape
    cols = F.unfold(x.to(dtype).permute(0, 3, 1, 2), 3, padding=1, stride=stride)            # (B, C * 9, L), row c * 9 + tap
    wm = w.to(dtype).reshape(w.shape[0], C * 9)
    perm = torch.randperm(C * 9, generator=gen(77 + C))
    acc = torch.zeros(B, cols.shape[2], w.shape[0], dtype=dtype)
    for k0 in range(0, C * 9, step):
        idx = perm[k0:k0 + step]
        acc = acc + cols[:, idx, :].transpose(1, 2) @ wm[:, idx].t()
    return acc.reshape(B, out_size(H, stride), out_size(W, stride), w.shape[0])


def conv_shifted(x, w, stride, dtype=F64, transpose_taps=False, swap_mask=False, drop_tap_at_corner=False, offset=0):
    """Nine shifted matmuls over a zero-padded copy: the statement ``exact`` is checked against, and the carrier of the mutants that need the taps apart."""
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    x, w = x.to(dtype), w.to(dtype)
    if swap_mask:            # the border test `y < H && x < W` written with H and W swapped: pixels with y >= W or x >= H count as padding
        x = x.clone()
        x[:, W:], x[:, :, H:] = 0, 0
    xp = torch.zeros(B, H + 3, W + 3, C, dtype=dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=dtype)
    for ky in range(3):
        for kx in range(3):
            wt = w[:, :, kx, ky] if transpose_taps else w[:, :, ky, kx]
            part = xp[:, ky + offset:ky + offset + stride * (Ho - 1) + 1:stride, kx + offset:kx + offset + stride * (Wo - 1) + 1:stride] @ wt.t()
            if drop_tap_at_corner and (ky, kx) == (1, 1):
                part[0, 0, 0] = 0
            out = out + part
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the conv with its epilogue
# ------------------------------------------------------------------------------------------------------------------------------------------------
class Inputs:
    """x, x_lo, res, res_lo: channels-last maps (or None); w: [hi] or [hi, lo]; bias fp32 (Co); cv: real input channels."""

    def __init__(self, x, w, bias, stride, cv=None, x_lo=None, res=None, res_lo=None):
        self.x, self.w, self.bias, self.stride, self.x_lo, self.res, self.res_lo = x, w, bias, stride, x_lo, res, res_lo
        self.cv = x.shape[-1] if cv is None else cv


class conv3x3:
    @staticmethod
    def presum(inp, dtype, conv=conv_plain, skip_lo_cols=0, **conv_opt):
        """conv(x, hi) + conv(x, lo) + conv(x_lo, hi) over the real channels, no bias."""
        cv = inp.cv
        x, ws = inp.x[..., :cv], [w[:, :cv] for w in inp.w]
        s = conv(x, ws[0], inp.stride, dtype, **conv_opt)
        if len(ws) == 2:
            lo = ws[1]
            if skip_lo_cols:
                lo = lo.clone()
                lo[-skip_lo_cols:] = 0
            s = s + conv(x, lo, inp.stride, dtype, **conv_opt)
        if inp.x_lo is not None:
            s = s + conv(inp.x_lo[..., :cv], ws[0], inp.stride, dtype, **conv_opt)
        return s

    @staticmethod
    def finish(s, inp, act, res, dtype, res_first=False, bias_after_act=False, gelu=gelu_erf):
        """act(s + bias) + residual; the two flags are the epilogue mutants."""
        r = None
        if res:
            r = inp.res.to(dtype) if inp.res_lo is None or res == "hi" else inp.res.to(dtype) + inp.res_lo.to(dtype)
        b = inp.bias.to(dtype) if inp.bias is not None else torch.zeros((), dtype=dtype)
        if bias_after_act:
            return activate(s, act, gelu) + b + (r if r is not None else 0)
        y = s + b
        if res_first and r is not None:
            return activate(y + r, act, gelu)
        y = activate(y, act, gelu)
        return y + r if r is not None else y

    @staticmethod
    def exact(inp, act=0, res=False, conv=conv_plain, conv_opt=None, skip_lo_cols=0, **epilogue):
        return conv3x3.finish(conv3x3.presum(inp, F64, conv, skip_lo_cols, **(conv_opt or {})), inp, act, res, F64, **epilogue)

    @staticmethod
    def plain32(inp, act=0, res=False):
        return conv3x3.finish(conv3x3.presum(inp, F32), inp, act, res, F32)

    @staticmethod
    def chunk32(inp, act=0, res=False):
        return conv3x3.finish(conv3x3.presum(inp, F32, conv_chunk), inp, act, res, F32)


def conv_bound(exact, plain32, out_dtype, act=0, fast_gelu=True):
    """The bar per element; ``fast_gelu``: the route's GELU is the gelu_fast polynomial (the 16-bit routes)."""
    return bound(exact, plain32, out_dtype) + (gelu_fast_error() if act == 2 and fast_gelu else 0.0)


def conv_ratio(got, exact, plain32, out_dtype, act=0, fast_gelu=True, bar=None) -> float:
    """max_i |got[i] - exact[i]| / bar[i]; inf when ``got`` holds a non-finite value."""
    got = got.detach().cpu().to(F64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - exact.to(F64)).abs()
    bar = conv_bound(exact, plain32, out_dtype, act, fast_gelu) if bar is None else bar
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    return ratio.max().item() if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the stem: an image (B, H, W, 3) channels-last here, whatever layout the kernel is handed
# ------------------------------------------------------------------------------------------------------------------------------------------------
class StemInputs:
    """img: the image as the kernel uses it (rounded to the map type; img_lo: what the px kernel splits off in registers), w1 [hi] or [hi, lo]
    (64, 3, 3, 3), b1; w2 (64, 64, 3, 3), b2 for the fused kernel; raw: the caller's tensor values (B, 3, H, W), what the GPU test uploads."""

    def __init__(self, raw, dt, w1, b1, w2=None, b2=None, px=False):
        self.raw, self.dt, self.w1, self.b1, self.w2, self.b2 = raw, dt, w1, b1, w2, b2
        img = raw.permute(0, 2, 3, 1)
        self.img = rounded(img, dt)
        self.img_lo = rounded(img - self.img, dt) if px else None

    def conv1(self):
        return Inputs(self.img, self.w1, self.b1, 2, x_lo=self.img_lo)


class stem_conv:
    """fvit_stem_conv3x3s2 / _px: ReLU(conv(img, w1) + b1), stride 2, one rounding to the map type."""

    @staticmethod
    def exact(inp, **mut):
        return conv3x3.exact(inp.conv1(), 1, **mut)

    @staticmethod
    def plain32(inp):
        return conv3x3.plain32(inp.conv1(), 1)

    @staticmethod
    def chunk32(inp):
        return conv3x3.chunk32(inp.conv1(), 1)


class stem_fused:
    """ReLU(conv2(round_T(ReLU(conv1(img) + b1))) + b2), both stride 2."""

    @staticmethod
    def chain(inp, dtype1, dtype2, conv=conv_plain, narrow=True):
        c1 = inp.conv1()
        mid = conv3x3.finish(conv3x3.presum(c1, dtype1, conv), c1, 1, False, dtype1)
        mid = mid.to(inp.dt) if narrow else mid
        c2 = Inputs(mid.to(dtype2), [inp.w2], inp.b2, 2)
        return conv3x3.finish(conv3x3.presum(c2, dtype2, conv), c2, 1, False, dtype2)

    @staticmethod
    def exact(inp, narrow=True):
        return stem_fused.chain(inp, F64, F64, narrow=narrow)

    @staticmethod
    def plain32(inp):
        return stem_fused.chain(inp, F32, F32)

    @staticmethod
    def bar(exact, plain32, out_dtype):
        e16 = (plain32.to(F64) - exact).abs().max().item()
        return bound(exact, exact, out_dtype) + STEM_F * e16            # bound(exact, exact): the rounding and 2^-24 * peak terms, e32 = 0


STEM_VARIANTS = {
    "chunk32": lambda inp: stem_fused.chain(inp, F32, F32, conv_chunk),
    "mid64": lambda inp: stem_fused.chain(inp, F64, F32),
    "mid32": lambda inp: stem_fused.chain(inp, F32, F64),
}


class layernorm2d:
    """fvit_layernorm2d_cl over the first Cv of C channels: x (n, C) with zero pad channels, w / b (C) zero there."""

    @staticmethod
    def exact(x, w, b, cv, eps):
        return F.layer_norm(x[:, :cv].to(F64), (cv,), w[:cv].to(F64), b[:cv].to(F64), eps)

    @staticmethod
    def plain32(x, w, b, cv, eps):
        x = x[:, :cv].to(F32)
        xc = x - x.mean(-1, keepdim=True)
        return xc * ((xc * xc).mean(-1, keepdim=True) + eps).rsqrt() * w[:cv] + b[:cv]


LN2D_CASES = [(64, 16), (128, 80), (256, 196), (448, 392)]
LN2D_PIXELS, LN2D_EPS = 2 * 9 * 7, 1e-6


def ln2d_inputs(C, cv, dt=torch.float16):
    g = gen(9000 + C + cv)
    x = torch.zeros(LN2D_PIXELS, C)
    x[:, :cv] = torch.randn(LN2D_PIXELS, cv, generator=g) * 2 + 0.3
    x[0, :cv] = 0.5                                                 # a constant row: variance exactly 0
    w, b = torch.zeros(C), torch.zeros(C)
    w[:cv] = torch.rand(cv, generator=g) + 0.5
    b[:cv] = torch.randn(cv, generator=g)
    return rounded(x, dt), w, b, _f32(LN2D_EPS)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------------------------------------------------------
# route: the name fvit_conv3x3_route_name must give; knobs: the fvit_tune settings that force it (tests.util.tuned); terms: weight terms;
# in_lo: a two-term input; out: "16" one plane, "lo" hi + lo planes, "f32" one fp32 map (the last two and in_lo: the px instances)
ConvCase = collections.namedtuple("ConvCase", "route B H W Ci cv Co stride terms knobs in_lo out")
T128, T64, T256 = "conv3x3_kernel<2,2,4>", "conv3x3_kernel<2,2,2>", "conv3x3_kernel<4,1,4>"
HALO, BAND, PATCH = "conv3x3_c64_halo_kernel", "conv3x3_c128_band_kernel", "conv3x3_kernel<2,2,4,patch>"
NO_HALO = (("conv_halo", 0),)                           # 64 -> 64 channels, stride 1, one term: the implicit GEMM instead of the halo kernel
PATCH_KNOBS = (("conv_patch_max_waste_pct", 100000),)


def _route(tile, px=False, dense=False, patch=False):
    return tile[:-1] + (",px" if px else "") + (",dense" if dense else "") + (",patch" if patch else "") + ">"


def case_id(c) -> str:
    knobs = "".join(f"-{k.replace('conv_', '').replace('stem_', '')}{v}" for k, v in c.knobs if (k, v) not in NO_HALO + PATCH_KNOBS)
    return (f"{c.route}-{c.B}x{c.H}x{c.W}-{c.Ci}" + (f"({c.cv})" if c.cv != c.Ci else "") + f"to{c.Co}-s{c.stride}-t{c.terms}" + knobs +
            ("-inlo" if c.in_lo else "") + (f"-{c.out}" if c.out != "16" else ""))


def _case(route, B, H, W, Ci, Co, stride=1, terms=1, knobs=(), cv=None, in_lo=False, out="16"):
    if route in (T64, T256) and (Ci, Co, stride, terms) == (64, 64, 1, 1):
        knobs = NO_HALO + tuple(knobs)
    return ConvCase(route, B, H, W, Ci, Ci if cv is None else cv, Co, stride, terms, tuple(knobs), in_lo, out)


# (B, H, W, stride): M = 351 -- a ragged last tile and tiles that straddle images; stride 2 on odd and even maps; single pixels and a single row
GEMM_MAPS = [(3, 9, 13, 1), (3, 9, 13, 2), (2, 8, 6, 2), (2, 1, 1, 1), (2, 1, 5, 1)]
# (tile, Cout, extra knobs): 128 x 128 tiles (192 channels: the ragged last N tile), 128 x 64 and 256 x 64 tiles (192 channels: three N tiles)
GEMM_TILES = [(T128, 128, ()), (T128, 192, (("conv_n128_ragged", 1),)), (T64, 64, ()), (T64, 192, (("conv_n128_ragged", 0),)),
              (T256, 64, (("conv64_variant", 1),)), (T256, 192, (("conv_n128_ragged", 0), ("conv64_variant", 1)))]
# (Cin, cin_valid): K steps straddle taps, non-empty zero tail.  376: one of the three multiples of 8 up to 448 (328, 376, 440) at which fp32 k * (1 / cv)
# falls below the integer k / cv, i.e. at which the + 0.5 of the dense-K tap computation (fvit_conv_gemm.hip, stage_x) decides the tap
DENSE_CV = [(64, 8), (64, 24), (64, 40), (128, 72), (128, 104), (256, 200), (448, 392), (448, 376)]
PX_FORMS = [(in_lo, out) for in_lo in (False, True) for out in ("16", "lo", "f32")]


def _gemm_cases():
    cases = []
    for tile, Co, extra in GEMM_TILES:
        for i, (B, H, W, s) in enumerate(GEMM_MAPS):
            cases.append(_case(tile, B, H, W, 64, Co, s, 1 + i % 2, extra))
        for Ci, terms in ((128, 2), (448, 1)):
            cases.append(_case(tile, 3, 9, 13, Ci, Co, 1, terms, extra))
    for tile, Co, extra in GEMM_TILES[:4]:
        for i, (Ci, cv) in enumerate(DENSE_CV):
            B, H, W, s = GEMM_MAPS[0] if i % 3 else GEMM_MAPS[1 + (i // 3) % 2]
            cases.append(_case(_route(tile, dense=True), B, H, W, Ci, Co, s, 1 + (i + (Co == 192)) % 2, extra, cv=cv))
    for tile, Co in ((T128, 128), (T64, 64)):
        for j, (in_lo, out) in enumerate(PX_FORMS):
            B, H, W, s = GEMM_MAPS[j % 3]
            cases.append(_case(_route(tile, px=True), B, H, W, 64 if j % 2 else 128, Co, s, 2 if in_lo else 1 + j % 2, in_lo=in_lo, out=out))
            Ci, cv = DENSE_CV[(2 * j + (Co == 64)) % len(DENSE_CV)]
            cases.append(_case(_route(tile, px=True, dense=True), B, H, W, Ci, Co, s, 2 if in_lo else 1 + (j + 1) % 2, cv=cv, in_lo=in_lo, out=out))
    cases.append(_case(_route(T128, px=True), 3, 9, 13, 128, 192, 1, 2, in_lo=True, out="lo"))     # px on the ragged N tile
    return cases


GEMM_CASES = _gemm_cases()
# the halo kernel defers each tile's store into the next iteration: several tiles per workgroup (grid 1, 3) and one (512)
HALO_CASES = [_case(HALO, B, H, W, 64, 64, knobs=(("conv_halo_grid", grid),)) for B, H, W in ((2, 1, 1), (2, 3, 40), (2, 37, 5), (2, 17, 33))
              for grid in (1, 3, 512)]
BAND_CASES = [_case(BAND, 3, H, W, 128, 128, knobs=()) for H, W in ((1, 1), (9, 14), (33, 7), (5, 30), (20, 20))]
PATCH_CASES = ([_case(PATCH, 2, H, W, 64 if Co == 192 else 128, Co, 1, 2, PATCH_KNOBS) for H, W in ((1, 1), (8, 16), (9, 13), (24, 32))
                for Co in (128, 192, 256)] +
               [_case(_route(T128, px=True, patch=True), 2, H, W, 64, Co, 1, 2, PATCH_KNOBS, in_lo=True, out=out)
                for (H, W, Co, out) in ((9, 13, 128, "lo"), (8, 16, 192, "f32"), (24, 32, 128, "16"))])
CONV_CASES = GEMM_CASES + HALO_CASES + BAND_CASES + PATCH_CASES
# one or two per route and edge for the value tests (16-bit routes only: the px routes keep their 2e-6 x scale check, see tests/test_gpu_px.py)
VALUE_CASES = [c for c in CONV_CASES if c.out == "16" and not c.in_lo and "px" not in c.route and (
    (c.route in (T128, T64, T256) and (c.H, c.W, c.Ci) in ((9, 13, 64), (8, 6, 64), (9, 13, 448))) or
    ("dense" in c.route and c.cv in (24, 104, 376)) or
    (c.route == HALO and (c.H, dict(c.knobs)["conv_halo_grid"]) in ((17, 3), (3, 1), (37, 512))) or
    (c.route == BAND and c.H in (9, 33, 5)) or (c.route == PATCH and (c.H, c.Co) in ((9, 192), (24, 128), (8, 256))))]
# the px forms whose references the CPU test also holds to the bar (fp32 and two-plane outputs: u_T = 0)
PX_VALUE_CASES = [c for c in CONV_CASES if c.out != "16" and c.H == 9]

# the stem: (B, H, W, input format); crop: fp32 NCHW inside a larger tensor (non-trivial batch and row strides through FvitMapView)
STEM_FORMATS = ["f32_nchw", "f32_nhwc", "f16_nhwc", "bf16_nchw", "crop"]
StemCase = collections.namedtuple("StemCase", "kernel B H W fmt knobs")
STEM_IMAGES = [(2, 7, 5), (2, 8, 8), (2, 30, 22), (2, 51, 37)]
STEM_CONV_CASES = [StemCase("stem_conv", B, H, W, fmt, ()) for B, H, W in STEM_IMAGES for fmt in STEM_FORMATS]
STEM_FUSED_CASES = ([StemCase("stem_fused", B, H, W, fmt, (("stem_nhwc3", n3),)) for B, H, W in STEM_IMAGES for fmt in STEM_FORMATS
                     for n3 in ((0, 1) if fmt == "f32_nhwc" else (1,))] +
                    # 18 tiles on 8 workgroups, ragged in both directions
                    [StemCase("stem_fused", 2, 67, 131, fmt, (("stem_fused_grid", 8), ("stem_nhwc3", n3))) for fmt, n3 in
                     (("f32_nchw", 1), ("f32_nhwc", 1), ("f32_nhwc", 0))])
STEM_PX_CASES = [StemCase("stem_conv_px", B, H, W, fmt, ()) for (B, H, W), fmt in zip(STEM_IMAGES, STEM_FORMATS)]
STEM_VALUE_CASES = ([c for c in STEM_CONV_CASES if (c.H, c.fmt) in ((7, "f32_nchw"), (30, "f16_nhwc"), (51, "crop"), (8, "bf16_nchw"))] + STEM_PX_CASES +
                    [c for c in STEM_FUSED_CASES if (c.H, c.fmt) in ((7, "f32_nhwc"), (8, "bf16_nchw"), (30, "f16_nhwc"), (51, "crop"), (51, "f32_nhwc"),
                                                                     (67, "f32_nchw"), (67, "f32_nhwc"))])
FORMAT_DTYPE = {"f32_nchw": F32, "f32_nhwc": F32, "f16_nhwc": torch.float16, "bf16_nchw": torch.bfloat16, "crop": F32}


def stem_id(c) -> str:
    return f"{c.kernel}-{c.B}x{c.H}x{c.W}-{c.fmt}" + "".join(f"-{k.replace('stem_', '')}{v}" for k, v in c.knobs)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _seed(c) -> int:
    return 10_000 + sum(int(v) * m for v, m in zip((c.B, c.H, c.W, getattr(c, "Ci", 3), getattr(c, "Co", 64), getattr(c, "stride", 2)), (1, 7, 31, 3, 5, 977)))


def _ints(shape, g, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _int_weight(shape, g):
    return _ints(shape, g) * (torch.rand(shape, generator=g) < 0.375).float()         # 3/8 kept x 2/3 non-zero = a quarter of the entries


def _assert_int(t, what):
    assert torch.equal(t, t.round()) and t.abs().max().item() <= INT_LIMIT, f"{what}: max |.| = {t.abs().max().item()}"


def int_inputs(c) -> Inputs:
    """The integer case of a conv case (module docstring); every epilogue the exact test runs is checked against the <= 256 condition here."""
    g = gen(_seed(c))
    Ho, Wo = out_size(c.H, c.stride), out_size(c.W, c.stride)
    x = _ints((c.B, c.H, c.W, c.Ci), g)
    x_lo = _ints((c.B, c.H, c.W, c.Ci), g) if c.in_lo else None
    w = [_int_weight((c.Co, c.Ci, 3, 3), g) for _ in range(c.terms)]
    for m in (x, x_lo):
        if m is not None:
            m[..., c.cv:] = 0
    for p in w:
        p[:, c.cv:] = 0
    px =c.out != "16" or c.in_lo or "px" in c.route
    inp = Inputs(x, w, _ints((c.Co,), g, -2, 2), c.stride, c.cv, x_lo, _ints((c.B, Ho, Wo, c.Co), g), _ints((c.B, Ho, Wo, c.Co), g) if px else None)
    s = conv3x3.presum(inp, F64)
    _assert_int(s, "pre-activation sum")
    for act in (0, 1):
        for res in (False, "hi", True):
            _assert_int(conv3x3.finish(s, inp, act, res, F64), f"act {act} res {res}")
    return inp


def value_inputs(c, dt) -> Inputs:
    """randn maps, weights randn / sqrt(9 cin_valid) split into ``terms`` planes, randn bias and residual: the scaling of the earlier conv tests."""
    g = gen(_seed(c) + 1)
    Ho, Wo = out_size(c.H, c.stride), out_size(c.W, c.stride)
    x = torch.randn(c.B, c.H, c.W, c.Ci, generator=g)
    w = torch.randn(c.Co, c.Ci, 3, 3, generator=g) / (9 * c.cv) ** 0.5
    x[..., c.cv:], w[:, c.cv:] = 0, 0
    hi = rounded(w, dt)
    ws = [hi, rounded(w - hi, dt)][:c.terms]
    xh = rounded(x, dt)
    px = c.out != "16" or c.in_lo
    r = torch.randn(c.B, Ho, Wo, c.Co, generator=g) * (3.0 if px else 1.0)
    rh = rounded(r, dt)
    inp = Inputs(xh, ws, torch.randn(c.Co, generator=g), c.stride, c.cv, rounded(x - xh, dt) if c.in_lo else None, rh, rounded(r - rh, dt) if px else None)
    assert (conv3x3.presum(inp, F64) + inp.bias).abs().max().item() < GELU_RANGE
    return inp


def _stem_raw(c, g, integer):
    raw = _ints((c.B, 3, c.H, c.W), g) if integer else torch.randn(c.B, 3, c.H, c.W, generator=g)
    return rounded(raw, FORMAT_DTYPE[c.fmt])                         # what a tensor of the format's type holds


def stem_int_inputs(c) -> StemInputs:
    g = gen(_seed(c) + 2)
    raw = _stem_raw(c, g, True)
    w1 = [_int_weight((64, 3, 3, 3), g) for _ in range(2 if c.kernel == "stem_conv_px" else 1)]
    inp = StemInputs(raw, torch.float16, w1, _ints((64,), g, -2, 2), _int_weight((64, 64, 3, 3), g), _ints((64,), g, -2, 2))
    c1 = inp.conv1()
    mid = conv3x3.finish(conv3x3.presum(c1, F64), c1, 1, False, F64)
    _assert_int(conv3x3.presum(c1, F64), "conv1 sum")
    _assert_int(mid, "conv1 output")
    if c.kernel == "stem_fused":
        _assert_int(conv3x3.presum(Inputs(mid, [inp.w2], inp.b2, 2), F64), "conv2 sum")
        _assert_int(stem_fused.exact(inp), "conv2 output")
    return inp


def stem_value_inputs(c, dt) -> StemInputs:
    g = gen(_seed(c) + 3)
    raw = _stem_raw(c, g, False)
    w1 = torch.randn(64, 3, 3, 3, generator=g) / 27 ** 0.5
    h1 = rounded(w1, dt)
    px = c.kernel == "stem_conv_px"
    b1 = torch.randn(64, generator=g)
    return StemInputs(raw, dt, [h1, rounded(w1 - h1, dt)][:2 if px else 1], b1, rounded(torch.randn(64, 64, 3, 3, generator=g) / 24, dt),
                      torch.randn(64, generator=g), px)


def stem_ref(c):
    return stem_fused if c.kernel == "stem_fused" else stem_conv
