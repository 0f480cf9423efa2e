"""The edge strip of transposed tiles in conv3x3_c64_halo_kernel (both instances) and stem_fused_kernel (all three gathers) (csrc/fvit_conv_halo.hip, csrc/fvit_stem.hip; geometry:
tests/conv_edge_geometry.py).  Needs an MI355X.

Three kinds of check, in fp16 and bf16:
* integer inputs (tests/conv_refs.py: every partial sum an integer of magnitude <= 256, exact in any summation order): the output EQUALS the reference, with
  NaN around every buffer (tests/conv_launch.py);
* fvit_tune "conv_edge_tiles" 1 against 0 on random data: the same bits, and a repeated launch the same bits again -- the strip changes which workgroup
  computes a pixel, not one product or the order of its sum;
* the tile count the driver reports ("conv_halo_debug") equals the restatement's, with the knob on and off.
A halo launch with GELU keeps the plain tiling whatever the knob says: hipcc contracts gelu_fast's last step differently in the epilogue's four unrolled row
copies, so a GELU map's bits depend on a pixel's row inside its tile, and a strip tile would change that row (measured: the parent's own output changes in
13 of 166 400 elements, all in channels 1 mod 8, when the image is rolled down by one row; the accumulators are the same bits).  The tile-count test
asserts that too, and the on / off test runs GELU launches like any other."""
import functools
import re

import pytest
import torch

from fastervit_amd import _lib, hat_runtime
from tests import conv_edge_geometry as G
from tests import conv_launch as L
from tests import conv_refs as R
from tests import test_gpu_uint8_input as U
from tests.util import tuned

pytestmark = pytest.mark.gpu
DTYPES = R.OPERAND_DTYPES
# one plain column + a strip of one full and one half tile; the flagship map; Wr = 5 and ragged H; the strip alone; Wr = 1; Wr = 9: no strip
HALO_SHAPES = [(2, 24, 24), (1, 56, 56), (2, 13, 21), (2, 20, 8), (1, 16, 17), (1, 9, 25)]
OFF = dict(conv_edge_tiles=0)


def _sid(s):
    return "x".join(map(str, s))


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- the halo conv ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _halo_int(shape):
    c = R._case(R.HALO, *shape, 64, 64)
    inp = R.int_inputs(c)
    return c, inp, {(act, res): R.conv3x3.exact(inp, act, res) for act in (0, 1) for res in (False, True)}


def _reported_tiles(capfd):
    found = re.findall(r"conv3x3_c64_halo_kernel\S*: grid \d+, tiles (\d+),", capfd.readouterr().err)
    assert len(found) == 1, found
    return int(found[0])


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", HALO_SHAPES, ids=_sid)
def test_halo_integer_case_and_tile_count(shape, dt, capfd):
    c, inp, want = _halo_int(shape)
    B, H, W = shape
    run = L.ConvRun(c, inp, dt)
    for edge in (1, 0):
        for act in (0, 1, 2):             # a GELU launch keeps the plain tiling: its bits depend on a pixel's row in its tile (fvit_conv_halo.hip, launch)
            capfd.readouterr()
            with tuned(conv_halo_debug=1, conv_edge_tiles=edge):
                got = run.run(act)["hi"]
            assert _reported_tiles(capfd) == B * G.tiles_per_image(H, W, edge and act != 2), (edge, act)
            assert act == 2 or torch.equal(got, want[act, False]), (edge, act)
    assert (G.tiles_per_image(H, W, 1) < G.tiles_per_image(H, W, 0)) == (shape != (1, 9, 25))
    for act in (0, 1):
        for res, in_place in ((False, False), (True, False), (True, True)):
            got = run.run(act, res, in_place)["hi"]
            assert torch.equal(got, want[act, res]), (act, res, in_place, (got - want[act, res]).abs().max().item(), int((got != want[act, res]).sum()))


def _halo_data(shape, dt):
    B, H, W = shape
    g = R.gen(4100 + 100 * H + W)
    x = torch.randn(B, H, W, 64, generator=g).to(dt).cuda()
    r = torch.randn(B, H, W, 64, generator=g).to(dt).cuda()
    wk = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dt).cuda()
    return x, r, wk, torch.randn(64, generator=g).cuda(), torch.zeros(256, dtype=dt, device="cuda")


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", HALO_SHAPES, ids=_sid)
def test_halo_strip_has_the_bits_of_the_plain_tiling(shape, dt):
    lib, (B, H, W) = _lib.lib(), shape
    x, r, wk, bias, zeros = _halo_data(shape, dt)

    def launch(act, res):
        """res: None, "out" (out of place) or "inplace"."""
        out = r.clone() if res == "inplace" else torch.full_like(x, L.NAN)
        rp = out.data_ptr() if res == "inplace" else (r.data_ptr() if res else None)
        _lib.check(lib.fvit_conv3x3_nhwc(L.CODE[dt], x.data_ptr(), wk.data_ptr(), bias.data_ptr(), rp, out.data_ptr(), B, H, W, 64, 64, 1, act,
                                         zeros.data_ptr(), L.stream()), "conv3x3")
        torch.cuda.synchronize()
        return out

    for act, res in ((2, "out"), (1, None), (0, "inplace"), (2, None)):
        on = launch(act, res)
        with tuned(**OFF):
            off = launch(act, res)
        assert torch.isfinite(on.float()).all() and same_bits(on, off), (act, res)
        assert same_bits(launch(act, res), on), (act, res)


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(2, 24, 24), (1, 56, 56)], ids=_sid)
def test_halo_ln_strip_has_the_bits_of_the_plain_tiling(shape, dt):
    lib, (B, H, W) = _lib.lib(), shape
    x, r, wk, bias, zeros = _halo_data(shape, dt)
    g = R.gen(4200 + H)
    lw, lb = (1.0 + 0.5 * torch.randn(64, generator=g)).cuda(), (0.5 * torch.randn(64, generator=g)).cuda()

    def launch():
        out = r.clone()   # in place on the residual, as the plan runs it
        _lib.check(lib.fvit_conv3x3_c64_ln2d(L.CODE[dt], x.data_ptr(), wk.data_ptr(), bias.data_ptr(), out.data_ptr(), out.data_ptr(), lw.data_ptr(),
                                             lb.data_ptr(), 1e-6, B, H, W, zeros.data_ptr(), L.stream()), "conv3x3_c64_ln2d")
        torch.cuda.synchronize()
        return out

    on = launch()
    with tuned(**OFF):
        off = launch()
    assert torch.isfinite(on.float()).all() and same_bits(on, off)
    assert same_bits(launch(), on)


# ---- the fused stem ------------------------------------------------------------------------------------------------------------------------------
# (B, Hi, Wi) -> final maps 24 x 24, 56 x 56 and 13 x 21
STEM_SHAPES = [(2, 96, 96), (1, 224, 224), (2, 52, 84)]
N3 = (("stem_nhwc3", 1),)
N3_OFF = N3 + (("conv_edge_tiles", 0),)


def test_stem_shapes_take_the_strip():
    for B, Hi, Wi in STEM_SHAPES:
        H2, W2 = R.out_size(R.out_size(Hi, 2), 2), R.out_size(R.out_size(Wi, 2), 2)
        assert (H2, W2) in ((24, 24), (56, 56), (13, 21)) and G.tiling(H2, W2)[2] > 0


@functools.lru_cache(maxsize=None)
def _stem_int(shape):
    c = R.StemCase("stem_fused", *shape, "f32_nchw", N3)
    inp = R.stem_int_inputs(c)
    return inp, R.stem_fused.exact(inp)


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("fmt", ["f32_nhwc", "f32_nchw"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_sid)
def test_stem_float_gathers_integer_case(shape, fmt, dt):
    inp, want = _stem_int(shape)
    for knobs in (N3, N3_OFF):
        got = L.run_stem(R.StemCase("stem_fused", *shape, fmt, knobs), inp, dt)
        assert torch.equal(got, want), (knobs, (got - want).abs().max().item(), int((got != want).sum()))


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_sid)
def test_stem_uint8_gather_integer_case(shape, dt):
    u8, inp, want = U.exact_case("stem_fused", shape)
    w, norm = U.device_weights(inp, dt), U.norm_array(U.INT_SCALE, U.INT_SHIFT)
    for knobs in (N3, N3_OFF):
        got = U.launch("stem_fused", U.place(u8, "hwc"), dt, w, knobs, norm)
        assert torch.equal(got.map.cpu().to(R.F64), want), knobs


@functools.lru_cache(maxsize=None)
def _stem_random(shape):
    """(random uint8 image, the fp32 image it stands for under the ImageNet constants, the constants)"""
    B, Hi, Wi = shape
    u8 = torch.randint(0, 256, (B, 3, Hi, Wi), generator=R.gen(4300 + Hi), dtype=torch.uint8)
    scale, shift = hat_runtime.input_norm_constants(U.MEAN, U.STD, 3)
    return u8, U.lookup(U.table(scale, shift), u8), U.norm_array(scale, shift)


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("gather", ["f32_nhwc", "f32_nchw", "u8_hwc"])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_sid)
def test_stem_strip_has_the_bits_of_the_plain_tiling(shape, gather, dt):
    u8, img, norm = _stem_random(shape)
    w = U.device_weights(R.stem_value_inputs(R.StemCase("stem_fused", *shape, "f32_nchw", ()), dt), dt)
    x = U.place(u8, "hwc") if gather == "u8_hwc" else U.place(img, "hwc" if gather == "f32_nhwc" else "planar")
    on = U.launch("stem_fused", x, dt, w, N3, norm).map
    off = U.launch("stem_fused", x, dt, w, N3_OFF, norm).map
    assert torch.isfinite(on.float()).all() and same_bits(on, off)
    assert same_bits(U.launch("stem_fused", x, dt, w, N3, norm).map, on)
