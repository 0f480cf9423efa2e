"""uint8 images, everything that needs no GPU: the C ABI additions, the arithmetic facts the contract rests on, the constants'
validation and defaults, and the refusals that fire before any kernel is launched.

The contract: ``model(u8) == model(normalise(u8))`` with normalise(u)[c] = fmaf((float)u, scale[c], shift[c]) in fp32,
scale[c] = fp32(1 / (255 std[c])), shift[c] = fp32(-mean[c] / std[c]).  ``table`` below is that function over all 256 bytes, evaluated as
float32(float64(u) * float64(scale) + float64(shift)): the float64 evaluation is exact for the ImageNet constants (checked with rationals here), so
its rounding is the fused multiply-add's."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, hat_runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fvit_stem_conv3x3s2_u8", "fvit_stem_conv3x3s2_px_u8", "fvit_stem_fused_u8", "fvit_image_normalize_u8")
MEAN, STD = hat_runtime.IMAGENET_MEAN, hat_runtime.IMAGENET_STD
_TINY = dict(depths=[1, 1, 2, 1], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)


def table(scale, shift) -> np.ndarray:
    """(C, 256) fp32: the normalised value of every byte of every channel."""
    u = np.arange(256, dtype=np.float64)[None, :]
    return (u * np.asarray(scale, dtype=np.float64)[:, None] + np.asarray(shift, dtype=np.float64)[:, None]).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_uint8_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    assert re.search(r"#define\s+FVIT_U8\s+3\b", hdr)
    assert re.search(r"#define\s+FVIT_ABI_VERSION\s+10\b", hdr)
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in _lib.EXPORTED_SYMBOLS
    # each stem form: the float entry point's argument list + the host pointer to the constants
    for s in NEW_SYMBOLS[:3]:
        decl = re.search(r"\bint\s+" + s + r"\s*\(([^;]*)\);", hdr).group(1)
        base = re.search(r"\bint\s+" + s[:-3] + r"\s*\(([^;]*)\);", hdr).group(1)
        norm = lambda a: [re.sub(r"\s+", " ", p).strip() for p in a.split(",")]   # noqa: E731
        assert norm(decl) == norm(base) + ["const float* norm"]
    assert _lib.FVIT_U8 == 3 and _lib.FVIT_U8 not in (_lib.FVIT_F32, _lib.FVIT_F16, _lib.FVIT_BF16)


def test_abi_version_and_map_view_are_unchanged(lib):
    assert _lib.FVIT_ABI_VERSION == 10 and lib.fvit_abi_version() == 10
    assert ctypes.sizeof(_lib.FvitMapView) == 48


def test_both_libraries_export_the_symbols(lib):
    for name in ("libfvit_hip.so", "libfvit_hip_diag.so"):
        handle = ctypes.CDLL(os.path.join(_lib.CSRC_DIR, name))
        for s in NEW_SYMBOLS:
            assert hasattr(handle, s), (name, s)


def test_fp64_evaluation_is_exact_for_the_imagenet_constants():
    scale, shift = hat_runtime.input_norm_constants(MEAN, STD, 3)
    tab = table(scale, shift)
    for c in range(3):
        assert scale[c] == float(np.float32(1.0 / (255.0 * STD[c]))) and shift[c] == float(np.float32(-MEAN[c] / STD[c]))
        fs, fh = Fraction(scale[c]), Fraction(shift[c])
        for u in range(256):
            exact = u * fs + fh
            as64 = float(u) * scale[c] + shift[c]                                   # float64 product and sum
            assert Fraction(as64) == exact, (c, u)                                   # no rounding happened: 768 pairs
            assert float(tab[c, u]) == float(np.float32(as64))


def test_table_against_the_usual_formulas():
    scale, shift = hat_runtime.input_norm_constants(MEAN, STD, 3)
    tab = torch.from_numpy(table(scale, shift))
    u = torch.arange(256, dtype=torch.float32)[None, :]
    mean, std = torch.tensor(MEAN, dtype=torch.float32)[:, None], torch.tensor(STD, dtype=torch.float32)[:, None]
    m255 = torch.tensor([v * 255 for v in MEAN], dtype=torch.float32)[:, None]
    s255 = torch.tensor([v * 255 for v in STD], dtype=torch.float32)[:, None]
    timm = (u - m255) / s255                               # the prefetching loader: fp32 tensors of mean * 255 and std * 255
    tv = (u / 255 - mean) / std                            # ToTensor + Normalize
    for other in (timm, tv):
        assert (tab - other).abs().max().item() <= 4.8e-7
        for dt in (torch.float16, torch.bfloat16):
            assert torch.equal(tab.to(dt), other.to(dt))   # all 768 entries: the 16-bit plans read the same operands


def test_set_input_norm_validation_and_default():
    m = fastervit_amd.create_model("faster_vit_0_224", **_TINY)
    ref = hat_runtime.input_norm_constants(MEAN, STD, 3)
    assert m.input_norm() == ref                                        # default_cfg of the variant: the ImageNet constants
    cfg = dict(m.default_cfg, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 0.125))
    m.default_cfg = cfg
    assert m.input_norm() == hat_runtime.input_norm_constants(cfg["mean"], cfg["std"], 3)   # the default follows default_cfg
    assert m.set_input_norm((0.1, 0.2, 0.3), (0.5, 0.6, 0.7)) is m
    sc, sf = m.input_norm()
    assert sc == tuple(float(np.float32(1.0 / (255.0 * s))) for s in (0.5, 0.6, 0.7))
    assert sf == tuple(float(np.float32(-a / s)) for a, s in zip((0.1, 0.2, 0.3), (0.5, 0.6, 0.7)))
    assert list(m.input_norm_array()) == list(sc) + list(sf)
    for mean, std in (((0.1, 0.2), (0.5, 0.6, 0.7)), ((0.1, 0.2, 0.3), (0.5, 0.6)), ((0.1, 0.2, 0.3), (0.5, 0.0, 0.7)), ((0.1, 0.2, 0.3), (0.5, -1.0, 0.7)),
                      ((0.1, 0.2, 0.3, 0.4), (0.5, 0.6, 0.7, 0.8))):
        with pytest.raises(ValueError):
            m.set_input_norm(mean, std)
    assert m.input_norm() == (sc, sf)                                   # a refused call changes nothing
    # in_chans decides the length; without a default_cfg that fits there is no default
    m4 = fastervit_amd.create_model("faster_vit_0_224", in_chans=4, **_TINY)
    m4.default_cfg = {}
    with pytest.raises(RuntimeError, match="set_input_norm"):
        m4.input_norm()
    m4.set_input_norm((0.1, 0.2, 0.3, 0.4), (0.5, 0.6, 0.7, 0.8))
    assert len(m4.input_norm()[0]) == 4
    bb = fastervit_amd.build_fastervit("faster_vit_0_224", **dict(_TINY, depths=[1, 1, 2, 2]))
    assert bb.input_norm() == ref
    with pytest.raises(ValueError):
        bb.set_input_norm((0.1,), (0.5,))


def test_cpu_uint8_tensor_raises_the_device_error():
    u8 = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    m = fastervit_amd.create_model("faster_vit_0_224", **_TINY).eval()
    bb = fastervit_amd.build_fastervit("faster_vit_0_224", **dict(_TINY, depths=[1, 1, 2, 2])).eval()
    with torch.no_grad():
        for call in (lambda: m(u8), lambda: m.forward_features(u8), lambda: bb.forward_features(u8),
                     lambda: hat_runtime.normalize_u8(u8, m.input_norm_array())):
            with pytest.raises(RuntimeError, match="HIP device"):
                call()
        m.switch_to_deploy()
        with pytest.raises(RuntimeError, match="HIP device"):
            m(u8)


def test_uint8_is_an_image_type_only():
    u8 = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="unsupported feature-map dtype"):
        hat_runtime._map_view(u8)                                       # a uint8 map never reaches a HAT stage
    assert torch.uint8 not in hat_runtime._DT
    v = hat_runtime._image_view(u8)
    assert v.dtype == _lib.FVIT_U8 and (v.stride_b, v.stride_c, v.stride_h, v.stride_w) == u8.stride()
    assert hat_runtime._image_view(u8.float()).dtype == _lib.FVIT_F32


def test_entry_points_refuse_the_other_image_type(lib):
    """The argument checks run before anything touches the device: a FVIT_U8 view on a float entry point names the _u8 one, and the other way round."""
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    norm = (ctypes.c_float * 6)(1, 1, 1, 0, 0, 0)
    u8v = _lib.FvitMapView(p, 3 * 64, 64, 8, 1, _lib.FVIT_U8, 0)
    f32v = _lib.FvitMapView(p, 3 * 64, 64, 8, 1, _lib.FVIT_F32, 0)
    float_calls = {
        "fvit_stem_conv3x3s2": lambda v: lib.fvit_stem_conv3x3s2(_lib.FVIT_F16, ctypes.byref(v), p, p, p, 1, 8, 8, None),
        "fvit_stem_conv3x3s2_px": lambda v: lib.fvit_stem_conv3x3s2_px(_lib.FVIT_F16, ctypes.byref(v), p, p, p, p, 1, 8, 8, None),
        "fvit_stem_fused": lambda v: lib.fvit_stem_fused(_lib.FVIT_F16, ctypes.byref(v), p, p, p, p, p, 1, 8, 8, None),
    }
    u8_calls = {
        "fvit_stem_conv3x3s2": lambda v, n: lib.fvit_stem_conv3x3s2_u8(_lib.FVIT_F16, ctypes.byref(v), p, p, p, 1, 8, 8, None, n),
        "fvit_stem_conv3x3s2_px": lambda v, n: lib.fvit_stem_conv3x3s2_px_u8(_lib.FVIT_F16, ctypes.byref(v), p, p, p, p, 1, 8, 8, None, n),
        "fvit_stem_fused": lambda v, n: lib.fvit_stem_fused_u8(_lib.FVIT_F16, ctypes.byref(v), p, p, p, p, p, 1, 8, 8, None, n),
    }
    for name, call in float_calls.items():
        assert call(u8v) == -1
        assert (name + "_u8").encode() in lib.fvit_last_error()
    for name, call in u8_calls.items():
        assert call(f32v, norm) == -1
        err = lib.fvit_last_error()
        assert (name + "_u8").encode() in err and b"FVIT_U8" in err
        assert call(u8v, None) == -1 and b"normalisation" in lib.fvit_last_error()
    assert lib.fvit_image_normalize_u8(ctypes.byref(f32v), p, 0, 1, 3, 8, 8, norm, None, None) == -1
    assert b"FVIT_U8" in lib.fvit_last_error()
    assert lib.fvit_image_normalize_u8(ctypes.byref(u8v), p, 0, 1, 17, 8, 8, norm, None, None) == -1     # more channels than the kernel carries constants for
