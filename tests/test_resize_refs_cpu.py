"""The resize feature's yardsticks and host logic, without a GPU: the float64 restatement against PIL's recorded results, the
bound of tests/resize_refs.py against an fp32 evaluation (inside) and five wrong variants (outside), the size rules of ClassifierPreprocess /
DetectionPreprocess, the new ABI symbols, and every refusal that needs no device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from fastervit_amd import _lib, preprocess
from tests import resize_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_cases.npz")
KINDS = ("noise", "smooth", "mult8")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_restatement_matches_pil_to_one_level():
    """tests/golden/resize_cases.npz holds Image.resize results (Pillow 12.2.0): the restatement is never more than one level away, and differs on
    exactly the recorded share of bytes (0 - 4.6 %: ties decided by PIL's 22-bit fixed-point coefficients)."""
    assert os.path.getsize(GOLDEN) < 200 * 1024
    g = np.load(GOLDEN)
    sizes, shares = g["sizes"], g["diff_share"]
    assert len(sizes) >= 12
    for i, (H, W, rh, rw) in enumerate(sizes.tolist()):
        img = g[f"img_{i}"]
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        for f, name in enumerate(rr.FILTER_NAMES):
            pil = g[f"{name}_{i}"]
            assert pil.shape == (rh, rw, 3)
            diff = np.abs(pil.astype(np.int32) - rr.reference(img, rh, rw, name).out.astype(np.int32))
            assert diff.max() <= 1, (i, name)
            assert abs(float((diff > 0).mean()) - shares[i, f]) < 1e-12, (i, name)
    assert shares.max() < 0.06


@pytest.mark.parametrize("name", rr.FILTER_NAMES)
def test_fp32_evaluation_stays_inside_the_bound(name):
    """fp32 weights and sequential fp32 sums -- what a correct kernel computes -- leave no byte outside the bound, on every size as one two-axis call
    (widened bounds included) and as the calls the GPU test issues."""
    calls = set(rr.SIZES) | set(rr.value_calls(name))
    for (H, W, rh, rw) in sorted(calls):
        for kind in KINDS:
            img = rr.make_image(kind, H, W)
            ref = rr.reference(img, rh, rw, name)
            got = rr.restate(img, rh, rw, name, dtype=np.float32)
            assert not ref.outside(got).any(), (H, W, rh, rw, kind)
            assert not ref.outside(ref.out).any()


@pytest.mark.parametrize("name", rr.FILTER_NAMES)
def test_two_axis_cases_keep_the_widening_rare(name):
    """At most 5 % of a two-axis case's outputs may carry a widened bound (on the noise image the GPU test uses)."""
    two = [c for c in rr.value_calls(name) if rr.is_two_axis(c)]
    assert len(two) >= 4
    for (H, W, rh, rw) in two:
        ref = rr.reference(rr.make_image("noise", H, W), rh, rw, name)
        assert ref.widened <= rr.WIDEN_CAP, (H, W, rh, rw, ref.widened)
    for c in rr.value_calls(name):
        if not rr.is_two_axis(c):
            assert rr.reference(rr.make_image("noise", c[0], c[1]), c[2], c[3], name).widened == 0.0


def _share_outside(img, rh, rw, name, **variant):
    return float(rr.reference(img, rh, rw, name).outside(rr.restate(img, rh, rw, name, **variant)).mean())


# variant -> (keyword switches, [(filter, H, W, rh, rw)], least share of bytes it must leave outside the bound on each of them).  The least shares are the
# lower ends measured for the restatement's own wrong variants on noise images (a = -0.75: 21 - 93 %, no antialias: 21 - 100 %, no rounding between the
# passes: 0.3 - 24 %, vertical pass first: 1 - 33 %, centre without the + 0.5: 81 - 100 %), halved.
WRONG = {
    "a=-0.75": (dict(a=-0.75), [("bicubic", 37, 53, 16, 20), ("bicubic", 21, 34, 47, 71), ("bicubic", 17, 29, 40, 29)], 0.10),
    "no antialias": (dict(antialias=False), [("bilinear", 37, 53, 16, 20), ("bicubic", 37, 53, 16, 20), ("bilinear", 3, 130, 3, 9),
                                             ("bicubic", 96, 64, 48, 32)], 0.10),
    "one rounding": (dict(round_between=False), [("bicubic", 37, 53, 16, 20), ("bicubic", 21, 34, 47, 71), ("bilinear", 37, 53, 16, 20)], 0.0015),
    "vertical first": (dict(vertical_first=True), [("bicubic", 37, 53, 16, 20), ("bicubic", 21, 34, 47, 71), ("bilinear", 21, 34, 47, 71)], 0.005),
    "centre without +0.5": (dict(half=0.0), [("bilinear", 37, 53, 16, 20), ("bicubic", 21, 34, 47, 71), ("bilinear", 17, 29, 40, 29)], 0.40),
}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_wrong_variants_leave_the_bound(variant):
    kw, cases, least = WRONG[variant]
    for (name, H, W, rh, rw) in cases:
        share = _share_outside(rr.make_image("noise", H, W), rh, rw, name, **kw)
        print(f"{variant}: {name} {H}x{W}->{rh}x{rw}: {100 * share:.2f} % outside")
        assert share > least, (variant, name, H, W, rh, rw, share)


def test_classifier_size_rule():
    P = preprocess.ClassifierPreprocess
    assert P(224, 0.875).geometry(375, 500) == ((256, 341), (16, 58, 224, 224))     # (w, h) = (500, 375)
    assert P(224, 0.875).geometry(500, 375) == ((341, 256), (58, 16, 224, 224))     # (375, 500)
    assert P(384, 1.0).geometry(375, 500) == ((384, 512), (0, 64, 384, 384))
    rng = random.Random(1234)
    for _ in range(2000):
        img_size = rng.choice([96, 160, 224, 256, 384, 512])
        crop = rng.choice([0.875, 0.9, 0.95, 1.0, 0.8])
        h, w = rng.randint(17, 3000), rng.randint(17, 3000)
        (rh, rw), (top, left, ch, cw) = preprocess.classifier_geometry(h, w, img_size, crop)
        scale = int(np.floor(img_size / crop))
        assert min(rh, rw) == scale and (rh if h <= w else rw) == scale      # the short side equals scale
        assert (ch, cw) == (img_size, img_size)
        assert 0 <= top and top + ch <= rh and 0 <= left and left + cw <= rw
        assert abs((rh - ch) - 2 * top) <= 1 and abs((rw - cw) - 2 * left) <= 1


def test_detection_size_rule():
    P = preprocess.DetectionPreprocess()
    for (w, h), want in [((640, 480), (800, 1066)), ((1000, 300), (400, 1333)), ((333, 500), (1201, 800)), ((800, 1200), (1200, 800)),
                         ((427, 640), (1199, 800))]:
        assert P.output_size(h, w) == want, (w, h)
    rng = random.Random(4321)
    # aspect ratios up to 2 : 1: the long side is int(s hi / lo) with s = round(max_size lo / hi), at most max_size + hi / (2 lo)
    for _ in range(4000):
        size, max_size = rng.choice([(64, 96), (480, 800), (800, 1333), (1024, 2000), (800, None)])
        lo = rng.randint(40, 1600)
        hi = rng.randint(lo, 2 * lo)
        h, w = (lo, hi) if rng.random() < 0.5 else (hi, lo)
        oh, ow = preprocess.detection_size(h, w, size, max_size)
        eff = size if max_size is None or hi / lo * size <= max_size else int(round(max_size * lo / hi))
        if lo == eff:   # the unchanged-image branch: an image whose short side is already the size stays as it is, whatever its long side
            assert (oh, ow) == (h, w)
            continue
        assert min(oh, ow) == eff and (oh if h <= w else ow) == eff           # the short side equals the (possibly reduced) size
        assert max(oh, ow) == int(eff * hi / lo)
        if max_size is not None:
            assert max(oh, ow) <= max_size + 1


def test_from_model_reads_the_cfg():
    class M:
        default_cfg = {"input_size": (3, 384, 384), "crop_pct": 1.0, "interpolation": "bicubic"}

    p = preprocess.ClassifierPreprocess.from_model(M())
    assert (p.img_size, p.crop_pct, p.interpolation) == (384, 1.0, "bicubic")

    class N:
        default_cfg = None
        pretrained_cfg = {"input_size": (3, 224, 224), "crop_pct": 0.875, "interpolation": "bilinear"}

    p = preprocess.ClassifierPreprocess.from_model(N())
    assert (p.img_size, p.crop_pct, p.interpolation) == (224, 0.875, "bilinear")
    with pytest.raises(ValueError, match="default_cfg"):
        preprocess.ClassifierPreprocess.from_model(object())
    import fastervit_amd
    m = fastervit_amd.create_model("faster_vit_0_224", depths=[1, 1, 1, 1], dim=16, in_dim=16, num_heads=[1, 1, 2, 4])
    p = fastervit_amd.ClassifierPreprocess.from_model(m)
    assert (p.img_size, p.crop_pct, p.interpolation) == (224, 0.875, "bicubic")


def test_new_symbols_agree_at_abi_10(lib):
    """Header, binding and both library builds carry the two new entry points; the ABI version stays 10; the descriptor is 56 bytes on both sides."""
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    assert re.search(r"#define FVIT_ABI_VERSION 10\b", hdr) and _lib.FVIT_ABI_VERSION == 10 and lib.fvit_abi_version() == 10
    for sym in ("fvit_image_resize_u8", "fvit_image_resize_check"):
        assert re.search(r"\bint " + sym + r"\(", hdr) and sym in _lib.EXPORTED_SYMBOLS
        for so in ("libfvit_hip.so", "libfvit_hip_diag.so"):
            assert hasattr(ctypes.CDLL(os.path.join(_lib.CSRC_DIR, so)), sym), (so, sym)
    assert "fvit_resize.hip" in open(os.path.join(_lib.CSRC_DIR, "Makefile")).read()
    assert ctypes.sizeof(_lib.FvitResizeDesc) == 56 and _lib.FvitResizeDesc.H.offset == 16 and _lib.FvitResizeDesc.filter.offset == 48
    for code, text in re.findall(r"#define FVIT_RESIZE_E[A-Z]+ \((-\d+)\)\s*/\*\s*(.*?)\*/", hdr):
        assert int(code) in _lib.FVIT_RESIZE_REASONS, text
    assert len(_lib.FVIT_RESIZE_REASONS) == 7


def _desc(**kw):
    base = dict(src=0, row_stride=3 * 64, H=48, W=64, rh=24, rw=32, top=0, left=0, ch=24, cw=32, filter=_lib.FVIT_RESIZE_BICUBIC)
    base.update(kw)
    return _lib.FvitResizeDesc(**base)


REFUSALS = [
    ("size", dict(H=0)), ("size", dict(W=0)), ("size", dict(rh=0)), ("size", dict(rw=-3)), ("size", dict(ch=0)), ("size", dict(cw=0)),
    ("window", dict(top=1)), ("window", dict(left=-1)), ("window", dict(left=1)), ("window", dict(ch=25)),
    ("slot", dict(rh=48, rw=64, ch=41, cw=32)), ("slot", dict(rh=48, rw=64, ch=24, cw=49)),
    ("filter", dict(filter=0)), ("filter", dict(filter=3)),
    ("stride", dict(row_stride=3 * 64 - 1)),
    ("tap limit", dict(H=17 * 24, ch=24)),                                   # 17x bicubic vertically: 69 taps
    ("tap limit", dict(W=17 * 32, row_stride=3 * 17 * 32)),                  # 17x bicubic horizontally
    ("tap limit", dict(W=33 * 32, row_stride=3 * 33 * 32, filter=_lib.FVIT_RESIZE_BILINEAR)),   # 33x bilinear: 67 taps
    ("LDS limit", dict(H=24 * 24, filter=_lib.FVIT_RESIZE_BILINEAR)),        # 24x bilinear vertically: 49 taps, but 8 rows span 217 source rows
]


@pytest.mark.parametrize("reason,kw", REFUSALS)
def test_descriptor_query_refuses_by_name(lib, reason, kw):
    d = _desc(**kw)
    rc = lib.fvit_image_resize_check(ctypes.byref(d), 40, 48)
    assert rc < 0 and _lib.FVIT_RESIZE_REASONS[rc] == reason
    assert reason.encode() in lib.fvit_last_error()


def test_descriptor_query_accepts_the_supported_range(lib):
    ok = [dict(), dict(H=16 * 24, W=16 * 32, row_stride=3 * 16 * 32),                      # 16x bicubic on both axes: 65 taps, 177 rows
          dict(H=1, W=1, row_stride=3, rh=40, rw=48, ch=40, cw=48),                      # any upscale
          dict(H=21 * 24, filter=_lib.FVIT_RESIZE_BILINEAR),                             # 21x bilinear vertically: 190 rows
          dict(W=32 * 32, row_stride=3 * 32 * 32, filter=_lib.FVIT_RESIZE_BILINEAR),     # 32x bilinear horizontally: 65 taps
          dict(rh=48, rw=64, top=8, left=16, ch=40, cw=48), dict(row_stride=4096)]
    for kw in ok:
        assert lib.fvit_image_resize_check(ctypes.byref(_desc(**kw)), 40, 48) == 0, kw


def test_resize_batch_refusals_without_a_device(lib):
    """Bad inputs are refused by name before anything touches a device; a CPU destination raises (no CPU fallback)."""
    good = torch.zeros(48, 64, 3, dtype=torch.uint8)
    rb = preprocess.resize_batch
    with pytest.raises(ValueError, match="image 1: dtype torch.float32"):
        rb([good, torch.zeros(48, 64, 3)], [(24, 32)] * 2, filter="bicubic")
    with pytest.raises(ValueError, match=r"image 0: shape \(3, 48, 64\)"):
        rb([torch.zeros(3, 48, 64, dtype=torch.uint8)], [(24, 32)], filter="bicubic")
    with pytest.raises(ValueError, match="image 2: shape"):
        rb([good, good, torch.zeros(48, 64, 4, dtype=torch.uint8)], [(24, 32)] * 3, filter="bicubic")
    with pytest.raises(TypeError, match="image 0"):
        rb([np.zeros((4, 4, 3), np.uint8)], [(4, 4)], filter="bicubic")
    with pytest.raises(ValueError, match="unknown filter 'lanczos'"):
        rb([good], [(24, 32)], filter="lanczos")
    with pytest.raises(ValueError, match=r"image 1: refused \(window\)"):
        rb([good, good], [(24, 32)] * 2, [(0, 0, 24, 32), (4, 0, 24, 32)], filter="bilinear")
    with pytest.raises(ValueError, match=r"image 0: refused \(slot\)"):
        rb([good], [(24, 32)], filter="bilinear", out_size=(16, 32))
    with pytest.raises(ValueError, match=r"image 0: refused \(tap limit\)"):
        rb([good], [(2, 32)], filter="bicubic")
    with pytest.raises(ValueError, match=r"image 0: refused \(size\)"):
        rb([good], [(0, 32)], [(0, 0, 1, 1)], filter="bicubic")
    with pytest.raises(ValueError, match="fill=256"):
        rb([good], [(24, 32)], filter="bicubic", fill=256)
    with pytest.raises(ValueError, match=r"out must be \(1, 3, Ho, Wo\) uint8"):
        rb([good], [(24, 32)], filter="bicubic", out=torch.zeros(1, 3, 24, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        rb([good], [(24, 32)], filter="bicubic", out=torch.zeros(1, 3, 24, 32, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        preprocess.ClassifierPreprocess(32, 0.875)([good], out=torch.zeros(1, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        preprocess.resize_launch(torch.zeros(56, dtype=torch.uint8), torch.zeros(1, 3, 24, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="crop_pct"):
        preprocess.ClassifierPreprocess(224, 1.5)


def test_preprocess_imports_neither_oracle_nor_pil():
    src = open(os.path.join(ROOT, "fastervit_amd", "preprocess.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|PIL)", src, re.M)
