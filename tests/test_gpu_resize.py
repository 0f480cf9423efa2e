"""Resize + crop + pad of decoded uint8 images on the GPU (csrc/fvit_resize.hip through the C ABI, and fastervit_amd/preprocess.py on top of it),
held to the float64 restatement and the per-pixel bound of tests/resize_refs.py (tests/test_resize_refs_cpu.py shows that an fp32 evaluation meets
the bound on these very inputs and that five wrong variants do not).

Conventions: every source lives inside a larger buffer of 0xA5 bytes, every destination inside a buffer of 0x5A guard bytes that must stay as they are."""
import ctypes

import numpy as np
import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, preprocess
from tests import resize_refs as rr
from tests.backbone_cases import BACKBONE_CASES
from tests.cases import SEED
from tests.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PAD = 0x5A, 256
CODE = preprocess.FILTERS
_REFS = {}


def _ref(kind, H, W, rh, rw, name, seed=0):
    """(image, reference): computed once per case, shared by the tests and left unchanged."""
    key = (kind, H, W, rh, rw, name, seed)
    if key not in _REFS:
        img = rr.make_image(kind, H, W, seed)
        _REFS[key] = (img, rr.reference(img, rh, rw, name))
    return _REFS[key]


def _source(img: np.ndarray, extra_stride: int = 0) -> torch.Tensor:
    """The (H, W, 3) image on the device as a view into a buffer of 0xA5 bytes, rows ``3 W + extra_stride`` bytes apart."""
    H, W, _ = img.shape
    stride = 3 * W + extra_stride
    buf = torch.full((PAD + H * stride + PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(buf, (H, W, 3), (stride, 3, 1), PAD)
    view.copy_(torch.from_numpy(img).to(DEV))
    return view


class Dest:
    """A (B, 3, Ho, Wo) uint8 destination, planar or channels-last, whose slots are ``pitch`` >= 3 Ho Wo bytes apart inside a buffer of guard bytes."""

    def __init__(self, B, Ho, Wo, channels_last, gap=0):
        self.B, self.Ho, self.Wo = B, Ho, Wo
        self.pitch = 3 * Ho * Wo + gap
        self.buf = torch.full((PAD + B * self.pitch + PAD,), GUARD, dtype=torch.uint8, device=DEV)
        strides = (self.pitch, 1, 3 * Wo, 3) if channels_last else (self.pitch, Ho * Wo, Wo, 1)
        self.view = torch.as_strided(self.buf, (B, 3, Ho, Wo), strides, PAD)

    def guards_intact(self):
        b = self.buf.cpu()
        ok = bool((b[:PAD] == GUARD).all() and (b[PAD + self.B * self.pitch:] == GUARD).all())
        for i in range(self.B):
            ok = ok and bool((b[PAD + i * self.pitch + 3 * self.Ho * self.Wo:PAD + (i + 1) * self.pitch] == GUARD).all())
        return ok

    def hwc(self, i):
        """slot i as a (Ho, Wo, 3) numpy array"""
        return self.view[i].permute(1, 2, 0).cpu().numpy()


def _descs(sources, sizes, windows, name, out_size):
    arr = (_lib.FvitResizeDesc * len(sources))()
    for i, s in enumerate(sources):
        arr[i] = preprocess.make_descriptor(s.data_ptr(), s.shape[0], s.shape[1], s.stride(0), sizes[i], windows[i], CODE[name], out_size)
    return torch.frombuffer(arr, dtype=torch.uint8).clone().to(DEV)


def _abi(descs, dest: Dest, fill=0, mask=None):
    v = dest.view
    view = _lib.FvitMapView(data=v.data_ptr(), stride_b=v.stride(0), stride_c=v.stride(1), stride_h=v.stride(2), stride_w=v.stride(3), dtype=_lib.FVIT_U8)
    rc = _lib.lib().fvit_image_resize_u8(descs.data_ptr(), dest.B, ctypes.byref(view), dest.Ho, dest.Wo, fill, None if mask is None else mask.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().fvit_last_error()
    torch.cuda.synchronize()


def _held(got, ref, what):
    bad = ref.outside(got)
    err = np.abs(got.astype(np.float64) - ref.v)
    worst = float(np.where(err > 0, err / np.maximum(ref.bound, 1e-300), 0.0).max()) if got.size else 0.0   # (a same-size call has bound 0 and err 0)
    print(f"{what}: worst |err| / bound {worst:.4f}, {int((got != ref.out).sum())} of {got.size} bytes differ from the restatement")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes outside the bound (worst |err| / bound {worst:.3f})"


def _both_paths(img, ref, rh, rw, name, channels_last, window=None, extra_stride=0, what=""):
    """One image through the C ABI and through resize_batch (device source and CPU source), into a guarded destination."""
    window = window or (0, 0, rh, rw)
    ref = ref.crop(*window)
    ch, cw = window[2], window[3]
    src = _source(img, extra_stride)
    dest = Dest(1, ch, cw, channels_last, gap=5)
    _abi(_descs([src], [(rh, rw)], [window], name, (ch, cw)), dest)
    assert dest.guards_intact()
    got = dest.hwc(0)
    _held(got, ref, f"{what} abi")
    dest2 = Dest(1, ch, cw, channels_last, gap=5)
    preprocess.resize_batch([src], [(rh, rw)], [window], filter=name, out=dest2.view)
    torch.cuda.synchronize()
    assert dest2.guards_intact() and np.array_equal(dest2.hwc(0), got)
    out3 = preprocess.resize_batch([torch.from_numpy(img)], [(rh, rw)], [window], filter=name, channels_last=channels_last)   # pinned staging path
    assert np.array_equal(out3[0].permute(1, 2, 0).cpu().numpy(), got)
    return got


VALUE = [(name, call) for name in rr.FILTER_NAMES for call in rr.value_calls(name)]


@pytest.mark.parametrize("channels_last", [False, True], ids=["planar", "nhwc"])
@pytest.mark.parametrize("name,call", VALUE, ids=[f"{n}-{c[0]}x{c[1]}to{c[2]}x{c[3]}" for n, c in VALUE])
def test_values(name, call, channels_last):
    H, W, rh, rw = call
    img, ref = _ref("noise", H, W, rh, rw, name)
    _both_paths(img, ref, rh, rw, name, channels_last, what=f"{name} {H}x{W}->{rh}x{rw}")


@pytest.mark.parametrize("name", rr.FILTER_NAMES)
@pytest.mark.parametrize("kind", ["smooth", "mult8"])
def test_values_other_images(name, kind):
    for (H, W, rh, rw) in [(37, 53, 16, 20), (17, 29, 40, 29), (3, 130, 3, 9)]:
        img, ref = _ref(kind, H, W, rh, rw, name)
        _both_paths(img, ref, rh, rw, name, True, what=f"{name} {kind} {H}x{W}->{rh}x{rw}")


@pytest.mark.parametrize("name", rr.FILTER_NAMES)
def test_source_row_stride_and_inner_window(name):
    """A source whose rows are 3 W + 13 bytes apart; a window strictly inside the resized image whose first needed source row and column are not 0
    (37x53 -> 16x20, window rows 5 .. 12 and columns 7 .. 17: the first taps are source row 9 / column 15 or later)."""
    H, W, rh, rw = 37, 53, 16, 20
    img, ref = _ref("noise", H, W, rh, rw, name)
    for cl in (False, True):
        _both_paths(img, ref, rh, rw, name, cl, extra_stride=13, what=f"{name} stride")
        _both_paths(img, ref, rh, rw, name, cl, window=(5, 7, 8, 11), extra_stride=13, what=f"{name} window")
    k0_row = rr.coefficients(H, rh, name)[5][0]
    k0_col = rr.coefficients(W, rw, name)[7][0]
    assert k0_row > 0 and k0_col > 0
    # the window's bytes are exactly the full call's bytes at those positions: the crop is a selection
    src = _source(img)
    full = preprocess.resize_batch([src], [(rh, rw)], filter=name)[0]
    part = preprocess.resize_batch([src], [(rh, rw)], [(5, 7, 8, 11)], filter=name)[0]
    assert torch.equal(part, full[:, 5:13, 7:18])


@pytest.mark.parametrize("name", rr.FILTER_NAMES)
def test_exact_cases(name):
    # same size returns the source
    img = rr.make_image("noise", 23, 31)
    out = preprocess.resize_batch([_source(img, 7)], [(23, 31)], filter=name)
    assert torch.equal(out[0].permute(1, 2, 0).cpu(), torch.from_numpy(img))
    # constant images stay constant
    for value in (0, 1, 127, 254, 255):
        const = np.full((23, 31, 3), value, np.uint8)
        src = _source(const)
        for (rh, rw) in [(7, 9), (50, 40), (23, 9)]:
            out = preprocess.resize_batch([src], [(rh, rw)], filter=name, channels_last=False)
            assert out.shape == (1, 3, rh, rw) and bool((out == value).all()), (value, rh, rw)


def test_exact_bilinear_factors_of_two():
    """2x bilinear upscale of multiples of 16 and 2x downscale of multiples of 64: every weight and every sum is exact in fp32, no tie occurs.  The
    downscale is compared away from the one-pixel border, where the truncated support renormalises the weights to thirds."""
    rng = np.random.default_rng(5)
    up = (rng.integers(0, 16, (19, 27, 3)) * 16).astype(np.uint8)
    got = preprocess.resize_batch([_source(up)], [(38, 54)], filter="bilinear")[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got, rr.reference(up, 38, 54, "bilinear").out)
    down = (rng.integers(0, 4, (40, 52, 3)) * 64).astype(np.uint8)
    got = preprocess.resize_batch([_source(down)], [(20, 26)], filter="bilinear")[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got[1:-1, 1:-1], rr.reference(down, 20, 26, "bilinear").out[1:-1, 1:-1])


MIXED = [("bicubic", 1, 1, 4, 4), ("bilinear", 3, 130, 3, 9), ("bicubic", 37, 53, 16, 20), ("bicubic", 96, 64, 48, 32), ("bicubic", 160, 96, 10, 6)]


@pytest.mark.parametrize("channels_last", [False, True], ids=["planar", "nhwc"])
def test_one_launch_mixed_batch(channels_last):
    """Five images of different sizes (a 1x1 source, a 14x horizontal downscale, a 2x and a 16x bicubic downscale) and of both filters -- the filter
    is per descriptor -- in ONE launch, into slots of 48 x 72 that lie 37 guard bytes apart, with fill 7 and the mask."""
    Ho, Wo = 48, 72
    refs, srcs, sizes, windows = [], [], [], []
    for (name, H, W, rh, rw) in MIXED:
        img, ref = _ref("noise", H, W, rh, rw, name)
        refs.append(ref)
        srcs.append(_source(img, extra_stride=3))
        sizes.append((rh, rw))
        windows.append((0, 0, rh, rw))
    arr = (_lib.FvitResizeDesc * 5)()
    for i, (name, *_rest) in enumerate(MIXED):
        arr[i] = preprocess.make_descriptor(srcs[i].data_ptr(), srcs[i].shape[0], srcs[i].shape[1], srcs[i].stride(0), sizes[i], windows[i], CODE[name],
                                            (Ho, Wo))
    descs = torch.frombuffer(arr, dtype=torch.uint8).clone().to(DEV)
    dest = Dest(5, Ho, Wo, channels_last, gap=37)
    maskbuf = torch.full((PAD + 5 * Ho * Wo + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    mask = maskbuf[PAD:PAD + 5 * Ho * Wo].view(5, Ho, Wo)
    calls = [0]
    fn = _lib.lib().fvit_image_resize_u8

    def counted(*a):
        calls[0] += 1
        return fn(*a)
    _lib.lib().fvit_image_resize_u8 = counted
    try:
        _abi(descs, dest, fill=7, mask=mask)
    finally:
        _lib.lib().fvit_image_resize_u8 = fn
    assert calls[0] == 1 and dest.guards_intact()
    mb = maskbuf.cpu()
    assert bool((mb[:PAD] == GUARD).all() and (mb[-PAD:] == GUARD).all())
    for i, ref in enumerate(refs):
        rh, rw = sizes[i]
        got = dest.hwc(i)
        _held(got[:rh, :rw], ref, f"mixed image {i}")
        rest = np.ones((Ho, Wo), bool)
        rest[:rh, :rw] = False
        assert (got[rest] == 7).all(), i
        assert torch.equal(mask[i].cpu(), torch.from_numpy(rest.astype(np.uint8))), i
    # the same batch through resize_batch, with the bool mask
    out, m = preprocess.resize_batch(srcs, sizes, None, filter="bicubic", out_size=(Ho, Wo), mask=True, fill=7, channels_last=channels_last)
    assert m.dtype == torch.bool and m.shape == (5, Ho, Wo)
    for i in (0, 2, 3, 4):   # image 1 is bilinear above
        assert torch.equal(out[i], dest.view[i]) and torch.equal(m[i], mask[i].bool())


def test_repeatable_and_capturable():
    """A repeated call gives the same bytes; a captured call replayed with new source bytes under the same descriptors follows them."""
    H, W, rh, rw = 37, 53, 16, 20
    imgs = [rr.make_image("noise", H, W, seed) for seed in range(4)]
    src = _source(imgs[0])
    descs = _descs([src, src], [(rh, rw), (40, 29)], [(0, 0, rh, rw), (3, 2, 30, 20)], "bicubic", (32, 24))
    out = torch.full((2, 3, 32, 24), GUARD, dtype=torch.uint8, device=DEV)
    mask = torch.zeros((2, 32, 24), dtype=torch.bool, device=DEV)
    preprocess.resize_launch(descs, out, mask=mask, fill=9)
    first = out.clone()
    out.fill_(GUARD)
    preprocess.resize_launch(descs, out, mask=mask, fill=9)
    assert torch.equal(out, first)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        preprocess.resize_launch(descs, out, mask=mask, fill=9)   # warm-up on the capture stream
        with torch.cuda.graph(graph, stream=stream):
            preprocess.resize_launch(descs, out, mask=mask, fill=9)
    torch.cuda.current_stream().wait_stream(stream)
    for k in (1, 2, 3):
        src.copy_(torch.from_numpy(imgs[k]).to(DEV))
        out.fill_(GUARD)
        graph.replay()
        torch.cuda.synchronize()
        got = out[0, :, :rh, :rw].permute(1, 2, 0).cpu().numpy()
        _held(got, rr.reference(imgs[k], rh, rw, "bicubic"), f"replay {k}")
        want = torch.full_like(out, GUARD)
        preprocess.resize_launch(descs, want, mask=mask, fill=9)
        assert torch.equal(out, want)
        assert bool((out[0, :, rh:, :] == 9).all() and (out[1, :, 30:, :] == 9).all() and (out[1, :, :, 20:] == 9).all())


def test_refusals_launch_nothing():
    """Every refusal of the supported range, by name, through resize_batch on device sources: the entry point is never called."""
    good = _source(rr.make_image("noise", 48, 64))
    calls = [0]
    lib = _lib.lib()
    fn = lib.fvit_image_resize_u8

    def counted(*a):
        calls[0] += 1
        return fn(*a)
    lib.fvit_image_resize_u8 = counted
    try:
        rb = preprocess.resize_batch
        for reason, kw in [("size", dict(sizes=[(0, 32)], windows=[(0, 0, 1, 1)])), ("size", dict(sizes=[(24, 32)], windows=[(0, 0, 0, 32)])),
                           ("window", dict(sizes=[(24, 32)], windows=[(1, 0, 24, 32)])), ("window", dict(sizes=[(24, 32)], windows=[(0, -1, 24, 32)])),
                           ("slot", dict(sizes=[(24, 32)], windows=None, out_size=(24, 31))),
                           ("tap limit", dict(sizes=[(2, 32)], windows=None)), ("tap limit", dict(sizes=[(24, 3)], windows=None)),
                           ("LDS limit", dict(sizes=[(2, 64)], windows=None, filter="bilinear"))]:
            kw = dict(kw)
            flt = kw.pop("filter", "bicubic")
            with pytest.raises(ValueError, match=rf"image 0: refused \({reason}\)"):
                rb([good], kw.pop("sizes"), kw.pop("windows"), filter=flt, **kw)
        with pytest.raises(ValueError, match="unknown filter"):
            rb([good], [(24, 32)], filter="nearest")
        with pytest.raises(ValueError, match="image 1: strides"):
            rb([good, good.permute(1, 0, 2)], [(24, 32)] * 2, filter="bicubic")
        with pytest.raises(ValueError, match="image 0: dtype"):
            rb([good.float()], [(24, 32)], filter="bicubic")
        d = _lib.FvitResizeDesc(src=good.data_ptr(), row_stride=3 * 64 - 1, H=48, W=64, rh=24, rw=32, top=0, left=0, ch=24, cw=32, filter=2)
        assert _lib.FVIT_RESIZE_REASONS[lib.fvit_image_resize_check(ctypes.byref(d), 24, 32)] == "stride"
        d.row_stride, d.filter = 3 * 64, 5
        assert _lib.FVIT_RESIZE_REASONS[lib.fvit_image_resize_check(ctypes.byref(d), 24, 32)] == "filter" and b"filter" in lib.fvit_last_error()
    finally:
        lib.fvit_image_resize_u8 = fn
    assert calls[0] == 0
    # the entry point's own arguments
    out = torch.zeros(1, 3, 24, 32, dtype=torch.uint8, device=DEV)
    descs = _descs([good], [(24, 32)], [(0, 0, 24, 32)], "bicubic", (24, 32))
    view = _lib.FvitMapView(data=out.data_ptr(), stride_b=out.stride(0), stride_c=out.stride(1), stride_h=out.stride(2), stride_w=out.stride(3),
                            dtype=_lib.FVIT_F32)
    assert lib.fvit_image_resize_u8(descs.data_ptr(), 1, ctypes.byref(view), 24, 32, 0, None, None) == -1 and b"FVIT_U8" in lib.fvit_last_error()
    view.dtype = _lib.FVIT_U8
    assert lib.fvit_image_resize_u8(descs.data_ptr(), 1, ctypes.byref(view), 24, 32, 256, None, None) == -1 and b"fill" in lib.fvit_last_error()
    assert lib.fvit_image_resize_u8(None, 1, ctypes.byref(view), 24, 32, 0, None, None) == -1
    torch.cuda.synchronize()
    assert int(out.max()) == 0


def _decoded(seed, n, lo=40, hi=120):
    rng = np.random.default_rng(seed)
    imgs = []
    for i in range(n):
        h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        if i % 2:
            h, w = max(h, w), min(h, w)     # both orientations
        else:
            h, w = min(h, w), max(h, w)
        imgs.append(rr.make_image("smooth" if i % 3 == 0 else "noise", h, w, seed))
    return imgs


def test_classifier_preprocess_feeds_a_uint8_runner():
    """Six decoded images of different sizes and orientations, written where a compiled uint8 runner's graph reads them."""
    model = fastervit_amd.create_model("faster_vit_0_224").eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), SEED, "init"), strict=True)
    model = model.to(DEV).requires_grad_(False)
    model.switch_to_deploy()
    pre = fastervit_amd.ClassifierPreprocess.from_model(model)
    assert (pre.img_size, pre.crop_pct, pre.interpolation) == (224, 0.875, "bicubic")
    imgs = _decoded(11, 6, lo=230, hi=420)
    with torch.no_grad():
        runner = model.compile_inference(torch.zeros(8, 3, 224, 224, dtype=torch.uint8, device=DEV))
        assert runner.static_x.dtype == torch.uint8
        srcs = [torch.from_numpy(im) if i % 2 else _source(im) for i, im in enumerate(imgs)]   # host and device sources in one batch
        batch = pre(srcs, out=runner.static_x[:6])
        assert batch.data_ptr() == runner.static_x.data_ptr()
        torch.cuda.synchronize()
        for i, im in enumerate(imgs):
            (rh, rw), win = pre.geometry(*im.shape[:2])
            ref = rr.reference(im, rh, rw, "bicubic").crop(*win)
            _held(batch[i].permute(1, 2, 0).cpu().numpy(), ref, f"classifier image {i}")
        u8 = batch.clone()
        got = runner(runner.static_x[:6]).clone()
        want = model(u8)
        assert torch.isfinite(want).all() and torch.equal(got, want)


def test_detection_preprocess_feeds_the_backbone():
    case = BACKBONE_CASES["bb_tiny_odd"]
    m = fastervit_amd.build_fastervit(case["name"], **case["kwargs"])
    m.load_state_dict(synth_state_dict(m.state_dict(), SEED, case["family"]), strict=True)
    m = m.eval().to(DEV).requires_grad_(False)
    pre = fastervit_amd.DetectionPreprocess(size=64, max_size=96)
    shapes = [(48, 64), (70, 50), (30, 100), (64, 90)]      # (h, w); the third hits the max_size branch, the fourth is left as it is
    imgs = [rr.make_image("noise", h, w) for h, w in shapes]
    sizes = [pre.output_size(h, w) for h, w in shapes]
    assert sizes == [(64, 85), (89, 64), (29, 96), (64, 90)]
    nested = pre([_source(im) if i % 2 else torch.from_numpy(im) for i, im in enumerate(imgs)])
    Ho, Wo = max(s[0] for s in sizes), max(s[1] for s in sizes)
    assert nested.tensors.shape == (4, 3, Ho, Wo) and nested.tensors.dtype == torch.uint8 and nested.mask.dtype == torch.bool
    want_mask = torch.ones(4, Ho, Wo, dtype=torch.bool)
    for i, (oh, ow) in enumerate(sizes):
        want_mask[i, :oh, :ow] = False
        got = nested.tensors[i].permute(1, 2, 0).cpu().numpy()
        _held(got[:oh, :ow], rr.reference(imgs[i], oh, ow, "bilinear"), f"detection image {i}")
        rest = want_mask[i].numpy()
        assert (got[rest] == 0).all()
    assert torch.equal(nested.mask.cpu(), want_mask)
    assert np.array_equal(nested.tensors[3, :, :64, :90].permute(1, 2, 0).cpu().numpy(), imgs[3])     # the unchanged image: its own bytes
    padded = fastervit_amd.DetectionPreprocess(size=64, max_size=96, pad_to=(96, 128))([torch.from_numpy(im) for im in imgs])
    assert padded.tensors.shape == (4, 3, 96, 128) and torch.equal(padded.tensors[:, :, :Ho, :Wo], nested.tensors)
    assert torch.equal(padded.mask[:, :Ho, :Wo], nested.mask) and bool(padded.mask[:, Ho:].all()) and bool(padded.mask[:, :, Wo:].all())
    with torch.no_grad():
        feats = m(nested)
        plain = m.forward_features(nested.tensors)
    assert sorted(feats) == list(range(len(plain)))
    for k, f in feats.items():
        assert f.tensors.shape == plain[k].shape and torch.isfinite(f.tensors).all()
        assert f.mask.shape == (4,) + tuple(f.tensors.shape[-2:]) and f.mask.dtype == torch.bool
