"""Resize, crop, pad and batch decoded uint8 images on the GPU, in front of the uint8 stem.

A decoder produces ``(H, W, 3)`` uint8 images of different sizes.  ``resize_batch`` turns a list of them into one ``(B, 3, Ho, Wo)`` uint8 batch with ONE
launch of ``fvit_image_resize_u8`` (``csrc/fvit_resize.hip``): PIL's ``Image.resize`` semantics for 8-bit images (antialiased, bicubic with a = -0.5,
the horizontal pass rounded to uint8 before the vertical one), a window of the resized image written at the top-left corner of the slot, ``fill``
elsewhere and DINO's padding mask.  ``ClassifierPreprocess`` (``Resize + CenterCrop`` of a model's ``default_cfg``) and ``DetectionPreprocess``
(DINO's ``RandomResize([size], max_size)`` + ``nested_tensor_from_tensor_list``) are the two size rules on top of it.

There is no CPU path: without a HIP device every entry point here raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import torch

from . import _lib

FILTERS = {"bilinear": _lib.FVIT_RESIZE_BILINEAR, "bicubic": _lib.FVIT_RESIZE_BICUBIC}
_DESC_BYTES = C.sizeof(_lib.FvitResizeDesc)


class NestedTensor:
    """``tensors`` (B, 3, H, W) + ``mask`` (B, H, W) bool, True on padding -- the type ``FasterViTBackbone.forward`` and the backbone runners take."""

    def __init__(self, tensors: torch.Tensor, mask: torch.Tensor):
        self.tensors, self.mask = tensors, mask

    def to(self, device):
        return NestedTensor(self.tensors.to(device), None if self.mask is None else self.mask.to(device))

    def decompose(self):
        return self.tensors, self.mask

    def __repr__(self):
        return f"NestedTensor(tensors={tuple(self.tensors.shape)}, mask={None if self.mask is None else tuple(self.mask.shape)})"


def _filter_code(name) -> int:
    if name not in FILTERS:
        raise ValueError(f"unknown filter {name!r}: the resize kernel has {sorted(FILTERS)}")
    return FILTERS[name]


def classifier_geometry(h: int, w: int, img_size: int = 224, crop_pct: float = 0.875):
    """``Resize(floor(img_size / crop_pct)) + CenterCrop(img_size)`` of an (h, w) image: ``((rh, rw), (top, left, img_size, img_size))``."""
    scale = int(math.floor(img_size / crop_pct))
    if w <= h:
        rw, rh = scale, int(scale * h / w)
    else:
        rh, rw = scale, int(scale * w / h)
    top, left = int(round((rh - img_size) / 2.0)), int(round((rw - img_size) / 2.0))
    return (rh, rw), (top, left, img_size, img_size)


def detection_size(h: int, w: int, size: int = 800, max_size: int | None = 1333):
    """DINO's aspect-ratio rule: the short side becomes ``size`` unless the long side would pass ``max_size``; returns ``(oh, ow)``."""
    lo, hi = float(min(h, w)), float(max(h, w))
    if max_size is not None and hi / lo * size > max_size:
        size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def _check_image(i: int, img, device_only: bool = False):
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"image {i}: expected a torch.Tensor of shape (H, W, 3) and dtype uint8, got {type(img).__name__}")
    if img.dtype != torch.uint8:
        raise ValueError(f"image {i}: dtype {img.dtype} is not uint8 (the resize kernel takes what a decoder produces; the stem normalises)")
    if img.dim() != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image {i}: shape {tuple(img.shape)} is not (H, W, 3) -- HWC with three channels")
    if img.is_cuda and (img.stride(2) != 1 or img.stride(1) != 3 or (img.shape[0] > 1 and img.stride(0) < 3 * img.shape[1])):
        raise ValueError(f"image {i}: strides {tuple(img.stride())} are not HWC pixels (stride 1 over channels, 3 over columns, >= 3 W over rows)")


def _hw(i: int, img):
    """(H, W) of image i for the size rules; resize_batch makes the full check."""
    if not isinstance(img, torch.Tensor) or img.dim() != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        _check_image(i, img)
    return int(img.shape[0]), int(img.shape[1])


def make_descriptor(src_ptr: int, H: int, W: int, row_stride: int, size, window, filter_code: int, out_size, what: str = "image"):
    """One ``FvitResizeDesc``, checked by the library's own query (``fvit_image_resize_check``: no device call); raises ``ValueError`` with its reason."""
    (rh, rw), (top, left, ch, cw) = size, window
    geo = (int(row_stride), int(H), int(W), int(rh), int(rw), int(top), int(left), int(ch), int(cw), int(filter_code))
    rc, msg = _query(geo, int(out_size[0]), int(out_size[1]))
    if rc != 0:
        raise ValueError(f"{what}: refused ({_lib.FVIT_RESIZE_REASONS.get(rc, rc)}): {msg}")
    return _lib.FvitResizeDesc(src_ptr, *geo)


@functools.lru_cache(maxsize=8192)
def _query(geo, Ho, Wo):
    """(code, message) of fvit_image_resize_check for one geometry; a loader meets the same few image sizes again and again."""
    lib = _lib.lib()
    d = _lib.FvitResizeDesc(0, *geo)
    rc = lib.fvit_image_resize_check(C.byref(d), Ho, Wo)
    return rc, (lib.fvit_last_error().decode("utf-8", "replace") if rc != 0 else "")


def resize_launch(descs: torch.Tensor, out: torch.Tensor, *, mask: torch.Tensor | None = None, fill: int = 0) -> None:
    """The launch alone: ``descs`` = the bytes of ``out.shape[0]`` descriptors in device memory (uint8, 8-byte aligned).  No allocation, no copy, no
    synchronisation: capturable; a replay reads the descriptors and the source bytes of that moment."""
    if not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 4 or out.shape[1] != 3:
        raise RuntimeError(f"resize: out must be a (B, 3, Ho, Wo) uint8 tensor on a HIP device (got {tuple(out.shape)} {out.dtype} on {out.device}); "
                           "there is no CPU fallback")
    B, _, Ho, Wo = out.shape
    if descs.device != out.device or descs.dtype != torch.uint8 or descs.numel() < B * _DESC_BYTES or descs.data_ptr() % 8 or not descs.is_contiguous():
        raise RuntimeError(f"resize: descs must hold {B} descriptors ({B * _DESC_BYTES} contiguous uint8 bytes, 8-byte aligned) on {out.device}")
    if mask is not None and (mask.device != out.device or mask.dtype != torch.bool or tuple(mask.shape) != (B, Ho, Wo) or not mask.is_contiguous()):
        raise RuntimeError(f"resize: mask must be a contiguous ({B}, {Ho}, {Wo}) bool tensor on {out.device}")
    view = _lib.FvitMapView(data=out.data_ptr(), stride_b=out.stride(0), stride_c=out.stride(1), stride_h=out.stride(2), stride_w=out.stride(3),
                            dtype=_lib.FVIT_U8)
    with torch.cuda.device(out.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().fvit_image_resize_u8(descs.data_ptr(), B, C.byref(view), Ho, Wo, int(fill), None if mask is None else mask.data_ptr(),
                                                   stream), "fvit_image_resize_u8")


def resize_batch(images, sizes, windows=None, *, filter, out=None, out_size=None, mask=False, fill=0, channels_last=True):
    """Resize image i to ``sizes[i] = (rh, rw)`` and write ``windows[i] = (top, left, ch, cw)`` of it (default: all of it) into slot i of a
    ``(B, 3, Ho, Wo)`` uint8 batch, ``fill`` elsewhere.  One kernel launch.

    images    list of ``(H, W, 3)`` uint8 tensors.  CPU tensors are packed into one pinned staging buffer and uploaded with one copy (the descriptors
              ride in the same buffer); device tensors are read in place (HWC pixels, any row stride).
    out       the caller's ``(B, 3, Ho, Wo)`` uint8 tensor, planar, channels-last or a slice of either (``runner.static_x[:B]``); allocated when None
              (``out_size`` or the largest window; ``channels_last`` chooses its layout).
    mask      True: also return the ``(B, Ho, Wo)`` bool padding mask (False on the window); or a tensor of that shape to write into.
    Returns ``out``, or ``(out, mask)``.
    """
    code = _filter_code(filter)
    images = list(images)
    B = len(images)
    if B == 0:
        raise ValueError("resize_batch: no images")
    for i, img in enumerate(images):
        _check_image(i, img)
    sizes = [tuple(int(v) for v in s) for s in sizes]
    if windows is None:
        windows = [(0, 0, s[0], s[1]) for s in sizes]
    windows = [tuple(int(v) for v in w) for w in windows]
    if len(sizes) != B or len(windows) != B or any(len(s) != 2 for s in sizes) or any(len(w) != 4 for w in windows):
        raise ValueError(f"resize_batch: {B} images need {B} sizes (rh, rw) and {B} windows (top, left, ch, cw)")
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"resize_batch: fill={fill} is not a uint8 value")
    if out is not None:
        if out.dim() != 4 or out.shape[0] != B or out.shape[1] != 3 or out.dtype != torch.uint8:
            raise ValueError(f"resize_batch: out must be ({B}, 3, Ho, Wo) uint8, got {tuple(out.shape)} {out.dtype}")
        Ho, Wo = int(out.shape[2]), int(out.shape[3])
        if out_size is not None and tuple(out_size) != (Ho, Wo):
            raise ValueError(f"resize_batch: out_size {tuple(out_size)} contradicts out {tuple(out.shape)}")
    elif out_size is not None:
        Ho, Wo = int(out_size[0]), int(out_size[1])
    else:
        Ho, Wo = max(1, max(w[2] for w in windows)), max(1, max(w[3] for w in windows))   # (an empty window is refused by name below)
    # every descriptor is checked (on the host, by the library) before anything is allocated or uploaded; pointers are filled in below
    descs = (_lib.FvitResizeDesc * B)()
    for i, img in enumerate(images):
        H, W = int(img.shape[0]), int(img.shape[1])
        stride = int(img.stride(0)) if img.is_cuda and H > 1 else 3 * W
        descs[i] = make_descriptor(0, H, W, stride, sizes[i], windows[i], code, (Ho, Wo), what=f"image {i}")

    if out is not None:
        device = out.device
    else:
        device = next((img.device for img in images if img.is_cuda), None)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("resize_batch runs only on a HIP device (libfvit_hip.so kernels); there is no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise RuntimeError(f"resize_batch runs only on a HIP device (libfvit_hip.so kernels); out is on {device} and there is no CPU fallback")
    for i, img in enumerate(images):
        if img.is_cuda and img.device != device:
            raise RuntimeError(f"image {i} is on {img.device}, the batch on {device} (no implicit copy between devices)")

    # staging: [B descriptors][CPU image 0][CPU image 1] ... at 16-byte offsets, one pinned buffer, one copy
    offsets, total = {}, (B * _DESC_BYTES + 15) // 16 * 16
    for i, img in enumerate(images):
        if not img.is_cuda:
            offsets[i] = total
            total += (img.shape[0] * img.shape[1] * 3 + 15) // 16 * 16
    with torch.cuda.device(device):
        dev_buf = torch.empty(total, dtype=torch.uint8, device=device)
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        for i, img in enumerate(images):
            if img.is_cuda:
                descs[i].src = img.data_ptr()
            else:
                H, W = int(img.shape[0]), int(img.shape[1])
                stage[offsets[i]:offsets[i] + H * W * 3].view(H, W, 3).copy_(img)
                descs[i].src = dev_buf.data_ptr() + offsets[i]
        stage[:B * _DESC_BYTES].copy_(torch.frombuffer(descs, dtype=torch.uint8))
        dev_buf.copy_(stage, non_blocking=True)
        if out is None:
            out = torch.empty((B, 3, Ho, Wo), dtype=torch.uint8, device=device,
                              memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        mask_t = None
        if isinstance(mask, torch.Tensor):
            mask_t = mask
        elif mask:
            mask_t = torch.empty((B, Ho, Wo), dtype=torch.bool, device=device)
        resize_launch(dev_buf, out, mask=mask_t, fill=fill)
    return out if mask_t is None else (out, mask_t)


class ClassifierPreprocess:
    """``Resize(floor(img_size / crop_pct), interpolation) + CenterCrop(img_size)`` -- the validation transform a classifier's ``default_cfg`` prescribes --
    for a list of decoded images, written as one uint8 batch (``out=runner.static_x[:n]`` puts it where a compiled runner's graph reads it)."""

    def __init__(self, img_size: int = 224, crop_pct: float = 0.875, interpolation: str = "bicubic"):
        if not 0.0 < crop_pct <= 1.0:
            raise ValueError(f"ClassifierPreprocess: crop_pct={crop_pct} must lie in (0, 1]")
        _filter_code(interpolation)
        self.img_size, self.crop_pct, self.interpolation = int(img_size), float(crop_pct), interpolation

    @classmethod
    def from_model(cls, model):
        cfg = getattr(model, "default_cfg", None) or getattr(model, "pretrained_cfg", None)
        if not cfg:
            raise ValueError("ClassifierPreprocess.from_model: the model has neither default_cfg nor pretrained_cfg")
        return cls(img_size=int(cfg["input_size"][-1]), crop_pct=float(cfg.get("crop_pct", 0.875)), interpolation=cfg.get("interpolation", "bicubic"))

    def geometry(self, h: int, w: int):
        return classifier_geometry(h, w, self.img_size, self.crop_pct)

    def __call__(self, images, out=None, channels_last=True):
        images = list(images)
        geo = [self.geometry(*_hw(i, img)) for i, img in enumerate(images)]
        return resize_batch(images, [g[0] for g in geo], [g[1] for g in geo], filter=self.interpolation, out=out,
                            out_size=(self.img_size, self.img_size), channels_last=channels_last)


class DetectionPreprocess:
    """DINO's ``RandomResize([size], max_size=max_size)`` + ``nested_tensor_from_tensor_list``: every image resized by the aspect-ratio rule, written at
    the top-left corner of its slot, the batch padded with zeros to its largest image (or to ``pad_to = (H, W)``, a runner's bucket) with the padding
    mask.  Returns a ``NestedTensor`` of uint8 images, which ``FasterViTBackbone.forward`` and the backbone runners normalise with the mask."""

    def __init__(self, size: int = 800, max_size: int | None = 1333, interpolation: str = "bilinear", pad_to=None):
        _filter_code(interpolation)
        self.size, self.max_size, self.interpolation = int(size), max_size, interpolation
        self.pad_to = None if pad_to is None else (int(pad_to[0]), int(pad_to[1]))

    def output_size(self, h: int, w: int):
        return detection_size(h, w, self.size, self.max_size)

    def __call__(self, images, channels_last=False) -> NestedTensor:
        images = list(images)
        sizes = [self.output_size(*_hw(i, img)) for i, img in enumerate(images)]
        out_size = self.pad_to or (max(s[0] for s in sizes), max(s[1] for s in sizes))
        tensors, mask = resize_batch(images, sizes, None, filter=self.interpolation, out_size=out_size, mask=True, fill=0, channels_last=channels_last)
        return NestedTensor(tensors, mask)
