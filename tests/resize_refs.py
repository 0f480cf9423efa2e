"""float64 restatement of the resize semantics of DESIGN.md section 14 (PIL's Image.resize for 8-bit images) and the per-pixel bound a correct fp32
kernel is held to.  numpy only; shared by tests/test_resize_refs_cpu.py and tests/test_gpu_resize.py.

Along one axis n_in -> n_out: scale = n_in / n_out, fs = max(scale, 1), support = R fs, c = (j + 0.5) scale, k0 = max(0, trunc(c - support + 0.5)),
k1 = min(n_in, trunc(c + support + 0.5)), w_k ~ f((k + 0.5 - c) / fs) normalised to sum 1.  Horizontal pass first, stored as
clamp(floor(sum + 0.5), 0, 255); the vertical pass on that; an axis of unchanged size is skipped.

The bound.  With v the unrounded float64 sum of the LAST pass, clamped to [0, 255]:   |out - v| <= 0.5 + eps,  eps = 255 sum|w_k| (T + 8) 2^-23
(T fp32 multiply-adds on partial sums of at most 255 sum|w|, about eight more roundings in the weight and its normalisation): either side of a tie and
nothing else.  In a two-axis call the last pass reads the reference's own rounded intermediate, and an intermediate whose horizontal value lies within
its eps of a tie may legitimately be one level off: the bound of an output widens by sum_k |w_k| a_k with a_k = 1 for such an intermediate.  A case is
only a fair two-axis case while few outputs are widened (WIDEN_CAP).
"""
import zlib

import numpy as np

RADIUS = {"bilinear": 1.0, "bicubic": 2.0}
WIDEN_CAP = 0.05   # at most this share of a two-axis case's outputs may have a widened bound


def _filter(x, name, a, dtype):
    x = np.abs(x).astype(dtype)
    one, two = dtype(1), dtype(2)
    if name == "bilinear":
        return np.where(x < one, one - x, dtype(0))
    a = dtype(a)
    inner = ((a + two) * x - (a + dtype(3))) * x * x + one
    outer = (((x - dtype(5)) * x + dtype(8)) * x - dtype(4)) * a
    return np.where(x < one, inner, np.where(x < two, outer, dtype(0)))


def coefficients(n_in, n_out, name, *, a=-0.5, antialias=True, half=0.5, dtype=np.float64):
    """[(k0, w)] per output j: taps k0 .. k0 + len(w) - 1 with normalised weights of ``dtype``."""
    scale = n_in / n_out
    fs = max(scale, 1.0) if antialias else 1.0
    support = RADIUS[name] * fs
    out = []
    for j in range(n_out):
        c = (j + half) * scale
        k0 = max(0, int(c - support + 0.5))
        k1 = min(n_in, int(c + support + 0.5))
        if k1 <= k0:   # only a wrong variant (half = 0 at an edge) gets here
            k0 = min(max(k0, 0), n_in - 1)
            k1 = k0 + 1
        ks = np.arange(k0, k1)
        if dtype is np.float64:
            w = _filter((ks + 0.5 - c) / fs, name, a, np.float64)
        else:   # an fp32 evaluation: the argument from exact integers by one division, as an fp32 implementation would form it
            m = max(n_in, n_out) if antialias else n_out
            num = ((2 * ks + 1) * n_out - int(round(2 * (j + half))) * n_in).astype(dtype)
            w = _filter(num / dtype(2 * m), name, a, dtype)
        s = w.sum(dtype=dtype)
        if s != 0:
            w = (w / s).astype(dtype)
        out.append((k0, w))
    return out


def axis_pass(x, axis, n_out, name, *, dtype=np.float64, **kw):
    """Unrounded sums of one pass over ``axis`` (0 rows, 1 columns) of x (H, W, 3), sequential in tap order, in ``dtype``;
    also sum|w| and the tap count per output."""
    n_in = x.shape[axis]
    co = coefficients(n_in, n_out, name, dtype=dtype, **kw)
    shape = list(x.shape)
    shape[axis] = n_out
    v = np.zeros(shape, dtype=dtype)
    x = x.astype(dtype)
    for j, (k0, w) in enumerate(co):
        acc = np.zeros(np.take(x, 0, axis=axis).shape, dtype=dtype)
        for t, wt in enumerate(w):
            acc = (acc + wt * np.take(x, k0 + t, axis=axis)).astype(dtype)
        if axis == 0:
            v[j] = acc
        else:
            v[:, j] = acc
    absw = np.array([np.abs(w.astype(np.float64)).sum() for _, w in co])
    taps = np.array([len(w) for _, w in co])
    return v, absw, taps, co


def round_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def restate(img, rh, rw, name, *, round_between=True, vertical_first=False, dtype=np.float64, **kw):
    """The resized uint8 image; the keyword switches make the wrong variants (and dtype=np.float32 the fp32 evaluation) of the CPU tests."""
    H, W, _ = img.shape
    x = img
    order = [(0, rh, H), (1, rw, W)] if vertical_first else [(1, rw, W), (0, rh, H)]
    for i, (axis, n_out, n_in) in enumerate(order):
        if n_out == n_in:
            continue
        v = axis_pass(x, axis, n_out, name, dtype=dtype, **kw)[0]
        x = round_u8(v) if (round_between or i == 1) else v
    return round_u8(x) if x.dtype != np.uint8 else x


class Ref:
    """out = the restatement's bytes; v = the clamped unrounded sums of the last pass; bound = per-pixel |got - v| limit; widened = share of outputs
    whose bound carries a tie widening (0 for single-axis calls)."""

    def __init__(self, out, v, bound, widened):
        self.out, self.v, self.bound, self.widened = out, v, bound, widened

    def outside(self, got):
        got = np.asarray(got).astype(np.float64)
        return np.abs(got - self.v) > self.bound

    def crop(self, top, left, ch, cw):
        s = (slice(top, top + ch), slice(left, left + cw))
        return Ref(self.out[s], self.v[s], self.bound[s], self.widened)


def _eps(absw, taps):
    return 255.0 * absw * (taps + 8) * 2.0 ** -23


def reference(img, rh, rw, name):
    H, W, _ = img.shape
    img = np.ascontiguousarray(img)
    if rw != W:
        vh, absw, taps, _ = axis_pass(img, 1, rw, name)
        eps_h = _eps(absw, taps)[None, :, None]
        t = round_u8(vh)
        frac = vh - np.floor(vh)
        tie = ((np.abs(frac - 0.5) <= eps_h) & (vh > 0) & (vh < 255)).astype(np.float64)
    else:
        vh, eps_h, t, tie = img.astype(np.float64), None, img, np.zeros(img.shape)
    if rh == H:
        if rw == W:
            return Ref(img, img.astype(np.float64), np.zeros(img.shape), 0.0)
        return Ref(t, np.clip(vh, 0, 255), 0.5 + np.broadcast_to(eps_h, vh.shape), 0.0)
    vv, absw, taps, co = axis_pass(t, 0, rh, name)
    eps_v = _eps(absw, taps)[:, None, None]
    widen = np.zeros(vv.shape)
    for j, (k0, w) in enumerate(co):
        widen[j] = np.tensordot(np.abs(w), tie[k0:k0 + len(w)], axes=(0, 0))
    return Ref(round_u8(vv), np.clip(vv, 0, 255), 0.5 + eps_v + widen, float((widen > 0).mean()))


# ---- images and cases shared by the CPU and GPU tests ----
def make_image(kind, H, W, seed=0):
    rng = np.random.default_rng(zlib.crc32(f"{kind}-{H}-{W}-{seed}".encode()))
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "mult8":
        return (rng.integers(0, 32, (H, W, 3)) * 8).astype(np.uint8)
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        ph = rng.uniform(0, 6.28, 3)
        ch = [127.5 + 120 * np.sin(0.31 * x + 0.17 * y + ph[0]), 127.5 + 120 * np.cos(0.11 * x - 0.23 * y + ph[1]),
              255.0 * ((x + 2 * y) % 37) / 36.0]
        return np.clip(np.stack(ch, -1) + rng.uniform(-0.4, 0.4, (H, W, 3)), 0, 255).astype(np.uint8)
    raise ValueError(kind)


# (H, W, rh, rw) of every value case.  A (size, filter) whose two-axis reference stays under WIDEN_CAP on the noise image runs as ONE two-axis call.
# With bilinear weights the simple ratios (2:1, 8:3, 6:13: 9 - 44 % of the outputs would carry a widened bound on noise) and 20x31 -> 45x70 (5.1 %) do
# not: those run as their two single-axis calls, where the bound has no widening.  Measured shares: tests/test_resize_refs_cpu.py asserts the cap.
SIZES = [(37, 53, 16, 20), (64, 48, 24, 24), (20, 31, 45, 70), (21, 34, 47, 71), (33, 33, 33, 17), (17, 29, 40, 29), (9, 7, 5, 4), (6, 6, 13, 11),
         (1, 1, 4, 4), (3, 130, 3, 9), (96, 64, 48, 32)]
SPLIT_BILINEAR = {(64, 48, 24, 24), (20, 31, 45, 70), (6, 6, 13, 11), (96, 64, 48, 32)}
FILTER_NAMES = ("bilinear", "bicubic")


def value_calls(name):
    """[(H, W, rh, rw)] issued for filter ``name``: two-axis sizes as they are, split sizes as (H, W, rh, W) and (H, W, H, rw)."""
    calls = []
    for s in SIZES:
        H, W, rh, rw = s
        if name == "bilinear" and s in SPLIT_BILINEAR:
            calls += [(H, W, rh, W), (H, W, H, rw)]
        else:
            calls.append(s)
    return calls


def is_two_axis(call):
    H, W, rh, rw = call
    return rh != H and rw != W
