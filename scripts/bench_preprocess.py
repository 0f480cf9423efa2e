#!/usr/bin/env python3
"""Time the resize + crop + pad kernel (fastervit_amd.preprocess, csrc/fvit_resize.hip) against the per-image torch form on the same device.

    python scripts/bench_preprocess.py [--reps 7] [--iters 3] [--out profiles/bench_preprocess.json]

(a) classifier: 256 seeded images around 500 x 375 in both orientations, device resident, to 224 x 224 bicubic (Resize(256) + CenterCrop(224)).
    Forms: ``launch`` = fvit_image_resize_u8 on descriptors already on the device (the kernel); ``batch`` = resize_batch as a caller uses it
    (descriptor checks, one descriptor upload, the launch); ``torch`` = per image float(), F.interpolate(antialias=True), round, clamp, uint8, crop,
    then one stack.  The torch form computes a DIFFERENT bicubic (a = -0.75, fp32 between the passes): it is the only device path there was, not
    a reference for the values.
(b) detection: two 480 x 640 images to 800 x 1066 bilinear, padded to the batch, with the mask, against the same torch form plus F.pad.
(c) end to end: images / s of preprocess -> uint8 runner at batch 256 with the sources resident and with the sources in pinned host memory, against
    the runner alone on resident bytes in the same process.

All forms of a section alternate in one process, window by window, each window bracketed by device events after a warm-up of the same calls; the figure
recorded is the median over ``reps`` windows with min and max beside it.  The kernel's bytes are computed from the shapes: the source rows and columns
the windows' taps need, once, plus the destination once.  Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fastervit_amd  # noqa: E402
from fastervit_amd import _lib, preprocess  # noqa: E402

HBM_TBS = 6.29   # measured float4-copy rate of the part (8.0 TB/s datasheet)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def interleave(forms, reps, iters):
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(window(fn, iters))
    return times


def summary(times):
    return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in times.items()}


def tap_range(n_in, n_out, R, j0, j1):
    """source indices [lo, hi) the outputs j0 .. j1 - 1 of one axis read (the kernel's integer arithmetic)"""
    if n_in == n_out:
        return j0, j1
    m = max(n_in, n_out)
    lo = max(0, ((2 * j0 + 1) * n_in - 2 * R * m + n_out)) // (2 * n_out)
    hi = min(n_in, ((2 * (j1 - 1) + 1) * n_in + 2 * R * m + n_out) // (2 * n_out))
    return lo, hi


def needed_bytes(shapes, sizes, windows, R, Ho, Wo, mask):
    src = 0
    for (H, W), (rh, rw), (top, left, ch, cw) in zip(shapes, sizes, windows):
        r0, r1 = tap_range(H, rh, R, top, top + ch)
        c0, c1 = tap_range(W, rw, R, left, left + cw)
        src += (r1 - r0) * (c1 - c0) * 3
    return src, len(shapes) * Ho * Wo * (4 if mask else 3)


def torch_resize(img, rh, rw, mode):
    x = img.permute(2, 0, 1)[None].float()
    y = F.interpolate(x, size=(rh, rw), mode=mode, antialias=True, align_corners=False)
    return y.round_().clamp_(0, 255).to(torch.uint8)[0]


def descriptors(srcs, sizes, windows, code, out_size, dev):
    arr = (_lib.FvitResizeDesc * len(srcs))()
    for i, s in enumerate(srcs):
        arr[i] = preprocess.make_descriptor(s.data_ptr(), s.shape[0], s.shape[1], s.stride(0), sizes[i], windows[i], code, out_size)
    return torch.frombuffer(arr, dtype=torch.uint8).clone().to(dev)


def classifier_images(n, seed):
    rng = np.random.default_rng(seed)
    imgs = []
    for i in range(n):
        long, short = int(rng.integers(440, 561)), int(rng.integers(330, 421))
        h, w = (short, long) if i % 2 == 0 else (long, short)
        imgs.append(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
    return imgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-runner", action="store_true", help="sections (a) and (b) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_preprocess.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, iters=args.iters,
                  timing="device events around iters calls, median (min, max) over reps windows, the forms of a section interleaved per rep",
                  yardstick="per-image torch form on the same device: float, F.interpolate(antialias=True), round, clamp, uint8, crop, stack (+ F.pad). "
                            "It computes a different bicubic (a = -0.75, fp32 between the passes) than PIL and the kernel (a = -0.5, uint8 between)",
                  hbm_roof_TBps=HBM_TBS)

    # ---- (a) classifier ----
    pre = fastervit_amd.ClassifierPreprocess(224, 0.875, "bicubic")
    host = classifier_images(B, 2024)
    srcs = [im.to(dev) for im in host]
    geo = [pre.geometry(im.shape[0], im.shape[1]) for im in host]
    sizes, windows = [g[0] for g in geo], [g[1] for g in geo]
    out = torch.empty(B, 3, 224, 224, dtype=torch.uint8, device=dev)
    descs = descriptors(srcs, sizes, windows, preprocess.FILTERS["bicubic"], (224, 224), dev)

    def a_launch():
        preprocess.resize_launch(descs, out)

    def a_batch():
        pre(srcs, out=out)

    def a_torch():
        return torch.stack([torch_resize(s, rh, rw, "bicubic")[:, t:t + 224, l:l + 224] for s, (rh, rw), (t, l, _, _) in zip(srcs, sizes, windows)])

    a_launch()
    diff = (out.int() - a_torch().int()).abs()
    times = interleave(dict(launch=a_launch, batch=a_batch, torch=a_torch), args.reps, args.iters)
    src_b, dst_b = needed_bytes([tuple(s.shape[:2]) for s in srcs], sizes, windows, 2, 224, 224, False)
    med = statistics.median(times["launch"])
    result["classifier"] = dict(
        images=B, source="330-420 x 440-560 both orientations, device resident", to="224 x 224 bicubic (Resize 256 + CenterCrop 224)", us=summary(times),
        faster_than_torch_in_every_round=all(k < t for k, t in zip(times["launch"], times["torch"])) and all(k < t for k, t in zip(times["batch"], times["torch"])),
        speedup_launch=round(statistics.median(times["torch"]) / med, 1), speedup_batch=round(statistics.median(times["torch"]) / statistics.median(times["batch"]), 1),
        images_per_s_launch=round(B / med * 1e6), needed_source_bytes=src_b, needed_destination_bytes=dst_b,
        achieved_TBps=round((src_b + dst_b) / med * 1e-6, 3), share_of_hbm_roof=round((src_b + dst_b) / med * 1e-6 / HBM_TBS, 3),
        levels_from_torch_form=dict(max=int(diff.max()), mean=round(float(diff.float().mean()), 3)))
    print(json.dumps(result["classifier"]), flush=True)

    # ---- (b) detection ----
    rng = np.random.default_rng(7)
    dhost = [torch.from_numpy(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)) for _ in range(2)]
    dsrc = [im.to(dev) for im in dhost]
    det = fastervit_amd.DetectionPreprocess(800, 1333, "bilinear")
    dsz = [det.output_size(480, 640)] * 2
    dwin = [(0, 0, *dsz[0])] * 2
    Ho, Wo = 800, 1088           # a bucket wider than the images: 22 padded columns
    dout = torch.empty(2, 3, Ho, Wo, dtype=torch.uint8, device=dev)
    dmask = torch.empty(2, Ho, Wo, dtype=torch.bool, device=dev)
    ddesc = descriptors(dsrc, dsz, dwin, preprocess.FILTERS["bilinear"], (Ho, Wo), dev)
    detp = fastervit_amd.DetectionPreprocess(800, 1333, "bilinear", pad_to=(Ho, Wo))

    def b_launch():
        preprocess.resize_launch(ddesc, dout, mask=dmask)

    def b_batch():
        return detp(dsrc)

    def b_torch():
        ims = [F.pad(torch_resize(s, *sz, "bilinear"), (0, Wo - sz[1], 0, Ho - sz[0])) for s, sz in zip(dsrc, dsz)]
        m = torch.ones(2, Ho, Wo, dtype=torch.bool, device=dev)
        for i, sz in enumerate(dsz):
            m[i, :sz[0], :sz[1]] = False
        return torch.stack(ims), m

    times = interleave(dict(launch=b_launch, batch=b_batch, torch=b_torch), args.reps, max(args.iters, 10))
    src_b, dst_b = needed_bytes([(480, 640)] * 2, dsz, dwin, 1, Ho, Wo, True)
    med = statistics.median(times["launch"])
    result["detection"] = dict(images=2, source="480 x 640", to=f"{dsz[0][0]} x {dsz[0][1]} bilinear in a {Ho} x {Wo} slot with mask", us=summary(times),
                               speedup_launch=round(statistics.median(times["torch"]) / med, 1), needed_source_bytes=src_b, needed_destination_bytes=dst_b,
                               achieved_TBps=round((src_b + dst_b) / med * 1e-6, 3), share_of_hbm_roof=round((src_b + dst_b) / med * 1e-6 / HBM_TBS, 3))
    print(json.dumps(result["detection"]), flush=True)

    # ---- (c) end to end ----
    if not args.skip_runner:
        model = fastervit_amd.create_model("faster_vit_0_224").eval().to(dev).requires_grad_(False)
        model.switch_to_deploy()
        with torch.no_grad():
            runner = model.compile_inference(torch.zeros(B, 3, 224, 224, dtype=torch.uint8, device=dev))
            resident = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, device=dev)
            pinned = [im.pin_memory() for im in host]

            def c_runner():
                return runner(resident)

            def c_resident():
                pre(srcs, out=runner.static_x)
                return runner(runner.static_x)

            def c_pinned():
                pre(pinned, out=runner.static_x)
                return runner(runner.static_x)

            times = interleave(dict(runner_alone=c_runner, resident_sources=c_resident, pinned_host_sources=c_pinned), args.reps, args.iters)
        result["end_to_end"] = dict(batch=B, model="faster_vit_0_224 uint8 runner (compile_inference defaults)", us=summary(times),
                                    images_per_s={k: round(B / statistics.median(v) * 1e6) for k, v in times.items()},
                                    host_bytes_per_batch=sum(im.numel() for im in host))
        print(json.dumps(result["end_to_end"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
