#!/usr/bin/env python3
"""What uint8 input costs and saves.  Three measurements, each in a child process of its own under ``timeout -k 10``; the first
one that fails ends the run.  The rows are printed as JSON lines and written to ``--out`` (default profiles/uint8_input.json).

    python scripts/bench_uint8_input.py [--batch 256] [--rounds 3] [--out profiles/uint8_input.json]

  kernels   every stem kernel alone at batch x 3 x 224 x 224 (fp16 maps): the uint8 entry point against the float entry point on the fp32 image in the
            same layout (planar, channels-last), alternating ``--rounds`` times in one process; device-event time per launch.  Also
            fvit_image_normalize_u8 alone with its bytes per second (1 read + 4 written per element).
  runner    ``runner(x)`` of FasterViT-0 (``compile_inference``, the configuration bench.py times: 2 stream shards joined in front of level 3) with the
            copy-in of a device-resident batch inside the step: a uint8 runner against an fp32 runner, alternating in the same way; images per second.
  precise   the precise plan's logits (two-term streams, "f16x3" operands) from a uint8 batch against the same plan on the fp32 image normalised with
            timm's prefetcher formula, (u - 255 mean) / (255 std): max-abs difference.  The only route where the sub-ulp difference between the two
            fp32 formulas reaches an operand (the ``lo`` term of the image split); the 16-bit plan is measured next to it and must give 0.

Synthetic weights (tests/synth.py) and seeded random bytes: the timings do not depend on the values."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"kernels": 240, "runner": 420, "precise": 240}   # time limit of each child, seconds


def event_us(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def images(batch, hw=224, seed=0):
    """(uint8 batch, the fp32 image it stands for), planar, on the device."""
    import torch
    from fastervit_amd import hat_runtime
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (batch, 3, hw, hw), generator=g, dtype=torch.uint8).cuda()
    sc, sf = hat_runtime.input_norm_constants(hat_runtime.IMAGENET_MEAN, hat_runtime.IMAGENET_STD, 3)
    return u8, hat_runtime.normalize_u8(u8, (ctypes.c_float * 6)(*sc, *sf))


def step_kernels(a):
    import torch
    from fastervit_amd import _lib, hat_runtime
    lib, rows = _lib.lib(), []
    B, H, dt = a.batch, 224, torch.float16
    u8, f32 = images(B)
    sc, sf = hat_runtime.input_norm_constants(hat_runtime.IMAGENET_MEAN, hat_runtime.IMAGENET_STD, 3)
    norm = (ctypes.c_float * 6)(*sc, *sf)
    g = torch.Generator().manual_seed(1)
    w1 = torch.zeros(64, 32)
    w1[:, :27] = torch.randn(64, 27, generator=g) / 27 ** 0.5
    w1h = w1.to(dt).cuda()
    w1l = (w1 - w1h.cpu().float()).to(dt).cuda()
    b1, b2 = torch.randn(64, generator=g).cuda(), torch.randn(64, generator=g).cuda()
    w2 = (torch.randn(64, 3, 3, 64, generator=g) / 24).to(dt).cuda()
    y1 = torch.empty(B, 112, 112, 64, dtype=dt, device="cuda")
    y2 = torch.empty(B, 56, 56, 64, dtype=dt, device="cuda")
    st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    def call(kernel, x):
        v, u = hat_runtime._image_view(x), x.dtype == torch.uint8
        tail = (norm,) if u else ()
        if kernel == "stem_fused":
            fn = lib.fvit_stem_fused_u8 if u else lib.fvit_stem_fused
            return lambda: _lib.check(fn(_lib.FVIT_F16, v, w1h.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y2.data_ptr(), B, H, H, st(), *tail), kernel)
        if kernel == "stem_conv_px":
            fn = lib.fvit_stem_conv3x3s2_px_u8 if u else lib.fvit_stem_conv3x3s2_px
            return lambda: _lib.check(fn(_lib.FVIT_F16, v, w1h.data_ptr(), w1l.data_ptr(), b1.data_ptr(), y1.data_ptr(), B, H, H, st(), *tail), kernel)
        fn = lib.fvit_stem_conv3x3s2_u8 if u else lib.fvit_stem_conv3x3s2
        return lambda: _lib.check(fn(_lib.FVIT_F16, v, w1h.data_ptr(), b1.data_ptr(), y1.data_ptr(), B, H, H, st(), *tail), kernel)

    for layout in ("planar", "channels_last"):
        fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
        xu, xf = u8.contiguous(memory_format=fmt), f32.contiguous(memory_format=fmt)
        for kernel in ("stem_conv", "stem_conv_px", "stem_fused"):
            fu, ff = call(kernel, xu), call(kernel, xf)
            out = y2 if kernel == "stem_fused" else y1
            fu()
            got = out.clone()
            ff()
            same = bool(torch.equal(got, out))
            for f in (fu, ff):
                event_us(f, 10)
            us = {"uint8": [], "fp32": []}
            for _ in range(a.rounds):
                us["uint8"].append(round(event_us(fu, a.launches), 2))
                us["fp32"].append(round(event_us(ff, a.launches), 2))
            rows.append({"what": "stem_kernel", "kernel": kernel, "layout": layout, "batch": B, "same_bits": same, "us_uint8": us["uint8"],
                         "us_fp32": us["fp32"], "uint8_over_fp32": round(min(us["uint8"]) / min(us["fp32"]), 3)})
            print(json.dumps(rows[-1]), flush=True)
        fn = lambda: hat_runtime.normalize_u8(xu, norm, out=xf)   # noqa: E731
        event_us(fn, 10)
        us = [round(event_us(fn, a.launches), 2) for _ in range(a.rounds)]
        rows.append({"what": "image_normalize_u8", "layout": layout, "batch": B, "us": us, "GB_per_s": round(5.0 * u8.numel() / min(us) / 1e3, 1)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def _fvit0():
    import fastervit_amd
    from tests.synth import synth_state_dict
    m = fastervit_amd.create_model("faster_vit_0_224").eval()
    m.load_state_dict(synth_state_dict(m.state_dict(), 0, "init"), strict=True)
    return m.cuda().requires_grad_(False)


def step_runner(a):
    import torch
    rows, model = [], _fvit0()
    u8, f32 = images(a.batch)
    for layout in ("channels_last", "planar"):
        fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
        xu, xf = u8.contiguous(memory_format=fmt), f32.contiguous(memory_format=fmt)
        ru = model.compile_inference(xu, streams=2, join_from=3)
        rf = model.compile_inference(xf, streams=2, join_from=3)
        same = bool(torch.equal(ru(xu).clone(), rf(xf)))
        ips = {"uint8": [], "fp32": []}
        for r, x in ((ru, xu), (rf, xf)):
            event_us(lambda: r(x), 5)
        for _ in range(a.rounds):
            for key, r, x in (("uint8", ru, xu), ("fp32", rf, xf)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    r(x)
                torch.cuda.synchronize()
                ips[key].append(round(a.batch * a.steps / (time.perf_counter() - t0), 1))
        rows.append({"what": "runner", "model": "faster_vit_0_224", "layout": layout, "batch": a.batch, "streams": 2, "join_from": 3, "same_logits": same,
                     "copy_in_MB": {"uint8": round(xu.numel() / 1e6, 1), "fp32": round(xf.numel() * 4 / 1e6, 1)},
                     "images_per_s_uint8": ips["uint8"], "images_per_s_fp32": ips["fp32"],
                     "uint8_over_fp32": round(max(ips["uint8"]) / max(ips["fp32"]), 4)})
        print(json.dumps(rows[-1]), flush=True)
        del ru, rf
    return rows


def step_precise(a):
    import torch
    from fastervit_amd import hat_runtime
    rows = []
    u8, f32 = images(8, seed=3)
    mean = torch.tensor([v * 255 for v in hat_runtime.IMAGENET_MEAN], device="cuda").view(1, 3, 1, 1)
    std = torch.tensor([v * 255 for v in hat_runtime.IMAGENET_STD], device="cuda").view(1, 3, 1, 1)
    timm = (u8.float() - mean) / std                                     # the prefetching loader's normalisation, fp32
    for plan, operands in (("precise", "f16x3"), ("16-bit", "f16")):
        model = _fvit0()
        model.set_hat_operand_dtype(operands)
        model.switch_to_deploy()
        model.__dict__["_deploy_plan"].precise = plan == "precise"
        with torch.no_grad():
            yu, yt, yf = model(u8).clone(), model(timm).clone(), model(f32).clone()
        rows.append({"what": "logits_uint8_vs_timm_normalised_fp32", "plan": plan, "operands": operands, "batch": 8,
                     "image_max_abs_diff": float((f32 - timm).abs().max()), "logits_max_abs": float(yf.abs().max()),
                     "logits_max_abs_diff_vs_timm": float((yu - yt).abs().max()), "logits_equal_to_table_image": bool(torch.equal(yu, yf))})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="kernel launches per timed window")
    ap.add_argument("--steps", type=int, default=30, help="runner calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uint8_input.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one measurement in this process and print its rows")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "bench_uint8_input needs a GPU"
        rows = {"kernels": step_kernels, "runner": step_runner, "precise": step_precise}[a.step](a)
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows = []
    for step in ("kernels", "runner", "precise"):
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--batch", str(a.batch),
               "--rounds", str(a.rounds), "--launches", str(a.launches), "--steps", str(a.steps)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for line in res.stdout.splitlines():
            if line.startswith("ROWS "):
                rows += json.loads(line[5:])
            else:
                print(line, flush=True)
        if res.returncode != 0:   # a fault, an abort or a time limit: nothing more is started on the device
            print(f"step {step} ended with status {res.returncode}; stopping", flush=True)
            with open(a.out, "w") as f:
                json.dump({"incomplete_after": step, "rows": rows}, f, indent=1)
            return res.returncode
    with open(a.out, "w") as f:
        json.dump({"rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
