#!/usr/bin/env python3
"""Time the multi-scale detection backbone (fastervit_amd.build_fastervit) forward_features at detection sizes, batch 2, 'f16' operands,
and the fp32 restatement of tests/backbone_reference.py on the same GPU for comparison.  Prints one JSON line per size.

    python scripts/bench_backbone.py [--model faster_vit_0_224] [--steps 20] [--warmup 5] [--sizes 800x1333,1024x1024]

Synthetic weights (tests/synth.py): the timings do not depend on the values.  Per-level times are CUDA-event intervals of one extra
forward run level by level (stem, then each level including its feature tap)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fastervit_amd  # noqa: E402
from fastervit_amd.hat_runtime import feature_tap  # noqa: E402
from fastervit_amd.models.backbone import _BACKBONE_CFGS  # noqa: E402
from tests import backbone_reference as br  # noqa: E402
from tests.synth import synth_input, synth_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def per_level(model, x):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(model.levels) + 2)]
    ev[0].record()
    h = model.patch_embed(x)
    ev[1].record()
    for i, lvl in enumerate(model.levels):
        h, xo = lvl(h)
        if i in model.out_indices:
            feature_tap(xo, getattr(model, f"norm{i}"))
        ev[i + 2].record()
    torch.cuda.synchronize()
    return {"stem_ms": ev[0].elapsed_time(ev[1]), **{f"level{i}_ms": ev[i + 1].elapsed_time(ev[i + 2]) for i in range(len(model.levels))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="faster_vit_0_224")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="800x1333,1024x1024")
    ap.add_argument("--ref-steps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    out_indices = (1, 2, 3)
    model = fastervit_amd.build_fastervit(a.model, out_indices=out_indices)
    sd = synth_state_dict(model.state_dict(), 0, "init")
    model.load_state_dict(sd)
    model = model.eval().to(dev).requires_grad_(False)
    model.set_hat_operand_dtype("f16")
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    cfg = dict(_BACKBONE_CFGS[a.model], out_indices=out_indices)
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = synth_input(a.batch, H, W, 0).to(dev)
        with torch.no_grad():
            t = timed(lambda: model.forward_features(x), a.steps, a.warmup)
            levels = per_level(model, x)
            t_ref = timed(lambda: br.backbone_forward(sd_dev, x, cfg, out_indices, dtype=torch.float32), a.ref_steps, 1)
            got = model.forward_features(x)
            ref = br.backbone_forward(sd_dev, x, cfg, out_indices, dtype=torch.float32)
        err = max(((g - r).abs().max() / r.abs().max()).item() for g, r in zip(got, ref))
        print(json.dumps({"model": a.model, "size": [H, W], "batch": a.batch, "operands": "f16", "ms": round(t * 1e3, 3),
                          "images_per_s": round(a.batch / t, 2), "per_level_ms": {k: round(v, 3) for k, v in levels.items()},
                          "ref_fp32_ms": round(t_ref * 1e3, 3), "speedup_vs_ref_fp32": round(t_ref / t, 2),
                          "max_rel_err_vs_ref_fp32": float(f"{err:.3e}")}), flush=True)


if __name__ == "__main__":
    main()
