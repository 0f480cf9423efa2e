#!/usr/bin/env python3
"""Time the multi-scale detection backbone (fastervit_amd.build_fastervit) forward_features at detection sizes, batch 2, 'f16' operands,
and the fp32 restatement of tests/backbone_reference.py on the same GPU for comparison.  Prints one JSON line per size.

    python scripts/bench_backbone.py [--model faster_vit_0_224] [--steps 20] [--warmup 5] [--sizes 800x1333,1024x1024]

Synthetic weights (tests/synth.py): the timings do not depend on the values.  Per-level times are CUDA-event intervals of one extra
forward run level by level (stem, then each level including its feature tap).

    python scripts/bench_backbone.py --train [--out profiles/bench_backbone_train.json]

times one fine-tuning step instead (``enable_hat_backward().train()``: train-mode forward + backward + AdamW, batch-statistics BatchNorm,
drop_path_rate of the configuration) at the same sizes, and the two backward kernels of the backbone alone (fvit_token_init_dyn_backward,
fvit_feature_tap_backward) next to PyTorch autograd of the same ops on the same device; the JSON lines are also written to ``--out``."""
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


def event_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def bench_train(a, dev):
    import torch.nn.functional as F
    from fastervit_amd import hat_backward, hat_runtime
    rows = []
    out_indices = (1, 2, 3)
    model = fastervit_amd.build_fastervit(a.model, out_indices=out_indices)
    model.load_state_dict(synth_state_dict(model.state_dict(), 0, "init"))
    model = model.to(dev).enable_hat_backward().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = synth_input(a.batch, H, W, 0).to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            sum(o.square().mean() for o in model.forward_features(x)).backward()
            opt.step()

        t = timed(step, a.steps, a.warmup)
        rows.append({"what": "train_step", "model": a.model, "size": [H, W], "batch": a.batch, "operands": "f16", "ms": round(t * 1e3, 3),
                     "images_per_s": round(a.batch / t, 2)})
        print(json.dumps(rows[-1]), flush=True)
        # the two kernels alone, on the stage-2 map of this size (tokenizer) and the stage-1 output (the largest tap), vs PyTorch autograd of the same ops
        lvl = model.levels[2]
        ws, cw, C2 = lvl.window_size, lvl.global_tokenizer.window_size, model.num_features[2]
        h2, w2 = -(-H // 16), -(-W // 16)
        Hp, Wp = -(-h2 // ws) * ws, -(-w2 // ws) * ws
        xp = torch.randn(a.batch, C2, Hp, Wp, device=dev)
        kh, kw, sh, sw, _, _, Hq, Wq = hat_runtime.token_geometry(Hp, Wp, ws, cw)
        dct = torch.randn(a.batch, Hq * Wq, C2, device=dev)
        tok = lvl.global_tokenizer
        xr = xp.clone().requires_grad_()
        wt, bs = tok.pos_embed.weight, tok.pos_embed.bias

        def tok_torch():
            y = F.avg_pool2d(F.conv2d(xr, wt, bs, padding=1, groups=C2), (kh, kw), (sh, sw))
            y = F.pad(y, (0, Wq - y.shape[3], 0, Hq - y.shape[2])).reshape(a.batch, Hq * Wq, C2)
            return y

        y = tok_torch()
        t_k = event_us(lambda: hat_backward.token_init_dyn_backward(tok, xp, dct, ws), 50, 5)
        t_t = event_us(lambda: torch.autograd.grad(y, [xr, wt, bs], dct, retain_graph=True), 50, 5)
        rows.append({"what": "fvit_token_init_dyn_backward", "map": [a.batch, C2, Hp, Wp], "pool": [kh, kw, sh, sw], "us": round(t_k, 1), "torch_autograd_us": round(t_t, 1)})
        print(json.dumps(rows[-1]), flush=True)
        C1, h1, w1 = model.num_features[1], -(-H // 8), -(-W // 8)
        bn = model.norm1.eval()
        xm = torch.randn(a.batch, C1, h1, w1, device=dev)
        dout = torch.randn(a.batch, C1, h1, w1, device=dev)
        scale, _ = hat_runtime._folded_bn(bn, xm.device)
        xmr = xm.clone().requires_grad_()
        o = F.batch_norm(xmr, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        t_k = event_us(lambda: hat_backward.feature_tap_backward(dout, xm, scale), 50, 5)
        t_t = event_us(lambda: torch.autograd.grad(o, [xmr, bn.weight, bn.bias], dout, retain_graph=True), 50, 5)
        bn.train()
        rows.append({"what": "fvit_feature_tap_backward", "map": [a.batch, C1, h1, w1], "us": round(t_k, 1), "torch_autograd_us": round(t_t, 1)})
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time one fine-tuning step and the two backward kernels instead of the inference forward")
    ap.add_argument("--out", default="", help="with --train: also write the result rows to this JSON file")
    ap.add_argument("--model", default="faster_vit_0_224")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="800x1333,1024x1024")
    ap.add_argument("--ref-steps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    if a.train:
        return bench_train(a, dev)
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
