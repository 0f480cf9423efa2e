#!/usr/bin/env python3
"""Time the multi-scale detection backbone (fastervit_amd.build_fastervit) forward_features at detection sizes, batch 2, 'f16' operands,
and the fp32 restatement of tests/backbone_reference.py on the same GPU for comparison.  Prints one JSON line per size.

    python scripts/bench_backbone.py [--model faster_vit_0_224] [--steps 20] [--warmup 5] [--sizes 800x1333,1024x1024]

Synthetic weights (tests/synth.py): the timings do not depend on the values.  Per-level times are CUDA-event intervals of one extra
forward run level by level (stem, then each level including its feature tap).

    python scripts/bench_backbone.py --train [--out profiles/bench_backbone_train.json]

times one fine-tuning step instead (``enable_hat_backward().train()``: train-mode forward + backward + AdamW, batch-statistics BatchNorm,
drop_path_rate of the configuration) at the same sizes, and the two backward kernels of the backbone alone (fvit_token_init_dyn_backward,
fvit_feature_tap_backward) next to PyTorch autograd of the same ops on the same device; the JSON lines are also written to ``--out``.

    python scripts/bench_backbone.py --deploy [--out profiles/bench_backbone_deploy.json]

times, for each size and in one process, module mode, eager deploy (``switch_to_deploy()``) and the graph runner (``compile_inference``) in
interleaved rounds, the per-level times of eager deploy, and the two glue kernels of the plan alone on the level-0 map of that size
(fvit_map_pad_cl, fvit_layernorm2d_crop_cl next to the dense fvit_layernorm2d_cl on the same pixel count) with their bytes moved and GB/s."""
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


def per_level_deploy(plan, x):
    """Event intervals of one eager-deploy forward run step by step: stem, then each level with its tap and Downsample."""
    from fastervit_amd import hat_runtime
    from fastervit_amd.conv_runtime import LevelMap
    plan._enter(x)
    plan._refresh()
    levels, taps = plan.model.levels, plan.t["taps"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(levels) + 2)]
    with hat_runtime.workspace_slot(plan.slot_base):
        ev[0].record()
        y = plan._stem(x)
        m = LevelMap(y, y.shape[2], y.shape[3])
        ev[1].record()
        for li, (lvl, e) in enumerate(zip(levels, plan.t["levels"])):
            m = plan._conv_level_padded(m, e["blocks"], lvl.window_size) if "blocks" in e else plan._hat_level_dyn(lvl, m, padded_out="down" in e)
            if li in taps:
                plan._tap(m, taps[li])
            if "down" in e:
                m = plan._downsample_crop(m, e["down"])
            ev[li + 2].record()
    torch.cuda.synchronize()
    return {"stem_ms": ev[0].elapsed_time(ev[1]), **{f"level{i}_ms": ev[i + 1].elapsed_time(ev[i + 2]) for i in range(len(levels))}}


def glue_kernels(a, dev, H, W, dtype=torch.float16):
    """fvit_map_pad_cl and fvit_layernorm2d_crop_cl alone on the level-0 map of an H x W image (window 7), and the dense LayerNorm2d kernel on the same
    pixel count.  Bytes are what each pass must move (read + write, 16-bit); the roof is bytes over HBM bandwidth."""
    import ctypes
    from fastervit_amd import _lib
    lib, code = _lib.lib(), _lib.FVIT_F16
    st = torch.cuda.current_stream().cuda_stream
    B, C = a.batch, 64
    h, w = -(-H // 4), -(-W // 4)
    hp, wp = -(-h // 7) * 7, -(-w // 7) * 7
    x = torch.randn(B, h, w, C, device=dev).to(dtype)
    xp = torch.empty(B, hp, wp, C, device=dev, dtype=dtype)
    out = torch.empty_like(x)
    g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    eps = ctypes.c_float(1e-6)
    rows = []
    for what, fn, nbytes in [
            ("fvit_map_pad_cl", lambda: lib.fvit_map_pad_cl(code, x.data_ptr(), xp.data_ptr(), B, h, w, hp, wp, C, st), 2 * B * C * (h * w + hp * wp)),
            ("fvit_layernorm2d_crop_cl", lambda: lib.fvit_layernorm2d_crop_cl(code, xp.data_ptr(), out.data_ptr(), g.data_ptr(), b.data_ptr(), eps, B, h, w,
                                                                             hp, wp, C, C, st), 4 * B * C * h * w),
            ("fvit_layernorm2d_cl", lambda: lib.fvit_layernorm2d_cl(code, x.data_ptr(), out.data_ptr(), g.data_ptr(), b.data_ptr(), eps, B * h * w, C, C, st),
             4 * B * C * h * w)]:
        assert fn() == 0, lib.fvit_last_error()
        us = event_us(fn, 200, 20)
        rows.append({"what": what, "map": [B, h, w, C], "padded": [hp, wp], "us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1),
                     "hbm_roof_us_at_6.3TBps": round(nbytes / 6.3e6, 2)})
    return rows


def bench_deploy(a, dev):
    out_indices = (1, 2, 3)
    rows = []

    def build():
        m = fastervit_amd.build_fastervit(a.model, out_indices=out_indices)
        m.load_state_dict(synth_state_dict(m.state_dict(), 0, "init"))
        return m.eval().to(dev).requires_grad_(False)

    module, deploy = build(), build().switch_to_deploy()
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = synth_input(a.batch, H, W, 0).to(dev)
        with torch.no_grad():
            runner = deploy.compile_inference(x)
            forms = {"module": lambda: module.forward_features(x), "eager_deploy": lambda: deploy.forward_features(x), "runner": lambda: runner(x)}
            ref = forms["module"]()
            err = {k: max(((g - r).abs().max() / r.abs().max()).item() for g, r in zip(forms[k](), ref)) for k in ("eager_deploy", "runner")}
            times = {k: [] for k in forms}
            for _ in range(a.rounds):   # interleaved: every form sees the same machine state
                for k, fn in forms.items():
                    times[k].append(timed(fn, a.steps, a.warmup) * 1e3)
            levels = per_level_deploy(deploy.__dict__["_deploy_plan"], x)
            levels_module = per_level(module, x)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        rows.append({"what": "forward_features", "model": a.model, "size": [H, W], "batch": a.batch, "dtype": "float16", "operands": "f16",
                     "ms": {k: round(v, 3) for k, v in med.items()}, "ms_rounds": {k: [round(t, 3) for t in v] for k, v in times.items()},
                     "speedup_vs_module": {k: round(med["module"] / med[k], 2) for k in ("eager_deploy", "runner")},
                     "per_level_ms_eager_deploy": {k: round(v, 3) for k, v in levels.items()},
                     "per_level_ms_module": {k: round(v, 3) for k, v in levels_module.items()},
                     "max_rel_diff_vs_module": {k: float(f"{v:.3e}") for k, v in err.items()}})
        print(json.dumps(rows[-1]), flush=True)
        for r in glue_kernels(a, dev, H, W):
            r["share_of_level0"] = round(r["us"] * 1e-3 / levels["level0_ms"], 4)
            rows.append(r)
            print(json.dumps(r), flush=True)
        del runner
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "rows": rows}, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deploy", action="store_true", help="time module mode, eager deploy and the graph runner, and the plan's two glue kernels")
    ap.add_argument("--rounds", type=int, default=3, help="with --deploy: interleaved timing rounds per form (the median is reported)")
    ap.add_argument("--train", action="store_true", help="time one fine-tuning step and the two backward kernels instead of the inference forward")
    ap.add_argument("--out", default="", help="with --train / --deploy: also write the result rows to this JSON file")
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
    if a.deploy:
        return bench_deploy(a, dev)
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
