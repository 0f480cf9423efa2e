"""Times the attention-core backward for long sequences (fvit_bwd_window_attention_long, csrc/fvit_attnbwd.hip) with HIP events:

  (a) the new kernel sequence at (nwin, S, heads, D) = (64, 576, 16, 64), (32, 1024, 16, 64), (256, 240, 8, 32) with the compact bias table and its
      gradient, and at (1024, 53, 8, 32) with the dense table next to the scalar fp32 attn_bwd_kernel (fvit_bwd_window_attention + colsum_finish);
  (b) the outside yardstick: the same core written with PyTorch fp16 tensor ops (matmul, softmax) and differentiated by autograd on the same device
      (the forward is outside the timed region; no bias gradient, which favours (b));
  (c) with --model: one fine-tuning step (forward, backward, AdamW) of the full faster_vit_4_21k_384 in images / s.

TFLOP/s are on the ALGORITHMIC count, 5 products x 2 S^2 D per (window, head) with D the padded head_dim; the tiles the phases recompute (the kernel
evaluates 11 tile products for those 5, fvit_attnbwd.hip) are NOT counted.  Writes one JSON document (--out, default profiles/bench_backward_long.json)."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastervit_amd import _lib  # noqa: E402

CASES = [(64, 576, 16, 64, 24, 0), (32, 1024, 16, 64, 32, 0), (256, 240, 8, 32, 15, 15), (1024, 53, 8, 32, 0, 0)]   # nwin, S, heads, D, rel_w, rel_ng


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_case(nwin, S, heads, D, w, ng, reps):
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(S)
    dt, code = torch.float16, 1
    qkv = torch.randn(nwin * S, 3 * heads * D, generator=g).to(dt).cuda()
    dO = torch.randn(nwin * S, heads * D, generator=g).to(dt).cuda()
    dqkv = torch.empty_like(qkv)
    scale = ctypes.c_float(D ** -0.5)
    rel = bias = None
    spad = 0
    if w:
        rel = torch.randn(heads, (2 * w - 1) ** 2, generator=g).cuda()
        dbias = torch.zeros_like(rel)
    else:
        spad = lib.fvit_attention_spad(S)
        bias = torch.randn(heads, spad, spad, generator=g).cuda()
        dbias = torch.zeros(heads, S, S, device="cuda")
    nbytes = lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, D, w)
    ws = torch.empty(nbytes // 4, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def new():
        _lib.check(lib.fvit_bwd_window_attention_long(code, qkv.data_ptr(), qkv.shape[1], dO.data_ptr(), dO.shape[1], p(bias), spad, p(rel), w, ng, scale,
                                                      dqkv.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, nwin, S, heads, D, st), "long backward")

    flops = 5 * 2.0 * S * S * D * nwin * heads
    row = dict(nwin=nwin, S=S, heads=heads, D=D, bias="compact" if w else "dense", workspace_mb=round(nbytes / 2 ** 20, 2))
    row["new_ms"] = timed(new, reps)
    row["new_tflops"] = flops / row["new_ms"] / 1e9
    if S <= 64:
        part = torch.empty(nwin, heads, S, S, device="cuda")

        def old():
            _lib.check(lib.fvit_bwd_window_attention(code, qkv.data_ptr(), qkv.shape[1], dO.data_ptr(), dO.shape[1], bias.data_ptr(), spad, scale, dqkv.data_ptr(),
                                                     part.data_ptr(), nwin, S, heads, D, st), "short backward")
            _lib.check(lib.fvit_bwd_colsum_finish(part.data_ptr(), nwin, heads * S * S, dbias.data_ptr(), heads * S * S, 1, st), "dbias")

        row["scalar_fp32_kernel_ms"] = timed(old, reps)
    # (b) PyTorch fp16 tensor ops + autograd on the same device
    q, k, v = (qkv.view(nwin, S, 3, heads, D)[:, :, i].permute(0, 2, 1, 3).contiguous().requires_grad_(True) for i in range(3))
    do = dO.view(nwin, S, heads, D).permute(0, 2, 1, 3).contiguous()
    o = ((q @ k.transpose(-1, -2)) * (D ** -0.5)).softmax(-1) @ v

    def ref():
        torch.autograd.grad(o, (q, k, v), do, retain_graph=True)

    row["torch_fp16_autograd_ms"] = timed(ref, reps)
    row["ratio_torch_over_new"] = row["torch_fp16_autograd_ms"] / row["new_ms"]
    return row


def bench_model(batch, steps):
    import torch.nn.functional as F
    import fastervit_amd
    torch.manual_seed(0)
    model = fastervit_amd.create_model("faster_vit_4_21k_384").cuda().enable_hat_backward(True, long_sequences=True).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    x = torch.randn(batch, 3, 384, 384, device="cuda")
    y = torch.randint(0, 1000, (batch,), device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        return loss

    step()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.time() - t0) / steps
    return dict(model="faster_vit_4_21k_384", batch=batch, step_s=dt, images_per_s=batch / dt, loss_finite=bool(torch.isfinite(loss)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", action="store_true", help="also time one fine-tuning step of the full faster_vit_4_21k_384")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_backward_long.json"))
    a = ap.parse_args()
    doc = dict(device=torch.cuda.get_device_name(0), reps=a.reps, flop_count="5 products x 2 S^2 D per (window, head); recomputed tiles not counted", cases=[])
    for c in CASES:
        row = bench_case(*c, a.reps)
        doc["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.model:
        doc["finetune_step"] = bench_model(a.batch, a.steps)
        print(json.dumps(doc["finetune_step"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
