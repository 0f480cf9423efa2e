#!/usr/bin/env python3
"""Time multi-scale deformable attention (fastervit_amd.ops.ms_deform_attn, csrc/fvit_msda.hip) against the grid_sample form of the same op on the
same device, at the two shapes of the reference's DINO 4-scale configuration at 800 x 1333: N = 2, M = 8, D = 32, P = 4, levels 100x167, 50x84, 25x42,
13x21 (S = 22223); encoder Lq = S, decoder Lq = 900; fp32 and fp16 value.

    python scripts/bench_msda.py [--reps 7] [--iters 10] [--out profiles/bench_msda.json]

Both forms run in this process, interleaved rep by rep (HIP forward, grid_sample forward, HIP forward + backward, grid_sample forward + backward), each
window bracketed by device events after a warm-up of the same calls; the figure of a window is its time over ``iters`` calls, the figure recorded the
median over ``reps`` windows (min and max beside it).  For an fp16 value the grid_sample form does what the reference's module does under autocast:
it widens value to fp32 first and narrows the result.  Byte counts are computed from the shapes: the forward gathers four rows of D elements per sample,
the backward adds four rows of D floats per sample with float atomics (chip-wide rate of such adds on this part: about 1.3 TB/s).  Needs an MI355X;
there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastervit_amd.ops import ms_deform_attn  # noqa: E402

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
N, M, D, P = 2, 8, 32, 4
ATOMIC_RATE_TBS = 1.3


def grid_sample_form(value, levels, loc, attn):
    """The op through F.grid_sample: one (N * M, D, Lq, P) tensor of samples per level, weighted and summed afterwards."""
    n, _, m, d = value.shape
    lq, nl, p = loc.shape[1], loc.shape[3], loc.shape[4]
    grid = 2.0 * loc - 1.0
    sampled, start = [], 0
    for l, (h, w) in enumerate(levels):
        maps = value[:, start:start + h * w].permute(0, 2, 3, 1).reshape(n * m, d, h, w)
        g = grid[:, :, :, l].permute(0, 2, 1, 3, 4).reshape(n * m, lq, p, 2)
        sampled.append(F.grid_sample(maps, g, mode="bilinear", padding_mode="zeros", align_corners=False))
        start += h * w
    weights = attn.permute(0, 2, 1, 3, 4).reshape(n * m, 1, lq, nl * p)
    return (torch.cat(sampled, -1) * weights).sum(-1).view(n, m * d, lq).transpose(1, 2).contiguous()


def make_inputs(name, dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(20 + len(name))
    shapes = torch.tensor(LEVELS, dtype=torch.int64)
    sizes = shapes[:, 0] * shapes[:, 1]
    starts = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]])
    S, L = int(sizes.sum()), len(LEVELS)
    wh = shapes.flip(-1).float()
    if name == "encoder":      # every pixel of every level is a query that looks around its own position, a few pixels away
        Lq = S
        ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"), -1).flip(-1).reshape(-1, 2)
                         for h, w in LEVELS])[None, :, None, None, None, :]
        spread = 2.0
    else:                      # 900 object queries anywhere in the image, looking further
        Lq = 900
        ref = torch.rand(N, Lq, 1, 1, 1, 2, generator=g)
        spread = 4.0
    loc = (ref + spread * torch.randn(N, Lq, M, L, P, 2, generator=g) / wh[None, None, None, :, None, :]).contiguous()
    attn = torch.randn(N, Lq, M, L * P, generator=g).softmax(-1).view(N, Lq, M, L, P)
    value = torch.randn(N, S, M, D, generator=g)
    grad = torch.randn(N, Lq, M * D, generator=g)
    return dict(value=value.to(dev, dtype), shapes=shapes.to(dev), starts=starts.to(dev), loc=loc.to(dev), attn=attn.to(dev), grad=grad.to(dev, dtype), Lq=Lq, S=S)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_msda.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_msda.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for name in ("encoder", "decoder"):
        for dtype in (torch.float32, torch.float16):
            d = make_inputs(name, dtype, dev)
            leaves = [d[k].clone().requires_grad_(True) for k in ("value", "loc", "attn")]

            def hip_fwd():
                with torch.no_grad():
                    return ms_deform_attn(d["value"], d["shapes"], d["starts"], d["loc"], d["attn"])

            def gs_fwd():
                with torch.no_grad():
                    return grid_sample_form(d["value"].float(), LEVELS, d["loc"], d["attn"]).to(dtype)

            def hip_train():
                out = ms_deform_attn(leaves[0], d["shapes"], d["starts"], leaves[1], leaves[2])
                return torch.autograd.grad(out, leaves, d["grad"])

            def gs_train():
                out = grid_sample_form(leaves[0].float(), LEVELS, leaves[1], leaves[2]).to(dtype)
                return torch.autograd.grad(out, leaves, d["grad"])

            forms = dict(hip_fwd=hip_fwd, gs_fwd=gs_fwd, hip_fwd_bwd=hip_train, gs_fwd_bwd=gs_train)
            diff = (hip_fwd().float() - gs_fwd().float()).abs().max().item()
            gh, gg = hip_train(), gs_train()
            gdiff = [((a.float() - b.float()).abs().max() / b.float().abs().max()).item() for a, b in zip(gh, gg)]
            del gh, gg
            for fn in forms.values():          # warm-up: code objects, allocator pools
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.reps):         # interleaved: every rep times all four forms
                for k, fn in forms.items():
                    times[k].append(window(fn, args.iters))
            us = {k: statistics.median(v) for k, v in times.items()}
            samples = N * d["Lq"] * M * len(LEVELS) * P
            gather_bytes = samples * 4 * D * (4 if dtype == torch.float32 else 2)
            atomic_bytes = samples * 4 * D * 4
            bwd_us = us["hip_fwd_bwd"] - us["hip_fwd"]
            row = dict(shape=name, value_dtype=str(dtype).replace("torch.", ""), N=N, Lq=d["Lq"], S=d["S"], M=M, D=D, L=len(LEVELS), P=P,
                       us={k: round(v, 1) for k, v in us.items()},
                       us_min_max={k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                       speedup_fwd=round(us["gs_fwd"] / us["hip_fwd"], 2), speedup_fwd_bwd=round(us["gs_fwd_bwd"] / us["hip_fwd_bwd"], 2),
                       fwd_gathered_bytes=gather_bytes, fwd_gathered_TBps=round(gather_bytes / us["hip_fwd"] * 1e-6, 3),
                       bwd_atomic_bytes=atomic_bytes, bwd_us_fwd_bwd_minus_fwd=round(bwd_us, 1),
                       bwd_atomic_TBps=round(atomic_bytes / bwd_us * 1e-6, 3), atomic_rate_of_the_part_TBps=ATOMIC_RATE_TBS,
                       bwd_atomic_floor_us=round(atomic_bytes / (ATOMIC_RATE_TBS * 1e12) * 1e6, 1),
                       max_abs_diff_out_vs_grid_sample=diff, max_rel_diff_grads_vs_grid_sample=dict(zip(("value", "loc", "attn"), gdiff)))
            print(json.dumps(row), flush=True)
            rows.append(row)
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, iters=args.iters,
                  timing="device events around iters calls, median over reps windows, the four forms interleaved per rep; "
                         "bwd time = (forward + backward) - forward, it includes autograd's bookkeeping and the zero-fill of grad_value",
                  yardstick="F.grid_sample form of the same op in the same process (fp16 value: widened to fp32 first, as the reference does under autocast)",
                  rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
