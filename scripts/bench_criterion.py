#!/usr/bin/env python3
"""Time one DINO training step of the criterion (fastervit_amd.criterion, csrc/fvit_loss.hip), forward + backward, against the reference-shaped torch
form of the same criterion on the same device:

  shape    B = 2, Q = 900, C = 91, 20 targets per image; 7 matched sets (main, 5 aux, interm) and 6 denoising sets of 200 queries (5 groups of 40)
  hip      SetCriterion(HungarianMatcher): every cost matrix from its kernel, ONE copy to the host, scipy, then one label launch, one box launch and,
           in backward, one launch each
  torch    tests/criterion_refs.py moved to the device: per set the matcher's cost matrix in torch and its own copy to the host, the (B, Q, C + 1) one-hot,
           the elementwise focal passes, L1 and GIoU, and autograd's replay of all of them

    python scripts/bench_criterion.py [--reps 7] [--iters 20] [--out profiles/bench_criterion.json]

The method of scripts/bench_postprocess.py: both forms run in this process, interleaved rep by rep, each window bracketed by device events after a
warm-up of the same calls; the figure of a window is its time over ``iters`` steps, the figure recorded the median over ``reps`` windows.  A step ends
with the gradients of every pred_logits / pred_boxes in place.  Kernel launches and copies per step are counted with torch.profiler over one step of each
form (null when the profiler is not available); this library's own launches come from its built-in timer.  Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastervit_amd import HungarianMatcher, SetCriterion, _lib  # noqa: E402
from tests import criterion_refs as R  # noqa: E402

B, Q, C, NT, AUX, GROUPS, SINGLE_PAD = 2, 900, 91, 20, 5, 5, 40


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per step


def measure(forms, reps, iters):
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(window(fn, iters))
    return ({k: round(statistics.median(v), 1) for k, v in times.items()}, {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()})


def make_step(g, dev):
    def one(q):
        return {"pred_logits": (1.5 * torch.randn(B, q, C, generator=g) - 1.0).to(dev).requires_grad_(True),
                "pred_boxes": torch.cat([0.2 + 0.6 * torch.rand(B, q, 2, generator=g), 0.05 + 0.35 * torch.rand(B, q, 2, generator=g)], -1).to(dev).requires_grad_(True)}
    outputs = one(Q)
    outputs["aux_outputs"] = [one(Q) for _ in range(AUX)]
    outputs["interm_outputs"] = one(Q)
    known = one(GROUPS * SINGLE_PAD)
    known["aux_outputs"] = [one(GROUPS * SINGLE_PAD) for _ in range(AUX)]
    outputs["dn_meta"] = {"output_known_lbs_bboxes": known, "num_dn_group": GROUPS, "pad_size": GROUPS * SINGLE_PAD}
    targets = [{"labels": torch.randint(0, C, (NT,), generator=g).to(dev),
                "boxes": torch.cat([0.2 + 0.6 * torch.rand(NT, 2, generator=g), 0.05 + 0.35 * torch.rand(NT, 2, generator=g)], -1).to(dev)} for _ in range(B)]
    return outputs, targets


def count_events(fn):
    """(kernel launches, memcpys) of one call, from torch.profiler; (None, None) when it cannot be used here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        copies = [e for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower()]
        return len(dev) - len(copies), len(copies)
    except Exception as e:      # noqa: BLE001  (a missing tracer must not lose the timings)
        print(f"torch.profiler is not usable here: {e}", flush=True)
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_criterion.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_criterion.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    outputs, targets = make_step(torch.Generator().manual_seed(16), dev)
    weights = R.weight_dict(AUX, True)
    crit = SetCriterion(C, HungarianMatcher(**R.MATCH_WEIGHTS), weights, R.FOCAL_ALPHA, list(R.LOSSES))
    leaves = [o[k] for _, o in R.pred_sets(outputs) for k in ("pred_logits", "pred_boxes")]

    def clear():
        for leaf in leaves:
            leaf.grad = None

    def hip_step():
        clear()
        losses = crit(outputs, targets)
        sum(losses[k] * weights[k] for k in losses if k in weights).backward()
        return losses

    def torch_step():
        clear()
        indices = [R.match(o, targets, torch.float32) for o in R.matched_sets(outputs)]      # one cost matrix and one copy to the host per set
        terms, scalars = R.criterion(outputs, targets, indices, torch.float32)
        R.total(terms, weights).backward()
        return {**{k: v.sum() for k, v in terms.items()}, **scalars}

    a = hip_step()
    ga = [leaf.grad.clone() for leaf in leaves]
    b = torch_step()
    gb = [leaf.grad.clone() for leaf in leaves]
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b), "the two forms return different key sets"
    loss_diff = max(abs(a[k].item() - b[k].item()) / max(abs(b[k].item()), 1e-6) for k in a)
    grad_diff = max((x - y).abs().max().item() / max(y.abs().max().item(), 1e-12) for x, y in zip(ga, gb))

    _lib.prof_enable(True)
    hip_step()
    torch.cuda.synchronize()
    own = {}
    for r in _lib.prof_records():
        own[r["name"]] = own.get(r["name"], 0) + 1
    _lib.prof_enable(False)
    counts = {"hip": count_events(hip_step), "torch": count_events(torch_step)}

    us, mm = measure(dict(hip=hip_step, torch=torch_step), args.reps, args.iters)
    n_sets = len(R.pred_sets(outputs))
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, iters=args.iters,
                  shape=dict(B=B, Q=Q, C=C, targets_per_image=NT, matched_sets=2 + AUX, dn_sets=1 + AUX, dn_queries=GROUPS * SINGLE_PAD, sets=n_sets),
                  timing="forward + backward of one step; device events around iters steps, median over reps windows, the two forms interleaved per rep",
                  us_per_step=us, us_min_max=mm, torch_over_hip=round(us["torch"] / us["hip"], 2),
                  library_launches_per_step=own,
                  device_kernels_per_step=dict(hip=counts["hip"][0], torch=counts["torch"][0]),
                  device_copies_per_step=dict(hip=counts["hip"][1], torch=counts["torch"][1]),
                  host_synchronisations_per_step=dict(hip=1, torch=2 + AUX + 2,
                                                      how="by construction: hip = the one copy of the concatenated cost matrices; torch = per matched set the copy "
                                                          "of its cost matrix, and the two reads behind class_error (the reference reads num_boxes once more)"),
                  max_rel_loss_diff_between_forms=loss_diff, max_rel_grad_diff_between_forms=grad_diff)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
