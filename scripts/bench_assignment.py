#!/usr/bin/env python3
"""Time the device assignment solver (csrc/fvit_assign.hip) against the scipy path it can replace:

  (a) the solver alone   14 problems (7 sets x 2 images) of 900 x 20 and of 900 x 100 in ONE fvit_det_assign launch (table, offsets and workspace prepared
                         once), against what the scipy path does with the same cost matrices: one copy of all of them to the host, 14 calls of
                         linear_sum_assignment, the indices as tensors
  (b) the criterion step scripts/bench_criterion.py's DINO step (B = 2, Q = 900, C = 91, 20 targets per image, 7 matched and 6 denoising sets), forward +
                         backward, with HungarianMatcher(solver="device") against solver="scipy"

    python scripts/bench_assignment.py [--reps 7] [--iters 20] [--out profiles/bench_assignment.json]

The method of scripts/bench_criterion.py: both forms run in this process, interleaved rep by rep, each window bracketed by device events after a warm-up
of the same calls; the figure of a window is its time over ``iters`` calls, the figure recorded the median over ``reps`` windows, with the smallest and
largest window beside it.  The device form never waits for the device, so its windows are the longer of the host's and the device's time.  The
verdict of (b) is the issue's: the device path wins if every window of it is at or below every window of the scipy path.  Needs an MI355X."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_criterion import AUX, C, make_step, measure  # noqa: E402
from fastervit_amd import HungarianMatcher, SetCriterion, _lib  # noqa: E402
from tests import criterion_refs as R  # noqa: E402

SETS, B, Q = 7, 2, 900


def solver_forms(n_b, dev):
    from scipy.optimize import linear_sum_assignment
    g = torch.Generator().manual_seed(170 + n_b)
    sizes, T = [n_b] * B, n_b * B
    costs = [(2 * torch.randn(B, Q, T, generator=g)).to(dev) for _ in range(SETS)]
    P = sum(min(Q, n) for n in sizes)
    pairs = [torch.empty(2, P, dtype=torch.int64, device=dev) for _ in costs]
    status = torch.empty(SETS, B, dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, n_b, 2 * n_b, 0, min(Q, n_b), 2 * min(Q, n_b)], dtype=torch.int32, device=dev)
    lib = _lib.lib()
    table = (_lib.FvitDetAssignSet * SETS)(*[_lib.FvitDetAssignSet(cost=c.data_ptr(), src=p[0].data_ptr(), tgt=p[1].data_ptr(), Q=Q, T=T, n_pairs=P)
                                             for c, p in zip(costs, pairs)])
    need = int(lib.fvit_det_assign_workspace(table, SETS, B))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def device():
        _lib.check(lib.fvit_det_assign(table, SETS, B, offsets[:3].data_ptr(), offsets[3:].data_ptr(), n_b, status.data_ptr(), ws.data_ptr(), need,
                                       _lib.stream_ptr()), "fvit_det_assign")

    def scipy_loop():
        flat = torch.cat([c.reshape(-1) for c in costs]).cpu()
        out = []
        for block in flat.split([c.numel() for c in costs]):
            ind = [linear_sum_assignment(part[i]) for i, part in enumerate(block.view(B, Q, T).split(sizes, -1))]
            out.append([(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in ind])
        return out

    device()
    want = scipy_loop()
    torch.cuda.synchronize()
    assert (status == 0).all()
    for p, w in zip(pairs, want):
        assert torch.equal(p[0].cpu(), torch.cat([i for i, _ in w])) and torch.equal(p[1].cpu(), torch.cat([j for _, j in w])), "the two forms disagree"
    return dict(device=device, scipy=scipy_loop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_assignment.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assignment.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, iters=args.iters,
                  timing="device events around iters calls, median over reps windows, the two forms interleaved per rep; [min, max] over the windows")
    solver = {}
    for n_b in (20, 100):
        us, mm = measure(solver_forms(n_b, dev), args.reps, args.iters)
        solver[f"14x900x{n_b}"] = dict(us_per_call=us, us_min_max=mm, scipy_over_device=round(us["scipy"] / us["device"], 2))
        print(json.dumps({f"14x900x{n_b}": solver[f"14x900x{n_b}"]}), flush=True)
    result["solver_alone"] = solver

    outputs, targets = make_step(torch.Generator().manual_seed(16), dev)
    weights = R.weight_dict(AUX, True)
    leaves = [o[k] for _, o in R.pred_sets(outputs) for k in ("pred_logits", "pred_boxes")]
    crits = {s: SetCriterion(C, HungarianMatcher(**R.MATCH_WEIGHTS, solver=s), weights, R.FOCAL_ALPHA, list(R.LOSSES)) for s in ("device", "scipy")}

    def step(solver):
        def fn():
            for leaf in leaves:
                leaf.grad = None
            losses = crits[solver](outputs, targets)
            sum(losses[k] * weights[k] for k in losses if k in weights).backward()
            return losses
        return fn

    forms = dict(device=step("device"), scipy=step("scipy"))
    a, b = forms["device"](), forms["scipy"]()
    torch.cuda.synchronize()
    crits["device"].matcher.check_status()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a), "the two paths give different losses"
    us, mm = measure(forms, max(args.reps, 3), args.iters)
    result["criterion_step"] = dict(us_per_step=us, us_min_max=mm, scipy_over_device=round(us["scipy"] / us["device"], 2),
                                    every_device_window_at_or_below_every_scipy_window=bool(mm["device"][1] <= mm["scipy"][0]),
                                    host_synchronisations_per_step=dict(scipy=1, device=0, how="by construction, and tests/test_gpu_assignment.py runs the "
                                                                        "device path's forward with host synchronisation made an error"),
                                    parent_record_us=float(np.round(json.load(open(os.path.join(ROOT, "profiles", "bench_criterion.json")))["us_per_step"]["hip"], 1)))
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
