#!/usr/bin/env python3
"""Time the detection post-processing kernels (fastervit_amd.detection_ops, csrc/fvit_boxes.hip) against plain-torch forms of the same work on the same
device:

  (i)   select + decode at B = 2, Q = 900, C = 91, K = 300 (DINO's PostProcess without NMS) against the reference's torch sequence
        (sigmoid, topk, //, %, cxcywh -> xyxy, gather, mul); the HIP form as a plain launch and as a captured graph replay;
  (ii)  NMS at N = 300 and N = 4096 against a written-out torch loop (one IoU row and one host synchronisation per kept box); the HIP form as the
        ``nms`` call (stable sort + two kernels + the read of the count) and as the two kernels alone on sorted boxes;
  (iii) the matcher's cost at R = 1800, C = 91, T = 40 against the reference's torch sequence (two focal tensors, cdist, IoU / GIoU temporaries).

    python scripts/bench_postprocess.py [--reps 7] [--iters 20] [--out profiles/bench_postprocess.json]

All forms run in this process, interleaved rep by rep, each window bracketed by device events after a warm-up of the same calls; the figure of a window
is its time over ``iters`` calls (the torch NMS loop: over one call at N = 4096), the figure recorded the median over ``reps`` windows.  ``floor_us`` is
the time the bytes every form must at least move (inputs read once, outputs written once) take at 4 TB/s: for work this small it says how far from the
memory system's limit, and how close to launch latency, everything here is.  Needs an MI355X; there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastervit_amd import detection_ops as D  # noqa: E402

HBM_TBS = 4.0


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def measure(forms, reps, iters):
    """forms: name -> (fn, iters or None).  Interleaved windows; returns medians and (min, max)."""
    for fn, _ in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, (fn, it) in forms.items():
            times[k].append(window(fn, it or iters))
    return ({k: round(statistics.median(v), 1) for k, v in times.items()}, {k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()})


def torch_postprocess(logits, bbox, sizes, K):
    prob = logits.sigmoid()
    values, indexes = torch.topk(prob.view(logits.shape[0], -1), K, dim=1)
    topk_boxes = indexes // logits.shape[2]
    labels = indexes % logits.shape[2]
    boxes = torch.gather(D.box_cxcywh_to_xyxy(bbox), 1, topk_boxes.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    return values, labels, boxes * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]


def torch_nms_loop(boxes, scores, thr):
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    alive = torch.ones(b.shape[0], dtype=torch.bool, device=b.device)
    keep = []
    for i in range(b.shape[0]):
        if not alive[i].item():      # the host synchronisation of every portable NMS loop
            continue
        keep.append(i)
        w = (torch.minimum(b[i, 2], b[i + 1:, 2]) - torch.maximum(b[i, 0], b[i + 1:, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[i + 1:, 3]) - torch.maximum(b[i, 1], b[i + 1:, 1])).clamp(min=0)
        inter = w * h
        alive[i + 1:] &= ~(inter / (area[i] + area[i + 1:] - inter) > thr)
    return order[torch.tensor(keep, device=b.device)]


def torch_matcher_cost(logits, pred, ids, tgt, wc, wb, wg, alpha):
    p = logits.sigmoid()
    neg = (1 - alpha) * (p ** 2.0) * (-(1 - p + 1e-8).log())
    pos = alpha * ((1 - p) ** 2.0) * (-(p + 1e-8).log())
    c_class = pos[:, ids] - neg[:, ids]
    c_bbox = torch.cdist(pred, tgt, p=1)
    b1, b2 = D.box_cxcywh_to_xyxy(pred), D.box_cxcywh_to_xyxy(tgt)
    a1, a2 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]), (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = a1[:, None] + a2 - inter
    iou = inter / (union + 1e-6)
    wh = (torch.max(b1[:, None, 2:], b2[:, 2:]) - torch.min(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    area = wh[:, :, 0] * wh[:, :, 1]
    return wb * c_bbox + wc * c_class + wg * -(iou - (area - union) / (area + 1e-6))


def rand_cxcywh(n, g, dev):
    return torch.cat([0.2 + 0.6 * torch.rand(n, 2, generator=g), 0.05 + 0.35 * torch.rand(n, 2, generator=g)], 1).to(dev)


def floor_us(nbytes):
    return round(nbytes / (HBM_TBS * 1e12) * 1e6, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_postprocess.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_postprocess.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(15)
    rows = []

    # (i) select + decode
    B, Q, C, K = 2, 900, 91, 300
    logits = (torch.randn(B, Q, C, generator=g) - 2.0).to(dev)
    bbox = rand_cxcywh(B * Q, g, dev).view(B, Q, 4)
    sizes = torch.tensor([[800.0, 1333.0], [768.0, 1024.0]], device=dev)
    s, l, q, b = (torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.int64, device=dev), torch.empty(B, K, dtype=torch.int64, device=dev),
                  torch.empty(B, K, 4, device=dev))
    hip = lambda: D.postprocess_launch(logits, bbox, sizes, s, l, b, q)
    hip()
    ref = torch_postprocess(logits, bbox, sizes, K)
    same = bool(torch.equal(l, ref[1]) and torch.equal(b, ref[2]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip()
    us, mm = measure(dict(hip_launch=(hip, None), hip_graph_replay=(graph.replay, None), torch_sequence=(lambda: torch_postprocess(logits, bbox, sizes, K), None)),
                     args.reps, args.iters)
    nbytes = B * Q * C * 4 + B * K * (4 + 8 + 8 + 16 + 16)
    rows.append(dict(op="select_decode", B=B, Q=Q, C=C, K=K, us=us, us_min_max=mm, torch_over_hip=round(us["torch_sequence"] / us["hip_launch"], 2),
                     min_bytes=nbytes, floor_us=floor_us(nbytes), labels_and_boxes_equal_torch=same))
    print(json.dumps(rows[-1]), flush=True)

    # (ii) NMS
    for N in (300, 4096):
        side_len = 100.0 if N == 300 else 400.0      # the same crowding at both sizes
        c = side_len * torch.rand(N, 2, generator=g)
        wh = 20.0 + 40.0 * torch.rand(N, 2, generator=g)
        boxes = torch.cat([c - 0.5 * wh, c + 0.5 * wh], 1).to(dev)
        scores = torch.rand(N, generator=g).to(dev)
        sorted_boxes = boxes[torch.sort(scores, descending=True, stable=True).indices].contiguous()
        keep, count, ws = torch.empty(1, N, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev), D.nms_workspace(1, N, dev)
        kernels = lambda: D._nms_launch(sorted_boxes, None, None, 0.5, keep, count, ws, 1, N)
        got, want = D.nms(boxes, scores, 0.5), torch_nms_loop(boxes, scores, 0.5)
        us, mm = measure(dict(hip_nms_call=(lambda: D.nms(boxes, scores, 0.5), None), hip_kernels_only=(kernels, None),
                              torch_loop=(lambda: torch_nms_loop(boxes, scores, 0.5), 1 if N > 1000 else 3)), args.reps, args.iters)
        nb = (N + 63) // 64
        nbytes = N * 16 + N * 8 + N * nb * 8      # boxes, keep, the upper-triangle half of the mask words written once and read once
        rows.append(dict(op="nms", N=N, kept=int(got.numel()), us=us, us_min_max=mm, torch_over_hip=round(us["torch_loop"] / us["hip_nms_call"], 1),
                         min_bytes=nbytes, floor_us=floor_us(nbytes), keep_equal_torch=bool(torch.equal(got, want))))
        print(json.dumps(rows[-1]), flush=True)

    # (iii) the matcher's cost
    R_, C, T = 1800, 91, 40
    logits = (1.5 * torch.randn(R_, C, generator=g) - 1.0).to(dev)
    pred, tgt = rand_cxcywh(R_, g, dev), rand_cxcywh(T, g, dev)
    ids = torch.randint(0, C, (T,), generator=g).to(dev)
    m = D.HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    outputs, targets = {"pred_logits": logits.view(2, 900, C), "pred_boxes": pred.view(2, 900, 4)}, [{"labels": ids[:25], "boxes": tgt[:25]}, {"labels": ids[25:], "boxes": tgt[25:]}]
    hip = lambda: m.cost_matrix(outputs, targets)
    tor = lambda: torch_matcher_cost(logits, pred, ids, tgt, 2.0, 5.0, 2.0, 0.25)
    diff = (hip().view(R_, T) - tor()).abs().max().item()
    us, mm = measure(dict(hip_cost_matrix=(hip, None), torch_sequence=(tor, None)), args.reps, args.iters)
    nbytes = R_ * T * 4 + R_ * T * 4 + R_ * 16 + T * 24      # one gathered logit per element (cache lines: more), the output, the boxes
    rows.append(dict(op="matcher_cost", R=R_, C=C, T=T, us=us, us_min_max=mm, torch_over_hip=round(us["torch_sequence"] / us["hip_cost_matrix"], 2),
                     min_bytes=nbytes, floor_us=floor_us(nbytes), max_abs_diff_vs_torch=diff))
    print(json.dumps(rows[-1]), flush=True)

    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, iters=args.iters,
                  timing="device events around iters calls (the torch NMS loop: 3 calls at N = 300, 1 at N = 4096), median over reps windows, forms interleaved "
                         "per rep; hip_cost_matrix and hip_nms_call include their torch glue (cat of the targets, the stable sort, the read of the count)",
                  floor="min_bytes at %.1f TB/s" % HBM_TBS, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
