"""What comes after the DINO heads, on the gfx950 kernels of csrc/fvit_boxes.hip -- DESIGN.md section 15.

Drop-ins, by signature and result, for what the reference's detection code takes from ``util/box_ops.py``, ``torchvision.ops.boxes``, ``dino.py``
(``PostProcess``) and ``matcher.py`` (``HungarianMatcher``):

    box_cxcywh_to_xyxy, box_xyxy_to_cxcywh     plain torch (elementwise, differentiable)
    box_iou(b1, b2) -> (iou, union)            (N, 4) x (M, 4) -> (N, M), the reference's form with 1e-6 in the quotient
    generalized_box_iou(b1, b2) -> giou        the same, 1e-6 in both quotients
    nms(boxes, scores, thr), batched_nms(boxes, scores, idxs, thr)      torchvision's rule and results: int64 indices by descending score
    PostProcess(num_select, nms_iou_threshold)                          the reference's list of dicts; postprocess_launch is its capturable form
    HungarianMatcher(cost_class, cost_bbox, cost_giou, focal_alpha)     the cost matrix from one kernel, one copy to the host, scipy imported lazily
    hungarian_assign(cost, sizes), HungarianMatcher(solver="device")    the assignment itself on the device: no copy to the host

The pairwise ops are forward only: an input that requires grad while grad mode is on raises (the differentiable GIoU of the losses, over matched pairs,
lives in criterion.py).  The reference's ``generalized_box_iou`` asserts ``(boxes[:, 2:] >= boxes[:, :2]).all()``, a host synchronisation per call; it is deliberately
not kept: a degenerate box gives the value the formula gives.  16-bit inputs are widened to fp32 here and results narrowed back once; float64 is refused
by name; a CPU tensor raises (there is no CPU or eager fallback).  Ties in the top-k go to the lower flat index ``q * C + c``.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib

__all__ = ["box_cxcywh_to_xyxy", "box_xyxy_to_cxcywh", "box_iou", "generalized_box_iou", "nms", "batched_nms", "PostProcess", "postprocess_launch",
           "HungarianMatcher", "hungarian_assign", "NMS_MAX_BOXES", "SELECT_MAX_K", "ASSIGN_MAX_SIDE"]

NMS_MAX_BOXES = 8192
ASSIGN_MAX_SIDE = 2048      # queries, and targets of one image, the device assignment solver takes
SELECT_MAX_K = 1024
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


def box_cxcywh_to_xyxy(x):
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([x_c - 0.5 * w, y_c - 0.5 * h, x_c + 0.5 * w, y_c + 0.5 * h], dim=-1)


def box_xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x.unbind(-1)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], dim=-1)


def _float_input(who, name, t, grad_ok=True):
    """The checks only the Python side can make; returns the tensor as dense, 16-byte aligned fp32."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); {name} is a {t.device.type} tensor and there is no CPU fallback")
    if t.dtype == torch.float64:
        raise RuntimeError(f"{who}: {name} is float64, which is not supported (float32, float16 or bfloat16)")
    if t.dtype not in _FLOATS:
        raise RuntimeError(f"{who}: {name} has dtype {t.dtype}; float32, float16 or bfloat16 is expected")
    if not grad_ok and t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{who} is forward only: {name} requires grad and there is no backward kernel (call it under torch.no_grad() or detach)")
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _pairwise(who, mode, boxes1, boxes2):
    dt = boxes1.dtype if isinstance(boxes1, torch.Tensor) else None
    b1 = _float_input(who, "boxes1", boxes1, grad_ok=False)
    b2 = _float_input(who, "boxes2", boxes2, grad_ok=False)
    if b1.dim() != 2 or b2.dim() != 2 or b1.shape[1] != 4 or b2.shape[1] != 4:
        raise RuntimeError(f"{who}: expected boxes1 (N, 4) and boxes2 (M, 4), got {tuple(b1.shape)} and {tuple(b2.shape)}")
    N, M = b1.shape[0], b2.shape[0]
    out = torch.empty(N, M, dtype=torch.float32, device=b1.device)
    union = torch.empty(N, M, dtype=torch.float32, device=b1.device) if mode == _lib.FVIT_BOX_IOU else None
    with torch.cuda.device(b1.device):
        _lib.check(_lib.lib().fvit_box_pairwise(mode, b1.data_ptr(), b2.data_ptr(), out.data_ptr(), union.data_ptr() if union is not None else None, N, M,
                                                _lib.stream_ptr()), "fvit_box_pairwise")
    if dt != torch.float32:
        out = out.to(dt)
        union = union.to(dt) if union is not None else None
    return out, union


def box_iou(boxes1, boxes2):
    """(iou, union), both (N, M): inter / (union + 1e-6) and area1 + area2 - inter of xyxy boxes.  Forward only."""
    return _pairwise("box_iou", _lib.FVIT_BOX_IOU, boxes1, boxes2)


def generalized_box_iou(boxes1, boxes2):
    """(N, M) GIoU of xyxy boxes: iou - (area - union) / (area + 1e-6), area = the enclosing box.  Forward only; degenerate boxes are not asserted on."""
    return _pairwise("generalized_box_iou", _lib.FVIT_BOX_GIOU, boxes1, boxes2)[0]


def _nms_launch(boxes, order, idxs, thr, keep, count, workspace, G, N):
    lib = _lib.lib()
    with torch.cuda.device(boxes.device):
        _lib.check(lib.fvit_box_nms(boxes.data_ptr(), order.data_ptr() if order is not None else None, idxs.data_ptr() if idxs is not None else None,
                                    float(thr), keep.data_ptr(), count.data_ptr(), workspace.data_ptr(), workspace.numel(), G, N, _lib.stream_ptr()), "fvit_box_nms")


def nms_workspace(G: int, N: int, device) -> torch.Tensor:
    """The mask workspace fvit_box_nms needs for G groups of N boxes (uint8 tensor)."""
    if N > NMS_MAX_BOXES:
        raise RuntimeError(f"nms: N={N} boxes per group is not supported (N <= {NMS_MAX_BOXES})")
    return torch.empty(max(int(_lib.lib().fvit_box_nms_workspace(G, N)), 8), dtype=torch.uint8, device=device)


def _nms(who, boxes, scores, idxs, iou_threshold):
    b = _float_input(who, "boxes", boxes)
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); scores is not a tensor on it and there is no CPU fallback")
    if scores.dtype == torch.float64:
        raise RuntimeError(f"{who}: scores is float64, which is not supported (float32, float16 or bfloat16)")
    if b.dim() != 2 or b.shape[1] != 4 or scores.dim() != 1 or scores.shape[0] != b.shape[0]:
        raise RuntimeError(f"{who}: expected boxes (N, 4) and scores (N,), got {tuple(b.shape)} and {tuple(scores.shape)}")
    N = b.shape[0]
    if idxs is not None:
        if not idxs.is_cuda:
            raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); idxs is a {idxs.device.type} tensor and there is no CPU fallback")
        if tuple(idxs.shape) != (N,):
            raise RuntimeError(f"{who}: idxs must be ({N},), got {tuple(idxs.shape)}")
        idxs = idxs.to(torch.int64).contiguous()
    if N > NMS_MAX_BOXES:
        raise RuntimeError(f"{who}: N={N} boxes is not supported (N <= {NMS_MAX_BOXES})")
    if N == 0:
        return torch.empty(0, dtype=torch.int64, device=b.device)
    order = torch.sort(scores.detach(), descending=True, stable=True).indices.contiguous()
    keep = torch.empty(N, dtype=torch.int64, device=b.device)
    count = torch.empty(1, dtype=torch.int32, device=b.device)
    _nms_launch(b, order, idxs, iou_threshold, keep, count, nms_workspace(1, N, b.device), 1, N)
    return keep[:int(count.item())]      # the one host read


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: the indices (int64, by descending score) of the boxes (N, 4) xyxy that no kept box of higher score overlaps with IoU > threshold."""
    return _nms("nms", boxes, scores, None, iou_threshold)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.batched_nms: NMS in which boxes of different ``idxs`` never suppress each other."""
    if idxs is None:
        raise RuntimeError("batched_nms: idxs is required (use nms without class ids)")
    return _nms("batched_nms", boxes, scores, idxs, iou_threshold)


def postprocess_launch(pred_logits, pred_boxes, target_sizes, scores, labels, boxes, query=None, *, not_to_xyxy=False, test=False,
                       nms_iou_threshold=-1.0, keep=None, count=None, workspace=None):
    """The capturable form of PostProcess: launches only, into caller-owned outputs; no allocation, no host read.

    pred_logits (B, Q, C), pred_boxes (B, Q, 4) and target_sizes (B, 2) = (h, w): dense fp32 device tensors.  scores (B, K) fp32, labels (B, K) int64,
    boxes (B, K, 4) fp32 and the optional query (B, K) int64 receive the K = scores.shape[1] best candidates of every image by descending score.  With
    nms_iou_threshold > 0, keep (B, K) int64 receives per image the positions (into the K candidates) that survive NMS, padded with -1, count (B,) int32
    how many; workspace comes from ``nms_workspace(B, K, device)``."""
    who = "postprocess_launch"
    for name, t in (("pred_logits", pred_logits), ("pred_boxes", pred_boxes), ("target_sizes", target_sizes), ("scores", scores), ("boxes", boxes)):
        if not t.is_cuda:
            raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); {name} is a {t.device.type} tensor and there is no CPU fallback")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{who}: {name} must be a dense float32 tensor (got {t.dtype}{'' if t.is_contiguous() else ', not contiguous'}); "
                               "PostProcess.forward widens 16-bit inputs")
    if pred_logits.dim() != 3 or pred_boxes.dim() != 3 or pred_boxes.shape[2] != 4 or tuple(pred_boxes.shape[:2]) != tuple(pred_logits.shape[:2]):
        raise RuntimeError(f"{who}: expected pred_logits (B, Q, C) and pred_boxes (B, Q, 4), got {tuple(pred_logits.shape)} and {tuple(pred_boxes.shape)}")
    B, Q, C = pred_logits.shape
    K = scores.shape[-1]
    if tuple(target_sizes.shape) != (B, 2):
        raise RuntimeError(f"{who}: target_sizes must be ({B}, 2) rows (h, w), got {tuple(target_sizes.shape)}")
    if tuple(scores.shape) != (B, K) or tuple(labels.shape) != (B, K) or tuple(boxes.shape) != (B, K, 4) or labels.dtype != torch.int64 or \
            not labels.is_contiguous() or not labels.is_cuda:
        raise RuntimeError(f"{who}: outputs must be scores ({B}, K) float32, labels ({B}, K) int64 and boxes ({B}, K, 4) float32 on the device")
    if query is None:
        query = labels.new_empty(B, K) if not torch.cuda.is_current_stream_capturing() else None
        if query is None:
            raise RuntimeError(f"{who}: pass query (B, K) int64 when capturing (the call allocates nothing)")
    elif tuple(query.shape) != (B, K) or query.dtype != torch.int64 or not query.is_contiguous() or not query.is_cuda:
        raise RuntimeError(f"{who}: query must be a dense ({B}, {K}) int64 device tensor")
    lib = _lib.lib()
    with torch.cuda.device(pred_logits.device):
        _lib.check(lib.fvit_det_select(pred_logits.data_ptr(), pred_boxes.data_ptr(), target_sizes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                       query.data_ptr(), boxes.data_ptr(), B, Q, C, K, int(bool(not_to_xyxy)), int(bool(test)), _lib.stream_ptr()), "fvit_det_select")
    if nms_iou_threshold > 0:
        if keep is None or count is None or workspace is None:
            raise RuntimeError(f"{who}: with NMS on, keep (B, K) int64, count (B,) int32 and workspace (nms_workspace(B, K, device)) are required")
        if tuple(keep.shape) != (B, K) or keep.dtype != torch.int64 or tuple(count.shape) != (B,) or count.dtype != torch.int32 or \
                not keep.is_contiguous() or not (keep.is_cuda and count.is_cuda and workspace.is_cuda) or workspace.dtype != torch.uint8:
            raise RuntimeError(f"{who}: keep must be ({B}, {K}) int64, count ({B},) int32 and workspace uint8, all on the device")
        _nms_launch(boxes, None, None, nms_iou_threshold, keep, count, workspace, B, K)     # the candidates are already in score order


class PostProcess(nn.Module):
    """DINO's PostProcess: the num_select best (query, class) pairs of every image as ``[{'scores', 'labels', 'boxes'}]``, boxes scaled to target_sizes,
    optionally thinned by NMS.  One select + decode launch per batch (plus two for NMS); one host read, of the NMS counts, and only when NMS is on."""

    def __init__(self, num_select=100, nms_iou_threshold=-1) -> None:
        super().__init__()
        self.num_select = num_select
        self.nms_iou_threshold = nms_iou_threshold

    @torch.no_grad()
    def forward(self, outputs, target_sizes, not_to_xyxy=False, test=False):
        out_logits, out_bbox = outputs["pred_logits"], outputs["pred_boxes"]
        assert len(out_logits) == len(target_sizes)
        assert target_sizes.shape[1] == 2
        if test:
            assert not not_to_xyxy
        dt = out_logits.dtype
        logits = _float_input("PostProcess", "pred_logits", out_logits)
        bbox = _float_input("PostProcess", "pred_boxes", out_bbox)
        if not target_sizes.is_cuda:
            raise RuntimeError("PostProcess runs only on a HIP device (libfvit_hip.so kernels); target_sizes is a cpu tensor and there is no CPU fallback")
        if target_sizes.dtype == torch.float64:
            raise RuntimeError("PostProcess: target_sizes is float64, which is not supported (an integer type, float32, float16 or bfloat16)")
        sizes = target_sizes.to(torch.float32).contiguous()
        B, K, dev = logits.shape[0], int(self.num_select), logits.device
        scores = torch.empty(B, K, dtype=torch.float32, device=dev)
        labels = torch.empty(B, K, dtype=torch.int64, device=dev)
        query = torch.empty(B, K, dtype=torch.int64, device=dev)
        boxes = torch.empty(B, K, 4, dtype=torch.float32, device=dev)
        use_nms = self.nms_iou_threshold > 0
        keep = count = ws = None
        if use_nms:
            keep = torch.empty(B, K, dtype=torch.int64, device=dev)
            count = torch.empty(B, dtype=torch.int32, device=dev)
            ws = nms_workspace(B, K, dev)
        postprocess_launch(logits, bbox, sizes, scores, labels, boxes, query, not_to_xyxy=not_to_xyxy, test=test,
                           nms_iou_threshold=float(self.nms_iou_threshold), keep=keep, count=count, workspace=ws)
        if dt != torch.float32:
            scores, boxes = scores.to(dt), boxes.to(out_bbox.dtype)
        if not use_nms:
            return [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(scores, labels, boxes)]
        counts = count.tolist()      # the one host read
        results = []
        for s, l, b, k, n in zip(scores, labels, boxes, keep, counts):
            i = k[:n]
            results.append({"scores": s[i], "labels": l[i], "boxes": b[i]})
        return results


def _host_to_device(values, dtype, device):
    """A host list as a device tensor through pinned memory and an asynchronous copy: no synchronisation of the stream."""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def assign_launch(costs, sizes):
    """The solver of csrc/fvit_assign.hip on a list of dense fp32 device (B, Q, T) cost matrices that share ``sizes`` (the host list of targets per
    image) and min(Q, n_b): ceil(len / 16) launches.  Returns (pairs, status): per set an int64 (2, P) device tensor, row 0 the queries and row 1 the
    image-local targets, image b's k_b = min(Q, n_b) pairs at the prefix sum of k, and the int32 (len, B) status.  No device-to-host copy."""
    who = "hungarian_assign"
    lib = _lib.lib()
    dev = costs[0].device
    B, T = len(sizes), int(sum(sizes))
    ks = None
    for c in costs:
        if c.dim() != 3 or c.shape[0] != B or c.shape[2] != T or c.shape[1] < 1:
            raise RuntimeError(f"{who}: cost must be (B, Q, T) with B = {B} images, Q >= 1 and T = {T} targets (the sum of sizes), got {tuple(c.shape)}")
        k = [min(int(c.shape[1]), n) for n in sizes]
        if ks is not None and k != ks:
            raise RuntimeError(f"{who}: the sets of one call share their pair offsets, so min(Q, n_b) must be the same in every set")
        ks = k
    P = sum(ks)
    pairs = [torch.empty(2, P, dtype=torch.int64, device=dev) for _ in costs]
    status = torch.zeros(len(costs), B, dtype=torch.int32, device=dev)
    if T == 0:
        return pairs, status
    offs = []
    for counts in (sizes, ks):
        offs.append(0)
        for n in counts:
            offs.append(offs[-1] + n)
    offsets = _host_to_device(offs, torch.int32, dev)             # toff [B + 1], then pair_off [B + 1]
    toff, pair_off = offsets[:B + 1], offsets[B + 1:]
    with torch.cuda.device(dev):
        for lo in range(0, len(costs), _lib.FVIT_DET_MAX_SETS):
            part = costs[lo:lo + _lib.FVIT_DET_MAX_SETS]
            table = (_lib.FvitDetAssignSet * len(part))(*[
                _lib.FvitDetAssignSet(cost=c.data_ptr(), src=pairs[lo + s][0].data_ptr(), tgt=pairs[lo + s][1].data_ptr(), Q=c.shape[1], T=T, n_pairs=P)
                for s, c in enumerate(part)])
            need = int(lib.fvit_det_assign_workspace(table, len(part), B))
            if need == 0:
                _lib.check(-1, "fvit_det_assign_workspace")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(lib.fvit_det_assign(table, len(part), B, toff.data_ptr(), pair_off.data_ptr(), max(sizes), status[lo:lo + len(part)].data_ptr(),
                                           ws.data_ptr(), need, _lib.stream_ptr()), "fvit_det_assign")
    return pairs, status


def _split_pairs(pairs, ks):
    out, lo = [], 0
    for k in ks:
        out.append((pairs[0, lo:lo + k], pairs[1, lo:lo + k]))
        lo += k
    return out


def hungarian_assign(cost, sizes):
    """scipy.optimize.linear_sum_assignment of every image's block ``cost[b, :, sum(sizes[:b]) : sum(sizes[:b + 1])]`` of a device (B, Q, T) cost matrix,
    solved on the device (csrc/fvit_assign.hip).  ``sizes`` is the host list of targets per image.  Returns ([(src, tgt)] per image, status): int64 device
    views of one buffer, src ascending, min(Q, n_b) pairs each, and the int32 (B,) device status (0 solved; 1 a non-finite cost, the pairing is then the
    identity; 2 / 3 see include/fvit_hip.h).  16-bit costs are widened to fp32; nothing is copied to the host."""
    who = "hungarian_assign"
    if not isinstance(cost, torch.Tensor):
        raise TypeError(f"{who}: cost must be a tensor, got {type(cost).__name__}")
    if cost.dtype == torch.float64:
        raise RuntimeError(f"{who}: cost is float64, which is not supported (float32, float16 or bfloat16)")
    c = _float_input(who, "cost", cost)
    if c.dim() != 3:
        raise RuntimeError(f"{who}: cost must be (B, Q, T), got {tuple(c.shape)}")
    sizes = [int(n) for n in sizes]
    if any(n < 0 for n in sizes) or not sizes:
        raise RuntimeError(f"{who}: sizes must be a non-empty list of target counts >= 0, got {sizes}")
    if c.shape[1] > ASSIGN_MAX_SIDE or max(sizes) > ASSIGN_MAX_SIDE:
        raise RuntimeError(f"{who}: Q = {c.shape[1]} or an image's target count is above {ASSIGN_MAX_SIDE}, the most the solver takes a side")
    pairs, status = assign_launch([c], sizes)
    Q = c.shape[1]
    return _split_pairs(pairs[0], [min(Q, n) for n in sizes]), status[0]


class HungarianMatcher(nn.Module):
    """The reference's matcher: a 1-to-1 assignment between predictions and targets that minimises
    cost_bbox * L1 + cost_class * focal + cost_giou * (-GIoU).  The (B * Q, T) cost matrix comes from one kernel that evaluates the sigmoid and both focal
    terms only at the gathered target classes; it goes to the host in one copy, where scipy (imported on first use) solves each image's block.
    ``solver="device"`` solves the blocks with ``hungarian_assign`` instead: nothing goes to the host, the indices are device tensors, and the solver's
    status stays on the device in ``last_status`` until ``check_status()`` is asked for it."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha=0.25, solver: str = "scipy"):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.focal_alpha = focal_alpha
        if solver not in ("scipy", "device"):
            raise ValueError(f"HungarianMatcher: solver must be 'scipy' or 'device', got {solver!r}")
        self.solver = solver
        self.last_status = None

    @torch.no_grad()
    def assign_sets(self, output_sets, targets):
        """The device solver on several output sets at once (one launch per 16): [[(src, tgt)] per image] per set, device tensors."""
        sizes = [len(v["boxes"]) for v in targets]
        costs = [self.cost_matrix(o, targets).to(torch.float32) for o in output_sets]      # the dtype round trip the scipy path sees
        groups = {}                                        # the sets of one launch share min(Q, n_b): one group per Q
        for s, c in enumerate(costs):
            groups.setdefault(c.shape[1], []).append(s)
        pairs, rows = [None] * len(costs), [None] * len(costs)
        for members in groups.values():
            got, status = assign_launch([costs[s] for s in members], sizes)
            for k, s in enumerate(members):
                pairs[s], rows[s] = got[k], status[k]
        self.last_status = torch.stack(rows)
        return [_split_pairs(p, [min(c.shape[1], n) for n in sizes]) for p, c in zip(pairs, costs)], pairs

    def check_status(self):
        """Synchronises, reads ``last_status`` and raises what scipy raises for a cost matrix with non-finite entries (the device solver refuses +inf
        entries too, which scipy reports only when they make the problem infeasible)."""
        if self.last_status is None:
            return
        st = self.last_status.cpu()
        if bool((st == 1).any()):
            where = [tuple(x) for x in (st == 1).nonzero().tolist()]
            raise ValueError(f"matrix contains invalid numeric entries, or: cost matrix is infeasible (a non-finite cost in (set, image) {where})")
        if bool((st != 0).any()):
            raise RuntimeError(f"hungarian_assign: the solver gave status {sorted(set(st.flatten().tolist()) - {0})} (2: a trip bound, 3: inconsistent offsets)")

    @torch.no_grad()
    def cost_matrix(self, outputs, targets):
        """The reference's ``C`` before ``.cpu()``: (B, Q, T) on the device, T = all targets of the batch concatenated."""
        who = "HungarianMatcher"
        bs, num_queries = outputs["pred_logits"].shape[:2]
        dt = outputs["pred_logits"].dtype
        logits = _float_input(who, "pred_logits", outputs["pred_logits"]).flatten(0, 1)
        pred = _float_input(who, "pred_boxes", outputs["pred_boxes"]).flatten(0, 1)
        tgt_ids = torch.cat([v["labels"] for v in targets])
        tgt_bbox = torch.cat([v["boxes"] for v in targets])
        if not tgt_ids.is_cuda:
            raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); the target labels are cpu tensors and there is no CPU fallback")
        tgt_ids = tgt_ids.to(torch.int64).contiguous()
        tgt = _float_input(who, "target boxes", tgt_bbox)
        R, C, T = logits.shape[0], logits.shape[1], tgt.shape[0]
        cost = torch.empty(R, T, dtype=torch.float32, device=logits.device)
        with torch.cuda.device(logits.device):
            _lib.check(_lib.lib().fvit_det_matcher_cost(logits.data_ptr(), pred.data_ptr(), tgt_ids.data_ptr(), tgt.data_ptr(), cost.data_ptr(), R, C, T,
                                                        float(self.cost_class), float(self.cost_bbox), float(self.cost_giou), float(self.focal_alpha),
                                                        _lib.stream_ptr()), "fvit_det_matcher_cost")
        if dt != torch.float32:
            cost = cost.to(dt)
        return cost.view(bs, num_queries, T)

    @torch.no_grad()
    def forward(self, outputs, targets):
        if self.solver == "device":
            return self.assign_sets([outputs], targets)[0][0]
        C = self.cost_matrix(outputs, targets).cpu()      # the single copy to the host
        from scipy.optimize import linear_sum_assignment
        sizes = [len(v["boxes"]) for v in targets]
        indices = [linear_sum_assignment(c[i]) for i, c in enumerate(C.split(sizes, -1))]
        return [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices]
