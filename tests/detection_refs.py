"""References, case tables and bars for the detection post-processing kernels (csrc/fvit_boxes.hip, fastervit_amd/detection_ops.py).

Every operation is restated here in plain torch with a ``dtype`` argument: ``torch.float64`` on the fp32 inputs is ``exact``, ``torch.float32`` is
``plain32`` (an ordinary fp32 evaluation, whose own error sets the bar).  Values (scores, IoU, GIoU, cost) are held to ``bound`` / ``worst_ratio`` of
tests/backward_primitive_refs.py with fp32 output; indices, labels, keeps, counts and fp32 boxes to ``torch.equal``.

The select, pairwise and cost restatements are checked against the reference's own ``PostProcess``, ``util/box_ops.py`` and ``HungarianMatcher``
through tests/golden/detection_cases.npz (tests/golden/make_detection_golden.py).  NMS HAS NO REFERENCE PROGRAM here (torchvision is not installed):
its yardstick is ``nms_rule`` below, torchvision's published rule written out -- box order[j] is kept iff no earlier kept box i has
inter / (area_i + area_j - inter) > thr, inter = max(0, min x2 - max x1) * max(0, min y2 - max y1), no epsilon, no +1 pixel, 0 / 0 = NaN compares false.

The keyword switches of the restatements (``ge``, ``plus1``, ``chain``, ``ignore_idxs``, ``ties_high``, ``swap_hw``, ``gamma``, ``eps_*``) produce the
wrong answers tests/test_detection_refs_cpu.py shows to fail.
"""
import os

import numpy as np
import torch

from tests.backward_primitive_refs import bound, worst_ratio  # noqa: F401

F64, F32 = torch.float64, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection_cases.npz")

# ---------------------------------------------------------------------------------------------------------------------------------------- case tables
SELECT_CASES = [(1, 1, 1, 1), (2, 7, 5, 3), (2, 7, 5, 35), (1, 13, 79, 64), (2, 33, 31, 65), (1, 1025, 1, 1), (2, 900, 91, 300)]   # (B, Q, C, K)
SELECT_FLAG_CASE = 1                                                       # (2, 7, 5, 3) also runs with not_to_xyxy and with test
SELECT_RUNS = [(c, False, False) for c in range(len(SELECT_CASES))] + [(SELECT_FLAG_CASE, True, False), (SELECT_FLAG_CASE, False, True)]
NMS_N = [1, 2, 63, 64, 65, 130, 300]
NMS_G = [1, 3]
NMS_THR = 0.5
NMS_MARGIN = 1e-5          # no pair of a value case has |IoU64 - thr| <= this: ~30 x the ~6-rounding fp32 error of the quotient
PAIR_CASES = [(1, 1), (5, 3), (65, 67)]                                    # (N, M)
COST_CASES = [(3, 2, 1), (14, 5, 6), (130, 91, 9)]                         # (R, C, T)
COST_WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=0.25)
PP_NMS_CASE, PP_NMS_THR = 4, 0.5                                           # PostProcess with NMS on: SELECT_CASES[4]


def run_name(case, raw, test):
    return f"sel{case}" + ("_raw" if raw else "") + ("_test" if test else "")


def load_golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


# ------------------------------------------------------------------------------------------------------------------------------------- box arithmetic
def cxcywh_to_xyxy(x):
    xc, yc, w, h = x.unbind(-1)
    return torch.stack([xc - 0.5 * w, yc - 0.5 * h, xc + 0.5 * w, yc + 0.5 * h], dim=-1)


def box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def pair_iou(b1, b2, dtype, eps_iou=1e-6, eps_union=0.0):
    b1, b2 = b1.to(dtype), b2.to(dtype)
    lt = torch.max(b1[:, None, :2], b2[:, :2])
    rb = torch.min(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = box_area(b1)[:, None] + box_area(b2) - inter + eps_union
    return inter / (union + eps_iou), union


def pair_giou(b1, b2, dtype, eps_iou=1e-6, eps_area=1e-6):
    b1, b2 = b1.to(dtype), b2.to(dtype)
    iou, union = pair_iou(b1, b2, dtype, eps_iou)
    lt = torch.min(b1[:, None, :2], b2[:, :2])
    rb = torch.max(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    area = wh[:, :, 0] * wh[:, :, 1]
    return iou - (area - union) / (area + eps_area)


def _rand_cxcywh(g, n, lo=0.05, hi=0.4):
    c = 0.2 + 0.6 * torch.rand(n, 2, generator=g)
    wh = lo + (hi - lo) * torch.rand(n, 2, generator=g)
    return torch.cat([c, wh], 1).to(F32)


def pair_inputs(case):
    N, M = PAIR_CASES[case]
    g = torch.Generator().manual_seed(4100 + case)
    return cxcywh_to_xyxy(_rand_cxcywh(g, N)), cxcywh_to_xyxy(_rand_cxcywh(g, M))


# ---------------------------------------------------------------------------------------------------------------------------------- select + decode
def select(logits, boxes, sizes, K, dtype, not_to_xyxy=False, test=False, ties_high=False, swap_hw=False):
    """PostProcess without NMS on the logits: descending, ties to the lower flat index, NaN first.  Returns scores, labels, query, boxes."""
    B, Q, C = logits.shape
    flat = logits.reshape(B, Q * C)
    if ties_high:
        idx = (Q * C - 1) - torch.sort(flat.flip(1), dim=1, descending=True, stable=True).indices[:, :K]
    else:
        idx = torch.sort(flat, dim=1, descending=True, stable=True).indices[:, :K]
    scores = torch.gather(flat.to(dtype), 1, idx).sigmoid()
    labels, query = idx % C, idx // C
    bx = boxes.to(dtype)
    if not not_to_xyxy:
        bx = cxcywh_to_xyxy(bx)
        if test:
            bx = torch.cat([bx[..., :2], bx[..., 2:] - bx[..., :2]], -1)
    bx = torch.gather(bx, 1, query.unsqueeze(-1).repeat(1, 1, 4))
    h, w = sizes.to(dtype).unbind(1)
    if swap_hw:
        h, w = w, h
    return scores, labels, query, bx * torch.stack([w, h, w, h], dim=1)[:, None, :]


def select_condition(logits, K):
    """The fp32 CPU sigmoids of the top K + 1 candidates of every image are pairwise distinct: the reference's topk over probabilities has one answer."""
    B = logits.shape[0]
    p = logits.to(F32).sigmoid().reshape(B, -1)
    top = torch.sort(p, dim=1, descending=True).values[:, :K + 1]
    return bool((top[:, 1:] != top[:, :-1]).all()) if top.shape[1] > 1 else True


_SIZES = torch.tensor([[480.0, 640.0], [600.0, 433.0]], dtype=F32)


def select_inputs(case):
    B, Q, C, K = SELECT_CASES[case]
    for attempt in range(64):
        g = torch.Generator().manual_seed(1000 * (case + 1) + attempt)
        logits = (torch.randn(B, Q, C, generator=g) - 2.0).to(F32)      # mostly negative, as a detector's are: the top sigmoids are well apart
        if select_condition(logits, K):
            break
    else:
        raise AssertionError(f"select case {case}: no seed gives distinct top sigmoids")
    boxes = _rand_cxcywh(g, B * Q).view(B, Q, 4)
    return logits, boxes, _SIZES[:B].clone(), K


def select_exact_inputs(name):
    """Tie and special-value cases: (logits, boxes, sizes, K); the answer is torch.sort(stable=True, descending=True)'s."""
    g = torch.Generator().manual_seed(77)
    if name == "four_values":
        B, Q, C, K = 2, 33, 31, 65
        logits = torch.tensor([-1.5, 0.0, 0.25, 2.0])[torch.randint(0, 4, (B, Q, C), generator=g)]
    elif name == "all_equal_small":
        B, Q, C, K = 2, 7, 5, 35
        logits = torch.full((B, Q, C), 0.75)
    elif name == "all_equal_large":
        B, Q, C, K = 2, 900, 91, 300
        logits = torch.full((B, Q, C), -0.5)
    elif name == "specials":
        B, Q, C, K = 2, 7, 5, 35
        logits = torch.randn(B, Q, C, generator=g)
        logits[0, 1, 2] = float("nan"); logits[0, 5, 0] = float("nan"); logits[0, 3, 3] = float("inf"); logits[0, 0, 0] = float("-inf")
        logits[1, 6, 4] = float("inf"); logits[1, 2, 1] = float("inf"); logits[1, 4, 4] = -0.0; logits[1, 0, 3] = 0.0
    else:
        raise KeyError(name)
    return logits.to(F32), _rand_cxcywh(g, B * Q).view(B, Q, 4), _SIZES[:B].clone(), K


SELECT_EXACT = ["four_values", "all_equal_small", "all_equal_large", "specials"]


# ------------------------------------------------------------------------------------------------------------------------------------------------ NMS
def nms_rule(boxes, order, thr, dtype, idxs=None, ge=False, plus1=False, chain=False, ignore_idxs=False):
    """torchvision's rule on one group, written out.  boxes (N, 4) xyxy, order (N,) int64 by descending score -> kept original indices in that order."""
    b = boxes.to(dtype)
    off = 1.0 if plus1 else 0.0
    area = (b[:, 2] - b[:, 0] + off) * (b[:, 3] - b[:, 1] + off)
    N = b.shape[0]
    gone = torch.zeros(N, dtype=torch.bool)
    keep = []
    t = torch.tensor(thr, dtype=F32).to(dtype)      # the threshold a C float argument carries
    for a in range(N):
        i = int(order[a])
        if not gone[i]:
            keep.append(i)
        elif not chain:
            continue
        rest = order[a + 1:]
        if rest.numel() == 0:
            continue
        w = (torch.min(b[i, 2], b[rest, 2]) - torch.max(b[i, 0], b[rest, 0]) + off).clamp(min=0)
        h = (torch.min(b[i, 3], b[rest, 3]) - torch.max(b[i, 1], b[rest, 1]) + off).clamp(min=0)
        inter = w * h
        iou = inter / (area[i] + area[rest] - inter)
        hit = (iou >= t) if ge else (iou > t)
        if idxs is not None and not ignore_idxs:
            hit &= idxs[rest] == idxs[i]
        gone[rest[hit]] = True
    return torch.tensor(keep, dtype=torch.int64)


def nms_groups(boxes, order, thr, dtype, idxs=None, **kw):
    """(G, N, 4) -> keep (G, N) padded with -1 and count (G,) int32, the kernel's outputs."""
    G, N = boxes.shape[:2]
    keep = torch.full((G, N), -1, dtype=torch.int64)
    count = torch.zeros(G, dtype=torch.int32)
    for g in range(G):
        o = order[g] if order is not None else torch.arange(N)
        k = nms_rule(boxes[g], o, thr, dtype, None if idxs is None else idxs[g], **kw)
        keep[g, :k.numel()] = k
        count[g] = k.numel()
    return keep, count


def nms_condition(boxes, thr, margin=NMS_MARGIN):
    """No pair of a group has |IoU64 - thr| <= margin (IoU without epsilon)."""
    for b in boxes:
        iou, _ = pair_iou(b, b, F64, eps_iou=0.0)
        iou = iou[torch.isfinite(iou)]
        if ((iou - thr).abs() <= margin).any():
            return False
    return True


def nms_inputs(N, G, with_idxs, with_order):
    """Crowded boxes (pixels): many overlaps around the threshold.  with_order: random scores and their stable descending order; else the boxes are
    already in score order and order is None."""
    for attempt in range(200):
        g = torch.Generator().manual_seed(7000 + 131 * N + 17 * G + 2 * int(with_idxs) + int(with_order) + 100000 * attempt)
        c = 100.0 * torch.rand(G, N, 2, generator=g)
        wh = 20.0 + 40.0 * torch.rand(G, N, 2, generator=g)
        boxes = torch.cat([c - 0.5 * wh, c + 0.5 * wh], -1).to(F32)
        if nms_condition(boxes, NMS_THR):
            break
    else:
        raise AssertionError(f"nms case N={N} G={G}: no seed keeps every IoU away from the threshold")
    idxs = torch.randint(0, 3, (G, N), generator=g) if with_idxs else None
    order = scores = None
    if with_order:
        scores = torch.rand(G, N, generator=g)
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    return boxes, order, idxs, scores


def nms_exact_inputs(name):
    """(boxes (N, 4), expected keep list, thr) in identity order."""
    far = lambda n, x0=1000.0: torch.tensor([[x0 + 20.0 * k, 0.0, x0 + 20.0 * k + 10.0, 10.0] for k in range(n)])      # pairwise disjoint
    if name == "iou_exactly_thr":          # inter 1, union 2: IoU = 0.5 is not > 0.5
        return torch.tensor([[0.0, 0.0, 2.0, 1.0], [0.0, 0.0, 1.0, 1.0]]), [0, 1], 0.5
    if name == "identical":
        return torch.tensor([[3.0, 4.0, 9.0, 11.0]] * 5), [0], 0.5
    if name == "disjoint":
        return far(70), list(range(70)), 0.5
    if name == "chain":                    # A (0) suppresses B (70), so B cannot suppress C (135): three different 64-blocks
        b = far(140)
        b[0] = torch.tensor([0.0, 0.0, 10.0, 10.0]); b[70] = torch.tensor([0.0, 3.0, 10.0, 13.0]); b[135] = torch.tensor([0.0, 6.0, 10.0, 16.0])
        return b, [i for i in range(140) if i != 70], 0.5
    if name == "degenerate":               # zero-area boxes: 0 / 0 = NaN and 0 / area = 0 suppress nothing
        return torch.tensor([[5.0, 5.0, 5.0, 5.0], [5.0, 5.0, 5.0, 5.0], [0.0, 0.0, 10.0, 10.0], [5.0, 5.0, 5.0, 5.0]]), [0, 1, 2, 3], 0.5
    raise KeyError(name)


NMS_EXACT = ["iou_exactly_thr", "identical", "disjoint", "chain", "degenerate"]


# --------------------------------------------------------------------------------------------------------------------------------- the matcher's cost
def matcher_cost(logits, pred, ids, tgt, dtype, cost_class, cost_bbox, cost_giou, focal_alpha, gamma=2.0):
    """HungarianMatcher.forward's C before .view: (R, T)."""
    p = logits.to(dtype).sigmoid()
    pred, tgt = pred.to(dtype), tgt.to(dtype)
    neg = (1 - focal_alpha) * (p ** gamma) * (-(1 - p + 1e-8).log())
    pos = focal_alpha * ((1 - p) ** gamma) * (-(p + 1e-8).log())
    c_class = pos[:, ids] - neg[:, ids]
    c_bbox = torch.cdist(pred, tgt, p=1)
    c_giou = -pair_giou(cxcywh_to_xyxy(pred), cxcywh_to_xyxy(tgt), dtype)
    return cost_bbox * c_bbox + cost_class * c_class + cost_giou * c_giou


def cost_inputs(case):
    R, C, T = COST_CASES[case]
    g = torch.Generator().manual_seed(5200 + case)
    logits = (1.5 * torch.randn(R, C, generator=g) - 1.0).to(F32)
    ids = torch.randint(0, C, (T,), generator=g)
    return logits, _rand_cxcywh(g, R), ids, _rand_cxcywh(g, T)
