"""References, case tables and bars for the training criterion (csrc/fvit_loss.hip, fastervit_amd/criterion.py).

The reference's ``sigmoid_focal_loss`` and ``SetCriterion`` are restated here in plain torch with a ``dtype`` argument: ``torch.float64`` on the fp32 inputs
is ``exact`` (its gradients come from autograd), ``torch.float32`` is ``plain32``, an ordinary fp32 evaluation whose own error sets the bars.  The
restatement returns every loss as its UNREDUCED terms, already scaled, so that the value is ``terms.sum()``:

  elementwise results (gradients)   ``bound`` / ``worst_ratio`` of tests/backward_primitive_refs.py, fp32 output
  scalar sums                       ``scalar_bar`` = 8 * sum_i |plain32_i - exact_i| + 48 * 2^-24 * sum_i |exact_i| over the unreduced terms: 8 x the fp32
                                    error of the terms, plus a chain of 48 fp32 additions (roundings) through which a term may pass -- the kernels' longest
                                    is 31 per lane + 6 in the wave + 2 across the waves + 6 over the partials + the scale = 46
  class_error, cardinality_error    ``COUNT_RTOL``: they are fp32 arithmetic on exact integer counts (a division and a subtraction, or a mean over B)
  counts, hits, indices             torch.equal

The restatement is checked against the reference's own programs through tests/golden/criterion_cases.npz (tests/golden/make_criterion_golden.py).  Its
keyword switches (``swap_alpha``, ``gamma``, ``eps_iou``, ``eps_area``, ``swap_halves``, ``no_q``, ``no_num_boxes``, ``dn_plain_num_boxes``,
``card_class0``, ``noobj_last``) produce the wrong answers tests/test_criterion_refs_cpu.py shows to fail.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.backward_primitive_refs import bound, worst_ratio  # noqa: F401
from tests import detection_refs as D

F64, F32 = torch.float64, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_cases.npz")

FOCAL_ALPHA = 0.25
MATCH_WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=FOCAL_ALPHA)
LOSSES = ["labels", "boxes", "cardinality"]
BASE_WEIGHTS = dict(loss_ce=1.0, loss_bbox=5.0, loss_giou=2.0)
CHAIN = 48
COUNT_RTOL = 2.0 ** -21      # four fp32 roundings of arithmetic on exact counts

# ---------------------------------------------------------------------------------------------------------------------------------------- case tables
LABEL_CASES = [(1, 1, 1), (2, 7, 5), (2, 33, 31), (1, 65, 91), (3, 130, 3), (2, 900, 91)]            # (B, Q, C)
LABEL_COUNTS = [[1], [3, 0], [5, 9], [20], [0, 7, 40], [20, 20]]                                    # targets per image: 0 is among them
LABEL_EMPTY_CASE = 1                                                                                 # also runs with no target at all
LABEL_SET_COUNTS = [1, 3, 16]                                                                        # n_sets per launch
BOX_M = [0, 1, 3, 64, 65, 300]
BOX_SMALL_M = 65                                                                                     # one more box case, of small boxes (box_inputs)
# SetCriterion.forward: B, Q, C, targets per image, aux layers, interm, denoising (groups, single_pad) or None
FORWARD_CASES = [
    dict(name="main", B=2, Q=7, C=5, nt=[2, 0], aux=0, interm=False, dn=None),
    dict(name="aux_interm", B=2, Q=33, C=31, nt=[3, 5], aux=2, interm=True, dn=None),
    dict(name="dn", B=2, Q=33, C=31, nt=[4, 0], aux=2, interm=True, dn=(3, 8)),
    dict(name="empty", B=2, Q=7, C=5, nt=[0, 0], aux=1, interm=False, dn=None),
    dict(name="sets17", B=2, Q=7, C=5, nt=[2, 3], aux=16, interm=False, dn=None),
]
TIE_GAP = 1e-4


def load_golden():
    """Arrays as tensors; the ``*_keys`` arrays (the reference's key sets) as sorted lists of str."""
    return {k: ([str(x) for x in v] if v.dtype.kind == "U" else torch.from_numpy(v)) for k, v in np.load(GOLDEN).items()}


def weight_dict(n_aux, interm):
    w = {}
    for sfx in [""] + [f"_{i}" for i in range(n_aux)] + (["_interm"] if interm else []):
        w.update({k + sfx: v for k, v in BASE_WEIGHTS.items()})
    for sfx in ["_dn"] + [f"_dn_{i}" for i in range(n_aux)]:
        w.update({k + sfx: v for k, v in BASE_WEIGHTS.items()})
    return w


# -------------------------------------------------------------------------------------------------------------------------------------------- bars
def scalar_bar(exact_terms, plain_terms):
    e, p = exact_terms.detach().to(F64), plain_terms.detach().to(F64)
    return 8.0 * (p - e).abs().sum().item() + CHAIN * 2.0 ** -24 * e.abs().sum().item()


def scalar_ratio(got, exact_terms, plain_terms):
    """|got - sum(exact)| / scalar_bar; a zero bar is met by the exact value only; inf for a non-finite ``got``."""
    got = float(got)
    if not np.isfinite(got):
        return float("inf")
    err, bar = abs(got - exact_terms.detach().to(F64).sum().item()), scalar_bar(exact_terms, plain_terms)
    return 0.0 if err == 0 else (err / bar if bar > 0 else float("inf"))


# ---------------------------------------------------------------------------------------------------------------------------------------- label loss
def focal_terms(logits, targets01, dtype, alpha=FOCAL_ALPHA, gamma=2.0, swap_alpha=False):
    """The reference's sigmoid_focal_loss before ``.mean(1).sum() / num_boxes``."""
    x, t = logits.to(dtype), targets01.to(dtype)
    prob = x.sigmoid()
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = prob * t + (1 - prob) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        a = (1 - alpha, alpha) if swap_alpha else (alpha, 1 - alpha)
        loss = (a[0] * t + a[1] * (1 - t)) * loss
    return loss


def onehot(classes, C, dtype, noobj_last=False):
    """(R,) class ids in [0, C] -> (R, C) 0 / 1, the reference's scatter into C + 1 columns with the last one dropped."""
    cls = torch.where(classes == C, torch.full_like(classes, C - 1), classes) if noobj_last else classes
    t = torch.zeros(classes.shape[0], C + 1, dtype=dtype, device=classes.device)
    t.scatter_(1, cls.unsqueeze(-1), 1)
    return t[:, :C]


def label_ref(logits, classes, num_boxes, dtype, alpha=FOCAL_ALPHA, gamma=2.0, swap_alpha=False, noobj_last=False, no_q=False, no_num_boxes=False,
              card_class0=False, count_hits=True):
    """logits (B, Q, C), classes (B * Q,) -> terms (B * Q, C) with loss_ce = terms.sum(), card (B,) int32, hits (int; the reference counts them only
    where it logs class_error, and count_hits=False skips the two reads)."""
    B, Q, C = logits.shape
    x = logits.reshape(B * Q, C)
    terms = focal_terms(x, onehot(classes, C, dtype, noobj_last), dtype, alpha, gamma, swap_alpha)
    # loss.mean(1).sum() / num_boxes * Q: every term over Q, over num_boxes, times Q
    terms = terms / (1.0 if no_num_boxes else num_boxes)
    if no_q:
        terms = terms / Q
    arg = logits.argmax(-1)
    card = (arg != (0 if card_class0 else C - 1)).sum(1).to(torch.int32)
    if not count_hits:
        return dict(terms=terms, card=card)
    matched = classes < C
    hits = int((arg.reshape(-1)[matched] == classes[matched]).sum())
    return dict(terms=terms, card=card, hits=hits, matched=int(matched.sum()))


def unique_row_max(logits):
    top = torch.topk(logits, min(2, logits.shape[-1]), dim=-1).values
    return logits.shape[-1] == 1 or bool((top[..., 0] != top[..., 1]).all())


def _logits(g, shape):
    for _ in range(64):
        x = (1.5 * torch.randn(*shape, generator=g) - 1.0).to(F32)
        if unique_row_max(x):
            return x
    raise AssertionError("no draw with a unique maximum in every row")


def label_inputs(case, empty=False, seed=0):
    """(logits (B, Q, C), classes (B * Q,) int64 with C = no object, num_boxes): ``counts`` distinct rows of every image carry a class < C."""
    B, Q, C = LABEL_CASES[case]
    return label_draw(B, Q, C, [0] * B if empty else LABEL_COUNTS[case], 8100 + 10 * case + int(empty) + 1000 * seed)


def label_draw(B, Q, C, counts, seed):
    counts = [min(n, Q) for n in counts]
    g = torch.Generator().manual_seed(seed)
    logits = _logits(g, (B, Q, C))
    classes = torch.full((B * Q,), C, dtype=torch.int64)
    for b, n in enumerate(counts):
        rows = torch.randperm(Q, generator=g)[:n]
        classes[b * Q + rows] = torch.randint(0, C, (n,), generator=g)
    return logits, classes, float(max(sum(counts), 1))


# ------------------------------------------------------------------------------------------------------------------------------------------ box loss
def giou_pairs(s, t, eps_iou=1e-6, eps_area=1e-6):
    """GIoU of box i of ``s`` with box i of ``t`` (xyxy): the diagonal of the reference's generalized_box_iou."""
    a1, a2 = (s[:, 2] - s[:, 0]) * (s[:, 3] - s[:, 1]), (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    wh = (torch.min(s[:, 2:], t[:, 2:]) - torch.max(s[:, :2], t[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = a1 + a2 - inter
    iou = inter / (union + eps_iou)
    wh = (torch.max(s[:, 2:], t[:, 2:]) - torch.min(s[:, :2], t[:, :2])).clamp(min=0)
    area = wh[:, 0] * wh[:, 1]
    return iou - (area - union) / (area + eps_area)


def box_ref(src, tgt, num_boxes, dtype, eps_iou=1e-6, eps_area=1e-6, swap_halves=False, no_num_boxes=False):
    """src, tgt (M, 4) cxcywh -> the unreduced terms of loss_bbox (M, 4), loss_xy, loss_hw (M, 2) and loss_giou (M,)."""
    s, t = src.to(dtype), tgt.to(dtype)
    nb = 1.0 if no_num_boxes else num_boxes
    l1 = (s - t).abs() / nb
    giou = (1 - giou_pairs(D.cxcywh_to_xyxy(s), D.cxcywh_to_xyxy(t), eps_iou, eps_area)) / nb
    xy, hw = (l1[:, 2:], l1[:, :2]) if swap_halves else (l1[:, :2], l1[:, 2:])
    return dict(loss_bbox=l1, loss_giou=giou, loss_xy=xy.detach(), loss_hw=hw.detach())


def no_ties(src, tgt, gap=TIE_GAP):
    """No coordinate of a pair ties: the L1 sign, the max / min of the corners and the clamps of the overlap all have one subgradient."""
    if src.shape[0] == 0:
        return True
    s, t = src.to(F64), tgt.to(F64)
    a, b = D.cxcywh_to_xyxy(s), D.cxcywh_to_xyxy(t)
    overlap = torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])
    return bool(((s - t).abs() > gap).all() and ((a - b).abs() > gap).all() and (overlap.abs() > gap).all())


def box_inputs(M, seed=0, small=False):
    """small: boxes of 1 .. 3 % of the image next to their targets, where the 1e-6 of the two quotients is 1e-3 of the area and cannot be dropped unseen."""
    for attempt in range(200):
        g = torch.Generator().manual_seed(8700 + 7 * M + 100000 * attempt + 1000 * seed + 500 * int(small))
        if small:
            src = D._rand_cxcywh(g, M, 0.01, 0.03)
            tgt = torch.cat([src[:, :2] + 0.01 * (torch.rand(M, 2, generator=g) - 0.5), D._rand_cxcywh(g, M, 0.01, 0.03)[:, 2:]], 1).to(F32)
        else:
            src, tgt = D._rand_cxcywh(g, M), D._rand_cxcywh(g, M)
        if no_ties(src, tgt, 1e-5 if small else TIE_GAP):
            return src, tgt
    raise AssertionError(f"box case M={M}: no seed without a coordinate tie")


# ------------------------------------------------------------------------------------------------------------------------------- the whole criterion
def pred_sets(outputs):
    """[(name, dict)] of every prediction set of an outputs dict, in the order gradients are recorded."""
    sets = [("main", outputs)]
    sets += [(f"aux{i}", o) for i, o in enumerate(outputs.get("aux_outputs", []))]
    if "interm_outputs" in outputs:
        sets.append(("interm", outputs["interm_outputs"]))
    dn = outputs.get("dn_meta") or {}
    if "output_known_lbs_bboxes" in dn:
        known = dn["output_known_lbs_bboxes"]
        sets.append(("dn", known))
        sets += [(f"dn_aux{i}", o) for i, o in enumerate(known.get("aux_outputs", []))]
    return sets


def convert(outputs, fn):
    """A copy of the outputs dict with ``fn`` applied to every pred_logits / pred_boxes."""
    def one(o):
        return {"pred_logits": fn(o["pred_logits"]), "pred_boxes": fn(o["pred_boxes"])}
    out = one(outputs)
    if "aux_outputs" in outputs:
        out["aux_outputs"] = [one(o) for o in outputs["aux_outputs"]]
    if "interm_outputs" in outputs:
        out["interm_outputs"] = one(outputs["interm_outputs"])
    dn = outputs.get("dn_meta")
    out["dn_meta"] = dn
    if dn and "output_known_lbs_bboxes" in dn:
        known = one(dn["output_known_lbs_bboxes"])
        known["aux_outputs"] = [one(o) for o in dn["output_known_lbs_bboxes"].get("aux_outputs", [])]
        out["dn_meta"] = dict(dn, output_known_lbs_bboxes=known)
    return out


def convert_targets(targets, fn):
    return [{"labels": t["labels"] if fn is None else fn(t["labels"]), "boxes": t["boxes"] if fn is None else fn(t["boxes"])} for t in targets]


def cost_matrices(o, targets, dtype):
    """The matcher's (Q, n_b) block of every image."""
    ids, tgt = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
    B, Q, C = o["pred_logits"].shape
    cost = D.matcher_cost(o["pred_logits"].detach().reshape(B * Q, C), o["pred_boxes"].detach().reshape(B * Q, 4), ids, tgt, dtype,
                          MATCH_WEIGHTS["cost_class"], MATCH_WEIGHTS["cost_bbox"], MATCH_WEIGHTS["cost_giou"], MATCH_WEIGHTS["focal_alpha"])
    sizes = [len(t["labels"]) for t in targets]
    return [c[i] for i, c in enumerate(cost.view(B, Q, -1).split(sizes, -1))]


def assign(blocks):
    from scipy.optimize import linear_sum_assignment
    out = []
    for c in blocks:
        i, j = linear_sum_assignment(c.cpu().numpy())      # on a device this is the reference's copy to the host, one per set
        out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
    return out


def match(o, targets, dtype=F64):
    return assign(cost_matrices(o, targets, dtype))


def matched_sets(outputs):
    return [outputs] + list(outputs.get("aux_outputs", [])) + ([outputs["interm_outputs"]] if "interm_outputs" in outputs else [])


def dn_indices(targets, groups, single_pad):
    out = []
    for t in targets:
        n = len(t["labels"])
        tt = torch.arange(n).unsqueeze(0).repeat(groups, 1)
        out.append((((torch.arange(groups) * single_pad).unsqueeze(1) + tt).flatten(), tt.flatten()))
    return out


def _set_terms(o, targets, indices, num_boxes, dtype, log, sw):
    """The unreduced terms of one output set: {key: terms}, and the count-derived scalars {key: 0-dim tensor}."""
    B, Q, C = o["pred_logits"].shape
    dev = o["pred_logits"].device
    classes = torch.full((B * Q,), C, dtype=torch.int64, device=dev)
    src_rows = torch.cat([b * Q + i for b, (i, _) in enumerate(indices)])
    classes[src_rows] = torch.cat([t["labels"][j] for t, (_, j) in zip(targets, indices)])
    lab = label_ref(o["pred_logits"], classes, num_boxes, dtype, count_hits=log, **{k: sw[k] for k in ("swap_alpha", "gamma", "noobj_last", "no_q",
                                                                                                        "no_num_boxes", "card_class0") if k in sw})
    terms, scalars = {"loss_ce": lab["terms"]}, {}
    if log:
        scalars["class_error"] = torch.tensor(100.0 - lab["hits"] * 100.0 / lab["matched"] if lab["matched"] else 100.0, dtype=dtype, device=dev)
    lengths = torch.tensor([len(t["labels"]) for t in targets], dtype=dtype, device=dev)
    scalars["cardinality_error"] = (lab["card"].to(dtype) - lengths).abs().mean()
    src = o["pred_boxes"].reshape(B * Q, 4)[src_rows]
    tgt = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, indices)])
    terms.update(box_ref(src, tgt, num_boxes, dtype, **{k: sw[k] for k in ("eps_iou", "eps_area", "swap_halves", "no_num_boxes") if k in sw}))
    return terms, scalars


def criterion(outputs, targets, indices, dtype, training=True, **sw):
    """The reference's SetCriterion.forward with losses = labels, boxes, cardinality, given the matcher's ``indices`` of the matched sets (main, aux ..,
    interm).  ``outputs`` already holds tensors of ``dtype`` (leaves that require grad for ``exact`` gradients).  Returns ({key: unreduced terms},
    {key: scalar}); the value of a loss is ``terms[key].sum()``, and the reference's zero-valued keys have empty terms."""
    num_boxes = float(max(sum(len(t["labels"]) for t in targets), 1))
    tg = convert_targets(targets, lambda v: v.to(dtype) if v.is_floating_point() else v)
    terms, scalars = {}, {}

    def add(sfx, pair):
        terms.update({k + sfx: v for k, v in pair[0].items()})
        scalars.update({k + sfx: v for k, v in pair[1].items()})

    n_aux = len(outputs.get("aux_outputs", []))
    dn = outputs.get("dn_meta")
    use_dn = bool(training and dn and "output_known_lbs_bboxes" in dn)
    zero_keys = ("loss_bbox_dn", "loss_giou_dn", "loss_ce_dn", "loss_xy_dn", "loss_hw_dn", "cardinality_error_dn")
    if use_dn:
        groups, single_pad = dn["num_dn_group"], dn["pad_size"] // dn["num_dn_group"]
        known, dn_idx = dn["output_known_lbs_bboxes"], dn_indices(targets, groups, single_pad)
        dn_boxes = num_boxes if sw.get("dn_plain_num_boxes") else num_boxes * groups
        add("_dn", _set_terms(known, tg, dn_idx, dn_boxes, dtype, False, sw))
    else:
        terms.update({k: torch.zeros(0, dtype=dtype) for k in zero_keys})
    add("", _set_terms(outputs, tg, indices[0], num_boxes, dtype, True, sw))
    for i in range(n_aux):
        add(f"_{i}", _set_terms(outputs["aux_outputs"][i], tg, indices[1 + i], num_boxes, dtype, False, sw))
        if use_dn:
            add(f"_dn_{i}", _set_terms(known["aux_outputs"][i], tg, dn_idx, dn_boxes, dtype, False, sw))
        else:
            terms.update({f"{k}_{i}": torch.zeros(0, dtype=dtype) for k in zero_keys})
    if "interm_outputs" in outputs:
        add("_interm", _set_terms(outputs["interm_outputs"], tg, indices[1 + n_aux], num_boxes, dtype, False, sw))
    return terms, scalars


def total(terms, weights):
    return sum(terms[k].sum() * w for k, w in weights.items() if k in terms and terms[k].requires_grad)


def forward_condition(outputs, targets, indices):
    """What makes the reference's answer unique: a unique maximum in every row of every set, no coordinate tie in any matched pair."""
    for _, o in pred_sets(outputs):
        if not unique_row_max(o["pred_logits"]):
            return False
    pairs = list(zip(matched_sets(outputs), indices))
    dn = outputs.get("dn_meta")
    if dn and "output_known_lbs_bboxes" in dn:
        idx = dn_indices(targets, dn["num_dn_group"], dn["pad_size"] // dn["num_dn_group"])
        known = dn["output_known_lbs_bboxes"]
        pairs += [(o, idx) for o in [known] + list(known.get("aux_outputs", []))]
    for o, ind in pairs:
        src = torch.cat([o["pred_boxes"][b][i] for b, (i, _) in enumerate(ind)])
        tgt = torch.cat([t["boxes"][j] for t, (_, j) in zip(targets, ind)])
        if not no_ties(src, tgt):
            return False
    return True


def forward_inputs(case):
    """(outputs, targets) of FORWARD_CASES[case] as fp32 CPU tensors, and the exact matcher's indices of the matched sets."""
    c = FORWARD_CASES[case]
    B, Q, C = c["B"], c["Q"], c["C"]
    for attempt in range(200):
        g = torch.Generator().manual_seed(9300 + 50 * case + 100000 * attempt)

        def one(q):
            return {"pred_logits": _logits(g, (B, q, C)), "pred_boxes": D._rand_cxcywh(g, B * q).view(B, q, 4)}
        outputs = one(Q)
        if c["aux"]:
            outputs["aux_outputs"] = [one(Q) for _ in range(c["aux"])]
        if c["interm"]:
            outputs["interm_outputs"] = one(Q)
        outputs["dn_meta"] = None
        if c["dn"]:
            groups, single_pad = c["dn"]
            known = one(groups * single_pad)
            known["aux_outputs"] = [one(groups * single_pad) for _ in range(c["aux"])]
            outputs["dn_meta"] = {"output_known_lbs_bboxes": known, "num_dn_group": groups, "pad_size": groups * single_pad}
        targets = [{"labels": torch.randint(0, C, (n,), generator=g), "boxes": D._rand_cxcywh(g, n)} for n in c["nt"]]
        indices = [match(o, targets) for o in matched_sets(outputs)]
        if forward_condition(outputs, targets, indices):
            return outputs, targets, indices
    raise AssertionError(f"forward case {c['name']}: no seed meets the uniqueness conditions")


def checksum(outputs, targets):
    return np.array([sum(o["pred_logits"].double().sum().item() for _, o in pred_sets(outputs)),
                     sum(o["pred_boxes"].double().sum().item() for _, o in pred_sets(outputs)) + sum(t["boxes"].double().sum().item() for t in targets)])
