"""The DINO training criterion on the gfx950 kernels of csrc/fvit_loss.hip -- DESIGN.md section 16.

Drop-ins, by signature, key set and value, for the reference's ``models/dino/utils.py`` (``sigmoid_focal_loss``) and ``models/dino/dino.py``
(``SetCriterion``):

    sigmoid_focal_loss(inputs, targets, num_boxes, alpha=0.25, gamma=2)     dense 0 / 1 float targets, differentiable in inputs
    SetCriterion(num_classes, matcher, weight_dict, focal_alpha, losses)    forward(outputs, targets, return_indices=False), loss_labels, loss_boxes,
                                                                            loss_cardinality, get_loss

``SetCriterion.forward`` collects every output set of the step (main, aux, interm, enc and the denoising sets) first and then runs all label losses in
ceil(sets / 16) calls of the label kernel and all box losses in as many of the box kernel, each call one ``autograd.Function``.  With this library's
``HungarianMatcher`` (anything that has ``cost_matrix``) all sets are matched behind ONE device -> host copy of the concatenated cost matrices; any other
matcher is called per set, as the reference does.  With ``HungarianMatcher(solver="device")`` the assignment is solved on the device (DESIGN.md section
17): ``forward`` then copies nothing to the host and never waits for the device, and ``return_indices`` gives device tensors.  The one-hot target
tensor is never built: the kernel takes a per-row class map, which is formed for all sets at once from one host -> device copy of the matched indices
(of the offsets the solver's indices are added to, on the device path).  The denoising indices are host tensors.

16-bit inputs are widened to fp32 once and gradients come back in the input dtype; float64 is refused by name; a CPU tensor raises (there is no CPU or
eager fallback).  ``'masks'`` raises NotImplementedError: segmentation is not part of this library.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _lib

__all__ = ["sigmoid_focal_loss", "SetCriterion"]

_FLOATS = (torch.float32, torch.float16, torch.bfloat16)
MAX_SETS = _lib.FVIT_DET_MAX_SETS


def _check_float(who, name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype == torch.float64:
        raise RuntimeError(f"{who}: {name} is float64, which is not supported (float32, float16 or bfloat16)")
    if not t.is_cuda:
        raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); {name} is a {t.device.type} tensor and there is no CPU fallback")
    if t.dtype not in _FLOATS:
        raise RuntimeError(f"{who}: {name} has dtype {t.dtype}; float32, float16 or bfloat16 is expected")


def _dense32(t, align=4):
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % align else t


class _LabelMeta:
    """What one label launch needs besides the logits: per set the class map (int32 [R]) or dense targets ([R][C] fp32), (B, Q) and the scale."""

    def __init__(self, C, alpha, gamma, classes, targets, shapes, scales):
        self.C, self.alpha, self.gamma = int(C), float(alpha), float(gamma)
        self.classes, self.targets, self.shapes, self.scales = classes, targets, shapes, scales

    def table(self, logits, grads=None):
        sets = (_lib.FvitDetLabelSet * len(logits))()
        for s, lg in enumerate(logits):
            B, Q = self.shapes[s]
            sets[s] = _lib.FvitDetLabelSet(logits=lg.data_ptr(), classes=_lib.ptr(self.classes[s]), targets=_lib.ptr(self.targets[s]),
                                           grad_logits=_lib.ptr(grads[s]) if grads is not None else None, R=B * Q, Q=Q, B=B, scale=self.scales[s])
        return sets


class _LabelLoss(torch.autograd.Function):
    """One launch of the label kernel: (loss [n], cardinality [n][max B] int32, hits [n] int32) of n <= 16 sets; differentiable in the logits."""

    @staticmethod
    def forward(ctx, meta, *logits):
        lib = _lib.lib()
        n, dev = len(logits), logits[0].device
        wide = [_dense32(lg) for lg in logits]
        sets = meta.table(wide)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        stride = max(b for b, _ in meta.shapes)
        card = torch.empty(n, stride, dtype=torch.int32, device=dev)
        hits = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            need = int(lib.fvit_det_label_loss_workspace(sets, n, meta.C))
            if need == 0:
                _lib.check(-1, "fvit_det_label_loss_workspace")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(lib.fvit_det_label_loss(sets, n, meta.C, meta.alpha, meta.gamma, loss.data_ptr(), card.data_ptr(), stride, hits.data_ptr(),
                                               ws.data_ptr(), need, _lib.stream_ptr()), "fvit_det_label_loss")
        ctx.meta, ctx.dtypes, ctx.shapes = meta, [lg.dtype for lg in logits], [lg.shape for lg in logits]
        ctx.save_for_backward(*wide)
        ctx.mark_non_differentiable(card, hits)
        return loss, card, hits

    @staticmethod
    def backward(ctx, g_loss, _g_card, _g_hits):
        wide, meta = ctx.saved_tensors, ctx.meta
        n, dev = len(wide), wide[0].device
        g = _dense32(g_loss)
        flat = torch.empty(sum(w.numel() for w in wide), dtype=torch.float32, device=dev)      # the one (R, C) fp32 tensor per set
        grads = list(flat.split([w.numel() for w in wide]))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().fvit_det_label_loss_backward(meta.table(wide, grads), n, meta.C, meta.alpha, meta.gamma, g.data_ptr(), _lib.stream_ptr()),
                       "fvit_det_label_loss_backward")
        out = [gr.view(sh).to(dt) if need else None for gr, sh, dt, need in zip(grads, ctx.shapes, ctx.dtypes, ctx.needs_input_grad[1:])]
        return (None, *out)


class _BoxMeta:
    def __init__(self, tgts, scales):
        self.tgts, self.scales = tgts, scales      # per set: (M, 4) fp32 dense 16-byte aligned target boxes, the scale

    def table(self, srcs, grads=None):
        sets = (_lib.FvitDetBoxSet * len(srcs))()
        for s, src in enumerate(srcs):
            M = src.shape[0]
            sets[s] = _lib.FvitDetBoxSet(src=src.data_ptr() if M else None, tgt=self.tgts[s].data_ptr() if M else None,
                                         grad_src=grads[s].data_ptr() if grads is not None and M else None, M=M, scale=self.scales[s])
        return sets


class _BoxLoss(torch.autograd.Function):
    """One launch of the box kernel: out [n][4] = (loss_xy, loss_hw, loss_giou, loss_bbox) of n <= 16 sets; differentiable in the matched source boxes."""

    @staticmethod
    def forward(ctx, meta, *srcs):
        n, dev = len(srcs), srcs[0].device
        wide = [_dense32(s, 16) for s in srcs]
        total = sum(w.shape[0] for w in wide)
        out = torch.empty(n, 4, dtype=torch.float32, device=dev) if total else torch.zeros(n, 4, dtype=torch.float32, device=dev)
        if total:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().fvit_det_box_loss(meta.table(wide), n, out.data_ptr(), _lib.stream_ptr()), "fvit_det_box_loss")
        ctx.meta, ctx.dtypes = meta, [s.dtype for s in srcs]
        ctx.save_for_backward(*wide)
        return out

    @staticmethod
    def backward(ctx, g_out):
        wide, meta = ctx.saved_tensors, ctx.meta
        n, dev = len(wide), wide[0].device
        g = _dense32(g_out)
        rows = [w.shape[0] for w in wide]
        flat = torch.empty(sum(rows), 4, dtype=torch.float32, device=dev)
        grads = list(flat.split(rows))
        if sum(rows):
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().fvit_det_box_loss_backward(meta.table(wide, grads), n, g.data_ptr(), _lib.stream_ptr()), "fvit_det_box_loss_backward")
        return (None, *[gr.to(dt) if need else None for gr, dt, need in zip(grads, ctx.dtypes, ctx.needs_input_grad[1:])])


def sigmoid_focal_loss(inputs, targets, num_boxes, alpha: float = 0.25, gamma: float = 2):
    """The reference's focal loss (RetinaNet) on dense targets: ``loss.mean(1).sum() / num_boxes`` of alpha_t * BCE * (1 - p_t) ** gamma, differentiable in
    ``inputs``.  ``targets`` has the shape of ``inputs`` and holds only 0 and 1 (anything else is refused: one host read); alpha < 0 means no alpha
    weighting."""
    who = "sigmoid_focal_loss"
    _check_float(who, "inputs", inputs)
    _check_float(who, "targets", targets)
    if inputs.dim() < 2 or inputs.shape != targets.shape or inputs.numel() == 0:
        raise RuntimeError(f"{who}: inputs and targets must have the same non-empty shape with at least 2 dimensions, got {tuple(inputs.shape)} and "
                           f"{tuple(targets.shape)}")
    tg = _dense32(targets)
    if not bool(((tg == 0) | (tg == 1)).all()):
        raise RuntimeError(f"{who}: targets must hold only 0 and 1 (the kernel evaluates t = [target != 0]); soft targets are not supported")
    C = inputs.shape[-1]
    R = inputs.numel() // C
    meta = _LabelMeta(C, alpha, gamma, [None], [tg], [(1, R)], [1.0 / (float(inputs.shape[1]) * float(num_boxes))])
    return _LabelLoss.apply(meta, inputs)[0][0]


def _host_indices(indices):
    """[(src, tgt)] per image as int64 numpy arrays (the matcher's CPU tensors; a device tensor is copied)."""
    return [(np.asarray(torch.as_tensor(i).cpu(), dtype=np.int64).reshape(-1), np.asarray(torch.as_tensor(j).cpu(), dtype=np.int64).reshape(-1))
            for i, j in indices]


class _Job:
    """One output set of the step: its outputs dict, indices, num_boxes and the suffix of its keys."""

    def __init__(self, suffix, outputs, indices, num_boxes, log, pairs=None):
        self.suffix, self.outputs, self.indices, self.num_boxes, self.log = suffix, outputs, indices, float(num_boxes), log
        self.pairs = pairs      # the device solver's (2, P) int64 tensor behind ``indices``: the host then knows only where its pairs go


class SetCriterion(nn.Module):
    """The reference's DINO criterion: Hungarian assignment, then focal label loss, L1 + GIoU box loss and the cardinality error of every output set."""

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.losses = losses
        self.focal_alpha = focal_alpha

    # ------------------------------------------------------------------------------------------------------------------- the batched core
    def _run(self, jobs, targets, want):
        """{loss name: value} per job for the loss groups in ``want`` ('labels', 'cardinality', 'boxes')."""
        who = "SetCriterion"
        for loss in want:
            if loss == "masks":
                raise NotImplementedError("SetCriterion: the 'masks' loss (loss_masks / dice) is not implemented: segmentation is outside this library")
            assert loss in ("labels", "cardinality", "boxes"), f"do you really want to compute {loss} loss?"
        need_labels, need_boxes = "labels" in want or "cardinality" in want, "boxes" in want
        results = [dict() for _ in jobs]
        if not jobs or not (need_labels or need_boxes):
            return results
        for job in jobs:
            if need_labels:
                _check_float(who, "pred_logits", job.outputs["pred_logits"])
            if need_boxes:
                _check_float(who, "pred_boxes", job.outputs["pred_boxes"])
        dev = (jobs[0].outputs["pred_logits"] if need_labels else jobs[0].outputs["pred_boxes"]).device
        sizes = [len(t["labels"]) for t in targets]
        toff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        # the matched pairs of every job on the host: row b * Q + src of the job's (B * Q) rows, and the position of the target in the batch's concatenation
        rows, tgts, counts = [], [], []
        for job in jobs:
            ref = job.outputs["pred_logits"] if "pred_logits" in job.outputs else job.outputs["pred_boxes"]
            B, Q = ref.shape[:2]
            assert B == len(targets), f"{who}: {B} images in the outputs, {len(targets)} target dicts"
            if job.pairs is not None:                             # min(Q, n_b) pairs per image: what is added to the solver's src and tgt
                ks = [min(Q, n) for n in sizes]
                rows.append(np.repeat(np.arange(B, dtype=np.int64) * Q, ks))
                tgts.append(np.repeat(toff[:-1], ks))
            else:
                idx = _host_indices(job.indices)
                rows.append(np.concatenate([b * Q + i for b, (i, _) in enumerate(idx)]) if idx else np.zeros(0, np.int64))
                tgts.append(np.concatenate([toff[b] + j for b, (_, j) in enumerate(idx)]) if idx else np.zeros(0, np.int64))
            counts.append(int(rows[-1].shape[0]))
            job.B, job.Q = B, Q
        base = [0] + [int(x) for x in np.cumsum([job.B * job.Q for job in jobs])]
        n_pairs = sum(counts)
        plan = np.concatenate([np.concatenate(rows), np.concatenate([r + base[s] for s, r in enumerate(rows)]), np.concatenate(tgts),
                               np.asarray(sizes, dtype=np.int64)])
        on_device = any(job.pairs is not None for job in jobs)
        if on_device:                                             # pinned and asynchronous: the copy does not wait for the stream
            plan = torch.from_numpy(plan).pin_memory().to(dev, non_blocking=True)
        else:
            plan = torch.from_numpy(plan).to(dev)                 # the one host -> device copy
        local, glob, tsel, lengths = plan[:n_pairs], plan[n_pairs:2 * n_pairs], plan[2 * n_pairs:3 * n_pairs], plan[3 * n_pairs:]
        if on_device and n_pairs:                                 # the matched rows and target positions are formed here, from the solver's output
            solved = torch.cat([job.pairs if job.pairs is not None else torch.zeros(2, m, dtype=torch.int64, device=dev) for job, m in zip(jobs, counts)], 1)
            local, glob, tsel = local + solved[0], glob + solved[0], tsel + solved[1]
        starts = [0] + [int(x) for x in np.cumsum(counts)]

        if need_labels:
            C = jobs[0].outputs["pred_logits"].shape[2]
            labels_all = torch.cat([t["labels"] for t in targets]) if targets else torch.zeros(0, dtype=torch.int64, device=dev)
            if not labels_all.is_cuda:
                raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); the target labels are cpu tensors and there is no CPU fallback")
            cmap = torch.full((int(base[-1]),), self.num_classes, dtype=torch.int32, device=dev)      # every set's class map, one buffer
            if n_pairs:
                cmap[glob] = labels_all[tsel].to(torch.int32)
            tl = lengths.to(torch.float32)
            for lo in range(0, len(jobs), MAX_SETS):
                part = jobs[lo:lo + MAX_SETS]
                for job in part:
                    assert job.outputs["pred_logits"].shape[2] == C, f"{who}: the output sets differ in their number of classes"
                meta = _LabelMeta(C, self.focal_alpha, 2.0, [cmap[base[lo + k]:base[lo + k + 1]] for k in range(len(part))], [None] * len(part),
                                  [(job.B, job.Q) for job in part], [1.0 / job.num_boxes for job in part])
                loss, card, hits = _LabelLoss.apply(meta, *[job.outputs["pred_logits"] for job in part])
                if "cardinality" in want:                 # every set has the batch's B images: one pass for all of them
                    card_err = (card.to(torch.float32) - tl).abs().mean(1)
                for k, job in enumerate(part):
                    res = results[lo + k]
                    if "labels" in want:
                        res["loss_ce"] = loss[k]
                        if job.log:
                            m = counts[lo + k]
                            res["class_error"] = 100.0 - hits[k].to(torch.float32) * (100.0 / m) if m else torch.full((), 100.0, device=dev)
                    if "cardinality" in want:
                        res["cardinality_error"] = card_err[k]

        if need_boxes:
            boxes_all = torch.cat([t["boxes"] for t in targets]) if targets else torch.zeros(0, 4, device=dev)
            _check_float(who, "the target boxes", boxes_all)
            tgt_sel = _dense32(boxes_all)[tsel] if n_pairs else torch.zeros(0, 4, dtype=torch.float32, device=dev)
            for lo in range(0, len(jobs), MAX_SETS):
                part = jobs[lo:lo + MAX_SETS]
                srcs = [job.outputs["pred_boxes"].reshape(-1, 4)[local[starts[lo + k]:starts[lo + k + 1]]] for k, job in enumerate(part)]
                meta = _BoxMeta([tgt_sel[starts[lo + k]:starts[lo + k + 1]] for k in range(len(part))], [1.0 / job.num_boxes for job in part])
                out = _BoxLoss.apply(meta, *srcs)
                det = out.detach()
                for k in range(len(part)):
                    results[lo + k].update(loss_bbox=out[k, 3], loss_giou=out[k, 2], loss_xy=det[k, 0], loss_hw=det[k, 1])
        return results

    def _single(self, want, outputs, targets, indices, num_boxes, log=True):
        return self._run([_Job("", outputs, indices, num_boxes, log)], targets, want)[0]

    # ------------------------------------------------------------------------------------------------------------------ the reference's methods
    def loss_labels(self, outputs, targets, indices, num_boxes, log=True):
        """Classification loss (binary focal loss): loss_ce and, with log, class_error."""
        assert "pred_logits" in outputs
        return self._single(("labels",), outputs, targets, indices, num_boxes, log)

    @torch.no_grad()
    def loss_cardinality(self, outputs, targets, indices, num_boxes):
        """The absolute error in the number of predicted non-empty boxes (logging only)."""
        return self._single(("cardinality",), outputs, targets, indices, num_boxes)

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        """L1 and GIoU loss of the matched boxes (cxcywh, normalised): loss_bbox, loss_giou and the logged loss_xy, loss_hw."""
        assert "pred_boxes" in outputs
        return self._single(("boxes",), outputs, targets, indices, num_boxes)

    def loss_masks(self, outputs, targets, indices, num_boxes):
        raise NotImplementedError("SetCriterion: the 'masks' loss (loss_masks / dice) is not implemented: segmentation is outside this library")

    def get_loss(self, loss, outputs, targets, indices, num_boxes, **kwargs):
        loss_map = {"labels": self.loss_labels, "cardinality": self.loss_cardinality, "boxes": self.loss_boxes, "masks": self.loss_masks}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](outputs, targets, indices, num_boxes, **kwargs)

    def _match(self, sets, targets):
        """The matcher's indices of every set.  With ``cost_matrix``: every cost matrix is computed on the device, all go to the host in one copy."""
        if not hasattr(self.matcher, "cost_matrix"):
            return [self.matcher(o, targets) for o in sets]
        if getattr(self.matcher, "solver", "scipy") == "device":      # solved on the device, one launch per 16 sets: device index tensors, no copy
            return self.matcher.assign_sets(sets, targets)
        from scipy.optimize import linear_sum_assignment
        with torch.no_grad():
            costs = [self.matcher.cost_matrix(o, targets) for o in sets]
            flat = torch.cat([c.reshape(-1).to(torch.float32) for c in costs]).cpu()      # the single copy to the host
        sizes = [len(v["boxes"]) for v in targets]
        out = []
        for c, block in zip(costs, flat.split([c.numel() for c in costs])):
            block = block.view(c.shape)
            ind = [linear_sum_assignment(part[i]) for i, part in enumerate(block.split(sizes, -1))]
            out.append([(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in ind])
        return out

    def prep_for_dn(self, dn_meta):
        output_known_lbs_bboxes = dn_meta["output_known_lbs_bboxes"]
        num_dn_groups, pad_size = dn_meta["num_dn_group"], dn_meta["pad_size"]
        assert pad_size % num_dn_groups == 0
        return output_known_lbs_bboxes, pad_size // num_dn_groups, num_dn_groups

    def forward(self, outputs, targets, return_indices=False):
        """The reference's dict of losses (the same keys, the zero-valued ``*_dn`` ones included).  outputs: pred_logits (B, Q, C), pred_boxes (B, Q, 4),
        dn_meta, optionally aux_outputs, interm_outputs, enc_outputs; targets: one dict of labels (n,) and boxes (n, 4) per image, on the device."""
        for loss in self.losses:
            if loss == "masks":
                raise NotImplementedError("SetCriterion: the 'masks' loss (loss_masks / dice) is not implemented: segmentation is outside this library")
        outputs_without_aux = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        first = next(iter(outputs.values()))
        _check_float("SetCriterion", "the first output", first)
        device = first.device

        num_boxes = sum(len(t["labels"]) for t in targets)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            nb = torch.as_tensor([num_boxes], dtype=torch.float, device=device)
            torch.distributed.all_reduce(nb)
            num_boxes = torch.clamp(nb / torch.distributed.get_world_size(), min=1).item()
        else:
            num_boxes = max(float(num_boxes), 1.0)

        # the sets that are matched, in the reference's order
        matched = [("", outputs_without_aux, True)]
        matched += [(f"_{i}", aux, False) for i, aux in enumerate(outputs.get("aux_outputs", []))]
        if "interm_outputs" in outputs:
            matched.append(("_interm", outputs["interm_outputs"], False))
        matched += [(f"_enc_{i}", enc, False) for i, enc in enumerate(outputs.get("enc_outputs", []))]
        all_indices = self._match([o for _, o, _ in matched], targets)
        all_pairs = [None] * len(matched)
        if isinstance(all_indices, tuple):                       # the device solver: the indices as views, and the tensors they are views of
            all_indices, all_pairs = all_indices
        jobs = [_Job(sfx, o, ind, num_boxes, log, pairs) for (sfx, o, log), ind, pairs in zip(matched, all_indices, all_pairs)]

        dn_meta = outputs["dn_meta"]
        use_dn = bool(self.training and dn_meta and "output_known_lbs_bboxes" in dn_meta)
        if use_dn:
            known, single_pad, scalar = self.prep_for_dn(dn_meta)
            dn_pos_idx = []
            groups = torch.arange(scalar, dtype=torch.int64) * single_pad
            for t in targets:                                    # host tensors: no per-image device allocation
                n = len(t["labels"])
                tt = torch.arange(n, dtype=torch.int64).unsqueeze(0).repeat(scalar, 1)
                dn_pos_idx.append(((groups.unsqueeze(1) + tt).flatten(), tt.flatten()))
            jobs.append(_Job("_dn", known, dn_pos_idx, num_boxes * scalar, False))
            jobs += [_Job(f"_dn_{i}", known["aux_outputs"][i], dn_pos_idx, num_boxes * scalar, False) for i in range(len(outputs.get("aux_outputs", [])))]

        results = {job.suffix: res for job, res in zip(jobs, self._run(jobs, targets, tuple(self.losses)))}

        def named(suffix):
            return {k + suffix: v for k, v in results[suffix].items()}

        zero = torch.zeros((), dtype=torch.float32, device=device)
        zero_dn = ("loss_bbox_dn", "loss_giou_dn", "loss_ce_dn", "loss_xy_dn", "loss_hw_dn", "cardinality_error_dn")
        losses = {}
        losses.update(named("_dn") if use_dn else {k: zero for k in zero_dn})
        losses.update(named(""))
        for i in range(len(outputs.get("aux_outputs", []))):
            losses.update(named(f"_{i}"))
            losses.update(named(f"_dn_{i}") if use_dn else {f"{k}_{i}": zero for k in zero_dn})
        if "interm_outputs" in outputs:
            losses.update(named("_interm"))
        for i in range(len(outputs.get("enc_outputs", []))):
            losses.update(named(f"_enc_{i}"))

        if return_indices:
            return losses, all_indices[1:] + [all_indices[0]]
        return losses
