#!/usr/bin/env python3
"""Generate tests/golden/criterion_cases.npz by running the REAL reference programs of an upstream checkout on the CPU, in float64:
``downstream/object_detection/dino/util/box_ops.py``, ``models/dino/utils.py`` (sigmoid_focal_loss), ``models/dino/matcher.py`` (HungarianMatcher) and
``models/dino/dino.py`` (SetCriterion, with its denoising, aux and interm branches).

    python tests/golden/make_criterion_golden.py [REFERENCE_ROOT]     # default: /root/reference

The four files are loaded by path, unmodified, the way make_detection_golden.py loads three of them.  ``util.misc`` is a stub that carries this project's own
``accuracy`` (top-1, in per cent; 0 for no target, as upstream's), ``get_world_size`` (1) and ``is_dist_avail_and_initialized`` (False); dino.py's other
siblings are do-nothing stubs.  The criterion moves its denoising indices and zero losses to ``'cuda'`` by name: inside this generator only,
``Tensor.cuda()`` and ``Tensor.to('cuda')`` are identities, so that everything stays on the CPU.

Per case of tests/criterion_refs.FORWARD_CASES the file holds every returned loss, the gradient of the weighted total (criterion_refs.weight_dict) with
respect to every pred_logits / pred_boxes, the matcher's indices of every matched set, and a checksum of the inputs (they are regenerated from their seeds,
not stored); and, per LABEL_CASES entry, the value of the reference's sigmoid_focal_loss on dense one-hot targets.  Only data is written; tests read the
committed file, never the reference.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_detection_golden as G  # noqa: E402  (its loader and stubs)
from tests import criterion_refs as R  # noqa: E402

F64 = torch.float64


@torch.no_grad()
def accuracy(output, target, topk=(1,)):
    if target.numel() == 0:
        return [torch.zeros([], device=output.device)]
    return [(output.argmax(1) == target).float().sum() * (100.0 / target.numel())]


def load_reference():
    box_ops, _, _ = G.load_reference()      # util.box_ops, the matcher and a dino.py with stubbed siblings: loaded again below with the real utils
    misc = types.ModuleType("util.misc")
    for name in ("NestedTensor", "nested_tensor_from_tensor_list", "interpolate", "inverse_sigmoid"):
        setattr(misc, name, G._Anything())
    misc.accuracy, misc.get_world_size, misc.is_dist_avail_and_initialized = accuracy, (lambda: 1), (lambda: False)
    sys.modules["util.misc"] = misc
    sys.modules["util"].misc = misc
    utils = G._load("refdino.models.dino.utils", os.path.join(G.DINO, "models", "dino", "utils.py"))
    dino = G._load("refdino.models.dino.dino", os.path.join(G.DINO, "models", "dino", "dino.py"))
    return box_ops, utils, sys.modules["refdino.models.dino.matcher"], dino


def cpu_only():
    """Tensor.cuda() and Tensor.to('cuda') as identities (this process only)."""
    to = torch.Tensor.to

    def to_cpu(self, *a, **k):
        if a and isinstance(a[0], str) and a[0].startswith("cuda"):
            return self
        return to(self, *a, **k)
    torch.Tensor.to = to_cpu
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    _, utils, matcher, dino = load_reference()
    cpu_only()
    arrays = {}

    for case in range(len(R.LABEL_CASES)):
        logits, classes, num_boxes = R.label_inputs(case)
        B, Q, C = logits.shape
        t = R.onehot(classes, C, F64).view(B, Q, C)
        arrays[f"focal{case}"] = np.array(utils.sigmoid_focal_loss(logits.double(), t, num_boxes, alpha=R.FOCAL_ALPHA, gamma=2).item())

    for case, c in enumerate(R.FORWARD_CASES):
        outputs, targets, _ = R.forward_inputs(case)
        name = c["name"]
        out64 = R.convert(outputs, lambda v: v.double().requires_grad_(True))
        tg64 = R.convert_targets(targets, lambda v: v.double() if v.is_floating_point() else v)
        weights = R.weight_dict(c["aux"], c["interm"])
        crit = dino.SetCriterion(C := c["C"], matcher.HungarianMatcher(**R.MATCH_WEIGHTS), weights, R.FOCAL_ALPHA, list(R.LOSSES))
        assert crit.training and C == outputs["pred_logits"].shape[2]
        losses, indices_list = crit(out64, tg64, return_indices=True)
        indices = [indices_list[-1]] + indices_list[:-1]      # the reference lists aux .., interm, then the main set
        arrays[f"{name}_keys"] = np.array(sorted(losses))
        for k, v in losses.items():
            arrays[f"{name}_loss_{k}"] = np.array(v.detach().double().item())
        total = sum(losses[k] * weights[k] for k in losses if k in weights)
        sets = R.pred_sets(out64)
        leaves = [o[k] for _, o in sets for k in ("pred_logits", "pred_boxes")]
        grads = torch.autograd.grad(total, leaves, allow_unused=True) if total.requires_grad else [None] * len(leaves)
        for (sname, _), gl, gb in zip(sets, grads[0::2], grads[1::2]):
            o = dict(sets)[sname]
            arrays[f"{name}_grad_{sname}_logits"] = (gl if gl is not None else torch.zeros_like(o["pred_logits"])).detach().numpy()
            arrays[f"{name}_grad_{sname}_boxes"] = (gb if gb is not None else torch.zeros_like(o["pred_boxes"])).detach().numpy()
        for s, ind in enumerate(indices):
            for b, (i, j) in enumerate(ind):
                arrays[f"{name}_idx{s}_{b}_src"], arrays[f"{name}_idx{s}_{b}_tgt"] = i.numpy().astype(np.int64), j.numpy().astype(np.int64)
        arrays[f"{name}_checksum"] = R.checksum(outputs, targets)

    path = os.path.join(HERE, "criterion_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
