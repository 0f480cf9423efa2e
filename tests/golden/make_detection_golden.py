#!/usr/bin/env python3
"""Generate tests/golden/detection_cases.npz by running the REAL reference programs of an upstream checkout on the CPU:
``downstream/object_detection/dino/util/box_ops.py`` (box_iou, generalized_box_iou), ``models/dino/matcher.py`` (HungarianMatcher) and
``models/dino/dino.py`` (PostProcess).

    python tests/golden/make_detection_golden.py [REFERENCE_ROOT]     # default: /root/reference

The three files are loaded by path, unmodified.  What they import and this machine lacks, or what is not needed, is satisfied by stub modules in
``sys.modules``: ``torchvision.ops.boxes`` carries this project's own ``box_area`` and an ``nms`` bound to the restatement of torchvision's rule
(tests/detection_refs.py: NMS has no reference program here, the restatement IS its yardstick, and the golden of PostProcess with NMS on says no more
than that the reference's PostProcess, given that nms, returns these rows); ``util.misc`` and dino.py's sibling modules (backbone, transformer,
segmentation, ...) are stubs whose every attribute is a do-nothing placeholder, since only the PostProcess class is used.  The matcher's cost matrix
``C`` is recorded by replacing the loaded module's ``linear_sum_assignment`` name with a recorder (one image per case, so the one recorded block is the
whole matrix).

Inputs are the fp32 case inputs of tests/detection_refs.py; every program is run on their float64 images (results float64), PostProcess also on the
fp32 inputs themselves for the boxes, which the kernels must reproduce bit for bit.  Inputs are not stored (they are regenerated from their seeds); a
float64 checksum per case is, so that a generator drift is reported as such.  Only data is written; tests read the committed file, never the reference.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
DINO = os.path.join(REF, "downstream", "object_detection", "dino")
sys.path.insert(0, ROOT)

from tests import detection_refs as R  # noqa: E402

F64 = torch.float64


class _Anything:
    """Placeholder for every name the stubbed modules are asked for: callable, usable as a decorator (returns the decorated function), subscriptable."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return a[0] if len(a) == 1 and callable(a[0]) and not k else _Anything()

    def __getattr__(self, name):
        return _Anything()


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _nms(boxes, scores, iou_threshold):
    order = torch.sort(scores, descending=True, stable=True).indices
    return R.nms_rule(boxes, order, iou_threshold, boxes.dtype)


def load_reference():
    tv, tvo, tvb = _Stub("torchvision"), _Stub("torchvision.ops"), types.ModuleType("torchvision.ops.boxes")
    tvb.box_area, tvb.nms = R.box_area, _nms
    tv.ops, tvo.boxes = tvo, tvb
    sys.modules.update({"torchvision": tv, "torchvision.ops": tvo, "torchvision.ops.boxes": tvb})
    box_ops = _load("util.box_ops", os.path.join(DINO, "util", "box_ops.py"))
    util = _Stub("util")
    util.__path__ = []
    util.box_ops = box_ops
    sys.modules.update({"util": util, "util.misc": _Stub("util.misc")})
    matcher = _load("refdino.models.dino.matcher", os.path.join(DINO, "models", "dino", "matcher.py"))
    for pkg in ("refdino", "refdino.models", "refdino.models.dino"):
        m = _Stub(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    for sib in ("backbone", "segmentation", "deformable_transformer", "utils", "dn_components"):
        sys.modules[f"refdino.models.dino.{sib}"] = _Stub(f"refdino.models.dino.{sib}")
    sys.modules["refdino.models.registry"] = _Stub("refdino.models.registry")
    dino = _load("refdino.models.dino.dino", os.path.join(DINO, "models", "dino", "dino.py"))
    return box_ops, matcher, dino


def main():
    box_ops, matcher, dino = load_reference()
    arrays = {}

    for case, raw, test in R.SELECT_RUNS:
        logits, boxes, sizes, K = R.select_inputs(case)
        name = R.run_name(case, raw, test)
        pp = dino.PostProcess(num_select=K)
        res = pp({"pred_logits": logits.double(), "pred_boxes": boxes.double()}, sizes.double(), not_to_xyxy=raw, test=test)
        res32 = pp({"pred_logits": logits, "pred_boxes": boxes}, sizes, not_to_xyxy=raw, test=test)
        arrays[f"{name}_scores"] = torch.stack([r["scores"] for r in res]).numpy()
        arrays[f"{name}_labels"] = torch.stack([r["labels"] for r in res]).numpy()
        arrays[f"{name}_boxes"] = torch.stack([r["boxes"] for r in res]).numpy()
        arrays[f"{name}_boxes32"] = torch.stack([r["boxes"] for r in res32]).numpy()
        assert arrays[f"{name}_scores"].dtype == np.float64 and arrays[f"{name}_boxes32"].dtype == np.float32
        arrays[f"{name}_checksum"] = np.array([logits.double().sum().item(), boxes.double().sum().item()])

    # PostProcess with NMS on (the stubbed nms = the restatement): rows of all images concatenated + counts
    logits, boxes, sizes, K = R.select_inputs(R.PP_NMS_CASE)
    res = dino.PostProcess(num_select=K, nms_iou_threshold=R.PP_NMS_THR)({"pred_logits": logits.double(), "pred_boxes": boxes.double()}, sizes.double())
    arrays["ppnms_counts"] = np.array([len(r["scores"]) for r in res], dtype=np.int64)
    for k in ("scores", "labels", "boxes"):
        arrays[f"ppnms_{k}"] = torch.cat([r[k] for r in res]).numpy()

    for case in range(len(R.PAIR_CASES)):
        b1, b2 = R.pair_inputs(case)
        iou, union = box_ops.box_iou(b1.double(), b2.double())
        arrays[f"pair{case}_iou"], arrays[f"pair{case}_union"] = iou.numpy(), union.numpy()
        arrays[f"pair{case}_giou"] = box_ops.generalized_box_iou(b1.double(), b2.double()).numpy()
        arrays[f"pair{case}_checksum"] = np.array([b1.double().sum().item(), b2.double().sum().item()])

    recorded = []
    matcher.linear_sum_assignment = lambda c: (recorded.append(c.clone()), (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))[1]
    for case in range(len(R.COST_CASES)):
        logits, pred, ids, tgt = R.cost_inputs(case)
        m = matcher.HungarianMatcher(**R.COST_WEIGHTS)
        del recorded[:]
        m({"pred_logits": logits.double()[None], "pred_boxes": pred.double()[None]}, [{"labels": ids, "boxes": tgt.double()}])
        assert len(recorded) == 1 and recorded[0].dtype == F64 and tuple(recorded[0].shape) == (logits.shape[0], tgt.shape[0])
        arrays[f"cost{case}_C"] = recorded[0].numpy()
        arrays[f"cost{case}_checksum"] = np.array([logits.double().sum().item(), pred.double().sum().item() + tgt.double().sum().item()])

    path = os.path.join(HERE, "detection_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
