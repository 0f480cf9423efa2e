#!/usr/bin/env python3
"""Generate the goldens of the multi-scale detection backbone by running the REAL reference detection file
(``downstream/object_detection/dino/models/dino/fastervit.py`` of an upstream checkout) in the build container.

    python tests/golden/make_backbone_golden.py [REFERENCE_ROOT]     # default: /root/reference

The file is loaded by path, unmodified, with the test-only timm shim (tests/golden/_shim) and a stub ``util.misc`` (tests/golden/_dino_stub)
on the path.  Weights are tests/synth.py's (BatchNorm running statistics of ``norm{i}`` included); inputs and masks are seeded.  Writes
tests/golden/backbone_<case>.npz (per-level outputs ``out{k}`` and masks ``mask{k}``, fp32 / bool) and tests/golden/backbone_keys.json
(key/shape digests of the eight builder names, and the missing / unexpected keys the reference backbone reports when it loads the matching
classification state_dict with strict=False).  Tests only ever read the committed files.
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, os.path.join(HERE, "_dino_stub"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from fastervit.models import create_model as ref_create_model  # noqa: E402

from tests.backbone_cases import BACKBONE_CASES, BATCH, SEED, make_mask  # noqa: E402
from tests.synth import synth_input, synth_state_dict  # noqa: E402


def _load_det():
    path = os.path.join(REF, "downstream", "object_detection", "dino", "models", "dino", "fastervit.py")
    spec = importlib.util.spec_from_file_location("ref_det_fastervit", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(sd):
    lines = sorted(f"{k}:{tuple(v.shape)}:{str(v.dtype).replace('torch.', '')}" for k, v in sd.items())
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines)


def run_case(det, name, case):
    from util.misc import NestedTensor
    torch.manual_seed(0)
    model = det.build_fastervit(case["name"], **case["kwargs"])
    model.eval()   # (the reference's train() returns None)
    sd = synth_state_dict(model.state_dict(), SEED, case["family"])
    model.load_state_dict(sd, strict=True)
    H, W = case["hw"]
    x = synth_input(BATCH, H, W, SEED)
    mask = make_mask(case["mask"], BATCH, H, W)
    with torch.no_grad():
        out = model(NestedTensor(x, mask))
    store = {}
    for k, nt in out.items():
        store[f"out{k}"] = nt.tensors.float().numpy()
        store[f"mask{k}"] = nt.mask.numpy()
    path = os.path.join(HERE, f"backbone_{name}.npz")
    np.savez_compressed(path, **store)
    print(f"{name}: {[v.shape for v in store.values()]} -> {os.path.getsize(path) / 1e6:.2f} MB")


def keys(det):
    """Digests of the eight builder names at their defaults (out_indices (0, 1, 2, 3)) and the strict=False load report."""
    rec = {}
    for name in _NAMES:
        bb = det.build_fastervit(name)
        cls = ref_create_model(name)
        h, n = digest(bb.state_dict())
        res = bb.load_state_dict(cls.state_dict(), strict=False)
        rec[name] = dict(sha256=h, n=n, num_features=list(bb.num_features), missing=sorted(res.missing_keys),
                         unexpected=sorted(res.unexpected_keys))
        print(name, n, len(res.missing_keys), len(res.unexpected_keys))
    with open(os.path.join(HERE, "backbone_keys.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


_NAMES = ["faster_vit_0_224", "faster_vit_1_224", "faster_vit_2_224", "faster_vit_3_224", "faster_vit_4_224", "faster_vit_4_21k_224",
          "faster_vit_4_21k_384", "faster_vit_4_21k_512"]


if __name__ == "__main__":
    det = _load_det()
    keys(det)
    for name, case in BACKBONE_CASES.items():
        run_case(det, name, case)
