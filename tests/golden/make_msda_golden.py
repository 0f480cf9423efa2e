#!/usr/bin/env python3
"""Generate tests/golden/msda_cases.npz by running the REAL reference ``ms_deform_attn_core_pytorch``
(``downstream/object_detection/dino/models/dino/ops/functions/ms_deform_attn_func.py`` of an upstream checkout) on the CPU.

    python tests/golden/make_msda_golden.py [REFERENCE_ROOT]     # default: /root/reference

The file is loaded by path, unmodified; its ``import MultiScaleDeformableAttention`` (the CUDA extension) is satisfied by an empty stub module placed
in ``sys.modules`` -- only the pure-PyTorch core function is called.  For the cases tests/msda_refs.py lists in GOLDEN_CASES (fp32 inputs) the npz
holds the inputs (fp32 / int64), the core function's output evaluated in float64 and its three autograd gradients under the case's grad_out (float64).
Only data is written; tests read the committed file and never the reference.
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
sys.path.insert(0, ROOT)

from tests import msda_refs as R  # noqa: E402


def load_reference_core():
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    path = os.path.join(REF, "downstream", "object_detection", "dino", "models", "dino", "ops", "functions", "ms_deform_attn_func.py")
    spec = importlib.util.spec_from_file_location("ref_ms_deform_attn_func", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ms_deform_attn_core_pytorch


def main():
    core = load_reference_core()
    arrays = {}
    for case_id in R.GOLDEN_CASES:
        inp = R.make_inputs(case_id, torch.float32)
        value, loc, attn = (inp[k].double().requires_grad_(True) for k in ("value", "loc", "attn"))
        out = core(value, inp["shapes"], loc, attn)
        out.backward(inp["grad_out"].double())
        for k in ("value", "loc", "attn", "grad_out", "shapes", "starts"):
            arrays[f"c{case_id}_{k}"] = inp[k].numpy()
        for k, t in (("out", out.detach()), ("grad_value", value.grad), ("grad_sampling_loc", loc.grad), ("grad_attn_weight", attn.grad)):
            assert t.dtype == torch.float64
            arrays[f"c{case_id}_{k}"] = t.numpy()
    path = os.path.join(HERE, "msda_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
