"""The deploy plans launch the conv kernels they launched before the conv driver: the (kernel name, grid) of every conv-kind record of the
kernel timer during one forward, in launch order, against tests/golden/conv_launches.json -- recorded with ``record`` below on an MI355X at the
commit before `fvit_conv3x3` / `choose_conv_route` existed (Python chose between the row-band, LayerNorm2d and implicit-GEMM entry points then).

Cases: tiny_hier with the 16-bit and the precise plan (padded channels, dense K, px routes), tiny_d40 (padded channels, dense K), fvit0_224 at
batch 2 (fused stem, halo, band, both LayerNorm2d epilogues), backbone case bb_tiny_odd through ``BackboneDeployPlan`` (odd, window-padded maps)."""
import json
import os

import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib
from tests.backbone_cases import BACKBONE_CASES, BATCH, SEED
from tests.synth import synth_input, synth_state_dict
from tests.util import build_product_model, case_input

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_launches.json")
CASES = ["tiny_hier", "tiny_hier_precise", "tiny_d40", "fvit0_224_b2", "bb_tiny_odd"]


def _plan_and_input(case):
    if case == "bb_tiny_odd":
        c = BACKBONE_CASES[case]
        model = fastervit_amd.build_fastervit(c["name"], **c["kwargs"])
        model.load_state_dict(synth_state_dict(model.state_dict(), SEED, c["family"]), strict=True)
        model = model.eval().to("cuda:0").requires_grad_(False)
        model.switch_to_deploy()
        return model.__dict__["_deploy_plan"], synth_input(BATCH, *c["hw"], SEED).to("cuda:0")
    name = {"tiny_hier_precise": "tiny_hier", "fvit0_224_b2": "fvit0_224"}.get(case, case)
    model, _ = build_product_model(name, "cuda:0")
    model.switch_to_deploy(torch.float16)
    plan = model.__dict__["_deploy_plan"]
    plan.precise = case.endswith("_precise")
    return plan, case_input(name)[:2].to("cuda:0")


def record(case):
    """(conv launches [[name, grid], ...] of one ``forward_single``, its output tensors on the CPU)."""
    plan, x = _plan_and_input(case)
    with torch.no_grad():
        plan.forward_single(x)   # packs the weights, sizes the workspaces
        _lib.prof_enable(True)
        try:
            out = plan.forward_single(x)
            recs = _lib.prof_records()
        finally:
            _lib.prof_enable(False)
    outs = [o.float().cpu() for o in (out if isinstance(out, tuple) else (out,))]
    return [[r["name"], r["grid"]] for r in recs if r["kind"] == "conv3x3"], outs


@pytest.mark.parametrize("case", CASES)
def test_plan_launches_the_recorded_conv_kernels(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got, _ = record(case)
    print(f"{case}: {got}")
    assert got == want
