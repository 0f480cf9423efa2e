"""No GPU: the proof that the references, the inputs and the bar of tests/test_gpu_msda.py are fair (tests/msda_refs.py), plus the structural checks
of the new surface (C ABI symbols, the Python entry points without a device).

    * ``exact`` agrees with the reference's own ms_deform_attn_core_pytorch (tests/golden/msda_cases.npz, float64) to 1e-12 of the tensor's peak
    * no sample of any case sits within 0.05 of an integer pixel coordinate, where the location gradient jumps
    * other legitimate fp32 evaluations (corners summed in reverse, the coordinate as (2 loc n - 1) / 2, levels summed last to first) stay at or under
      half the bar on every tensor of every case
    * seven wrong answers each exceed the bar on at least one case and break equality on the exact cases"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fastervit_amd import _lib
from tests import msda_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "msda_cases.npz"))


@pytest.mark.parametrize("case_id", R.GOLDEN_CASES)
def test_exact_agrees_with_the_reference_core(golden, case_id):
    inp, ex, _ = R.references(case_id, F32)
    for k in ("value", "loc", "attn", "grad_out", "shapes", "starts"):
        assert torch.equal(torch.from_numpy(golden[f"c{case_id}_{k}"]), inp[k]), f"the inputs of case {case_id} changed ({k}): regenerate the golden"
    for k in R.TENSORS:
        want = torch.from_numpy(golden[f"c{case_id}_{k}"])
        assert want.dtype == torch.float64
        got = ex[k].reshape(want.shape)
        err, peak = (got - want).abs().max().item(), want.abs().max().item()
        print(f"case {case_id} {k}: max |exact - reference| = {err:.1e} (peak {peak:.2f})")
        assert err <= 1e-12 * peak


def _all_inputs():
    for case_id, far in R.value_case_params():
        for dt in R.DTYPES:
            yield f"case {case_id}{' far' if far else ''} {dt}", R.references(case_id, dt, far)


def test_no_sample_is_near_an_integer_coordinate():
    worst = 1.0
    for name, (inp, _, _) in _all_inputs():
        margin = R.fraction_margin(inp)
        assert margin >= R.MARGIN, f"{name}: a pixel coordinate's fractional part is within {margin:.3f} of an integer"
        worst = min(worst, margin)
    print(f"smallest margin over all cases: {worst:.3f}")


@pytest.mark.parametrize("how", R.VARIANTS)
def test_other_fp32_evaluations_stay_under_half_the_bar(how):
    worst = 0.0
    for name, (inp, ex, p32) in _all_inputs():
        got = R.evaluate(inp, F32, how)
        for k, v in R.ratios(got, ex, p32, {t: F32 for t in R.TENSORS}).items():   # the fp32 bar: the tightest one
            assert v <= 0.5, f"{how}, {name}, {k}: {v:.3f} x the bar"
            worst = max(worst, v)
    print(f"{how}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("how", R.MUTANTS)
def test_mutants_exceed_the_bar_and_break_the_exact_cases(how):
    caught = []
    for case_id, far in R.value_case_params():
        inp, ex, p32 = R.references(case_id, F32, far)
        got = R.evaluate(inp, torch.float64, how)                                   # the wrong formula, evaluated without rounding error
        worst = max(R.ratios(got, ex, p32, {t: torch.bfloat16 for t in R.TENSORS}).values())   # the bf16 bar: the widest one any test applies
        if worst > 1.0:
            caught.append(case_id)
    print(f"{how}: over the bar on cases {caught}")
    assert caught, f"{how} passes every value case: add a case, never widen the bar"
    for D in R.EXACT_D:
        inp, ex = R.exact_references(D, F32)
        got = R.evaluate(inp, F32, how)
        assert any(not torch.equal(got[k].double(), ex[k]) for k in R.TENSORS), f"{how} survives the exact case D={D}"


@pytest.mark.parametrize("D", R.EXACT_D)
def test_exact_cases_are_exact_in_fp32_in_any_order(D):
    inp, ex = R.exact_references(D, F32)
    for how in (None,) + R.VARIANTS:
        got = R.evaluate(inp, F32, how)
        for k in R.TENSORS:
            assert torch.equal(got[k].double(), ex[k]), (how, k)
    for dt in (torch.float16, torch.bfloat16):       # the same inputs are representable in both 16-bit types
        R.make_exact_inputs(D, dt)
    locs = inp["loc"].double()
    for l, (H, W) in enumerate(inp["shapes"].tolist()):
        assert ((locs[..., l, :, 0] * W * 4).frac() == 0).all() and ((locs[..., l, :, 1] * H * 4).frac() == 0).all()
    assert inp["attn"].sum((-1, -2)).max() <= 2 and ((inp["attn"] * 8).frac() == 0).all()
    # the one-sided derivative at frac = 0 is in play: some coordinates are integers
    assert ((locs[..., 0, :, 0] * EXACT_W0 - 0.5).frac() == 0).any()


EXACT_W0 = R.EXACT_LEVELS[0][1]


# ---- structural checks (these fail on a tree without the op) ----------------------------------------------------------------------------------
def test_header_declares_and_libraries_export_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    diag_section = hdr[hdr.index("#ifdef FVIT_DIAG"):hdr.index("#endif /* FVIT_DIAG */")]
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    for sym in ("fvit_msda_forward", "fvit_msda_backward"):
        assert re.search(rf"\bint {sym}\s*\(", hdr) and sym not in diag_section
        assert sym in _lib.EXPORTED_SYMBOLS and not sym.startswith("fvit_debug_")
        for so in ("libfvit_hip.so", "libfvit_hip_diag.so"):
            assert hasattr(ctypes.CDLL(os.path.join(_lib.CSRC_DIR, so)), sym), (so, sym)
    assert "#define FVIT_ABI_VERSION 10" in hdr and _lib.FVIT_ABI_VERSION == 10 and _lib.FVIT_PROF_KINDS == 11
    handle = _lib.lib()
    assert len(handle.fvit_msda_forward.argtypes) == 15 and len(handle.fvit_msda_backward.argtypes) == 18


def test_ops_raise_without_a_hip_device():
    import fastervit_amd
    from fastervit_amd import ops
    assert fastervit_amd.ms_deform_attn is ops.ms_deform_attn and fastervit_amd.MSDeformAttn is ops.MSDeformAttn
    assert fastervit_amd.MSDeformAttnFunction is ops.MSDeformAttnFunction
    inp = R.make_inputs(1, F32)
    args = (inp["value"], inp["shapes"], inp["starts"], inp["loc"], inp["attn"])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ms_deform_attn(*args)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.MSDeformAttnFunction.apply(*args, 64)
    m = ops.MSDeformAttn(d_model=32, n_levels=2, n_heads=2, n_points=2)
    S = int((inp["shapes"][:, 0] * inp["shapes"][:, 1]).sum())
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.randn(1, 3, 32), torch.rand(1, 3, 2, 2), torch.randn(1, S, 32), inp["shapes"], inp["starts"])
    src = open(os.path.join(ROOT, "fastervit_amd", "ops.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M) and "grid_sample" not in src


def test_module_has_the_reference_parameters_and_initialisation():
    from fastervit_amd.ops import MSDeformAttn
    torch.manual_seed(0)
    m = MSDeformAttn()
    want = {"sampling_offsets.weight": (256, 256), "sampling_offsets.bias": (256,), "attention_weights.weight": (128, 256),
            "attention_weights.bias": (128,), "value_proj.weight": (256, 256), "value_proj.bias": (256,), "output_proj.weight": (256, 256),
            "output_proj.bias": (256,)}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert list(m.state_dict()) == list(want)
    m = MSDeformAttn(d_model=64, n_levels=3, n_heads=4, n_points=2)
    assert (m.d_model, m.n_levels, m.n_heads, m.n_points) == (64, 3, 4, 2)
    assert tuple(m.sampling_offsets.weight.shape) == (4 * 3 * 2 * 2, 64) and tuple(m.attention_weights.weight.shape) == (4 * 3 * 2, 64)
    # the initialisation: zero offset / attention weights, heads looking along the axes of the unit square (4 heads: +x, +y, -x, -y), point i at i + 1 steps
    assert not m.sampling_offsets.weight.any() and not m.attention_weights.weight.any() and not m.attention_weights.bias.any()
    b = m.sampling_offsets.bias.detach().view(4, 3, 2, 2)
    axes = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    for p in range(2):
        assert torch.allclose(b[:, :, p], ((p + 1) * axes)[:, None, :].expand(4, 3, 2), atol=1e-6)
    assert not m.value_proj.bias.any() and not m.output_proj.bias.any()
    limit = (6.0 / (64 + 64)) ** 0.5
    for w in (m.value_proj.weight, m.output_proj.weight):
        assert w.abs().max() <= limit and w.std() > 0.4 * limit
    with pytest.raises(ValueError):
        MSDeformAttn(d_model=30, n_heads=4)
