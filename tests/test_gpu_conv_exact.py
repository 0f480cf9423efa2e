"""Every 3x3 conv and stem route of csrc/fvit_conv_*.hip and csrc/fvit_stem.hip on the integer cases of tests/conv_refs.py: inputs, weights, bias and residual are small
integers, every partial sum is an integer of magnitude <= 256 -- exact in fp32, fp16 and bf16 in any summation order -- so the kernel's output must
EQUAL the reference (torch.equal on the values; -0 equals +0).  One dropped or mis-addressed (tap, channel) product at one pixel changes an integer.

Routes are forced with tests.util.tuned and checked by name (fvit_conv3x3_route_name); buffers are poisoned with NaN around the maps and in the pad
channels (tests/conv_launch.py).  tests/test_conv_refs_cpu.py holds the CPU side: the <= 256 condition, and the reference mutants these cases catch.
Not here: the <ln> instances (their 1-ulp tests are tests/test_gpu_level_glue_fusion.py and tests/test_gpu_conv_driver.py) and
fvit_stem_conv3x3s2_px (tests/test_gpu_conv_values.py)."""
import pytest
import torch

from tests import conv_refs as R
from tests.conv_launch import ConvRun, knobs, run_stem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.CONV_CASES, ids=R.case_id)
def test_conv_integer_case(c, dt):
    inp = R.int_inputs(c)
    run = ConvRun(c, inp, dt)
    px = "px" in c.route
    with knobs(c):
        for act in (0, 1):
            for res in ((False, "hi", True) if px else (False, True)):
                got, want = run.run(act, res), R.conv3x3.exact(inp, act, res)
                value = got["f32"] if c.out == "f32" else got["hi"]
                assert torch.equal(value, want), (act, res, (value - want).abs().max().item(), int((value != want).sum()))
                if c.out == "lo":
                    assert torch.equal(got["lo"], torch.zeros_like(want)), (act, res)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.STEM_CONV_CASES + R.STEM_FUSED_CASES, ids=R.stem_id)
def test_stem_integer_case(c, dt):
    inp = R.stem_int_inputs(c)
    got, want = run_stem(c, inp, dt), R.stem_ref(c).exact(inp)
    assert torch.equal(got, want), ((got - want).abs().max().item(), int((got != want).sum()))
