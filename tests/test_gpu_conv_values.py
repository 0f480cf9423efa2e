"""The 16-bit conv and stem routes of csrc/fvit_conv_*.hip and csrc/fvit_stem.hip on random inputs, held to the bar of tests/conv_refs.py: one correct rounding to the output
type plus 8 x the error of a plain fp32 evaluation of the same sum (plus G, the documented error of the gelu_fast polynomial, for act 2), against
float64 on the values the kernel receives.  Activations 0 / 1 / 2, without a residual, with one, and in place over it; fp16 and bf16.  Every case
prints its worst error / bar.  tests/test_conv_refs_cpu.py shows on the CPU that other fp32 summation orders meet this bar and which errors do not.

The two-term-map (px) conv routes keep their 2e-6 x scale check (tests/test_gpu_px.py, tests/test_gpu_conv_driver.py): that is already the level of fp32
accumulation.  Also here: fvit_layernorm2d_cl on channel-padded maps, the real channels to the same bar and the pad channels exactly zero."""
import ctypes

import pytest
import torch

from fastervit_amd import _lib
from tests import conv_refs as R
from tests.conv_launch import CODE, ConvRun, knobs, run_stem, stream
from tests.conv_refs import F32, F64, conv3x3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.VALUE_CASES, ids=R.case_id)
def test_conv_values(c, dt):
    inp = R.value_inputs(c, dt)
    run = ConvRun(c, inp, dt)
    s64, s32 = conv3x3.presum(inp, F64), conv3x3.presum(inp, F32)
    worst = {}
    with knobs(c):
        for act in (0, 1, 2):
            for res, in_place in ((False, False), (True, False), (True, True)):
                ex, p32 = conv3x3.finish(s64, inp, act, res, F64), conv3x3.finish(s32, inp, act, res, F32)
                worst[act, res, in_place] = R.conv_ratio(run.run(act, res, in_place)["hi"], ex, p32, dt, act)
    print(f"{R.case_id(c)} {dt}: worst error / bar {max(worst.values()):.3f}")
    assert max(worst.values()) <= 1.0, {k: round(v, 3) for k, v in worst.items() if v > 1.0}


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.STEM_VALUE_CASES, ids=R.stem_id)
def test_stem_values(c, dt):
    inp, ref = R.stem_value_inputs(c, dt), R.stem_ref(c)
    ex, p32 = ref.exact(inp), ref.plain32(inp)
    bar = R.stem_fused.bar(ex, p32, dt) if c.kernel == "stem_fused" else None
    worst = R.conv_ratio(run_stem(c, inp, dt), ex, p32, dt, 1, bar=bar)
    print(f"{R.stem_id(c)} {dt}: worst error / bar {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("C,cv", R.LN2D_CASES)
def test_layernorm2d_channel_padded(C, cv):
    x, w, b, eps = R.ln2d_inputs(C, cv)
    ex, p32 = R.layernorm2d.exact(x, w, b, cv, eps), R.layernorm2d.plain32(x, w, b, cv, eps)
    xd, wd, bd = x.half().cuda(), w.cuda(), b.cuda()
    out = torch.full_like(xd, float("nan"))
    _lib.check(_lib.lib().fvit_layernorm2d_cl(CODE[torch.float16], xd.data_ptr(), out.data_ptr(), wd.data_ptr(), bd.data_ptr(), ctypes.c_float(eps),
                                              R.LN2D_PIXELS, C, cv, stream()), "layernorm2d_cl")
    torch.cuda.synchronize()
    worst = R.worst_ratio(out[:, :cv], ex, p32, torch.float16)
    print(f"layernorm2d_cl C {C} Cv {cv}: worst error / bar {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(out[:, cv:].cpu().float(), torch.zeros(R.LN2D_PIXELS, C - cv))
