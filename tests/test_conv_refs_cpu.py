"""The references, inputs and bar of tests/conv_refs.py checked on the CPU, over the case tables the GPU tests run (tests/test_gpu_conv_exact.py,
tests/test_gpu_conv_values.py): the float32 evaluations sit inside the bar, ``exact`` agrees with an independently written statement, every integer case
is exactly representable, G and F are what the module says, and every reference mutant is caught -- the integer mutants by equality on the integer
cases, the value mutants by at least 2.5 x the value bar."""
import math

import pytest
import torch

from tests import conv_refs as R
from tests.conv_refs import F32, F64, conv3x3, stem_fused

EPILOGUES = [(act, res) for act in (0, 1, 2) for res in (False, True)]
CATCH = 2.5


def _out_dtype(c, dt):
    return dt if c.out == "16" else F32          # two planes (hi + lo) and fp32 maps: no 16-bit rounding of the value, u_T = 0


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.VALUE_CASES + R.PX_VALUE_CASES, ids=R.case_id)
def test_float32_evaluations_are_inside_the_bar(c, dt):
    inp, ot = R.value_inputs(c, dt), _out_dtype(c, dt)
    s64, s32, sc32 = conv3x3.presum(inp, F64), conv3x3.presum(inp, F32), conv3x3.presum(inp, F32, R.conv_chunk)
    for act, res in EPILOGUES:
        ex, p32, c32 = (conv3x3.finish(s, inp, act, res, s.dtype) for s in (s64, s32, sc32))
        fast = c.out == "16" and not c.in_lo
        rp, rc = (R.conv_ratio(t.to(ot), ex, p32, ot, act, fast) for t in (p32, c32))
        assert rp <= 1.0 and rc <= (1.0 if R.U_T[ot] else 0.5), (act, res, rp, rc)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.STEM_VALUE_CASES, ids=R.stem_id)
def test_stem_evaluations_are_inside_the_bar(c, dt):
    inp = R.stem_value_inputs(c, dt)
    if c.kernel != "stem_fused":
        ex, p32, c32 = R.stem_conv.exact(inp), R.stem_conv.plain32(inp), R.stem_conv.chunk32(inp)
        assert R.conv_ratio(p32.to(dt), ex, p32, dt) <= 1.0 and R.conv_ratio(c32.to(dt), ex, p32, dt) <= 1.0
        return
    ex, p32 = stem_fused.exact(inp), stem_fused.plain32(inp)
    bar = stem_fused.bar(ex, p32, dt)
    for name, fn in dict(R.STEM_VARIANTS, plain32=stem_fused.plain32).items():
        assert R.conv_ratio(fn(inp).to(dt), ex, p32, dt, bar=bar) <= 1.0, name


def test_stem_f_is_twice_the_worst_variant_ratio():
    worst = {}
    for dt in R.OPERAND_DTYPES:
        for c in R.STEM_VALUE_CASES:
            if c.kernel == "stem_fused":
                inp = R.stem_value_inputs(c, dt)
                ex = stem_fused.exact(inp)
                e16 = (stem_fused.plain32(inp).to(F64) - ex).abs().max().item()
                for name, fn in R.STEM_VARIANTS.items():
                    worst[name] = max(worst.get(name, 0.0), (fn(inp).to(F64) - ex).abs().max().item() / e16)
    print("stem_fused variant error / e16, worst over the cases:", {k: round(v, 3) for k, v in worst.items()})
    assert 2.0 * max(worst.values()) <= R.STEM_F <= 4.0


@pytest.mark.parametrize("c", [c for c in R.VALUE_CASES + R.PX_VALUE_CASES if c.Ci <= 128], ids=R.case_id)
def test_exact_is_nine_shifted_matmuls(c):
    inp = R.value_inputs(c, torch.float16)
    a, b = conv3x3.presum(inp, F64), conv3x3.presum(inp, F64, R.conv_shifted)
    assert (a - b).abs().max().item() <= 1e-11 * a.abs().max().item()


@pytest.mark.parametrize("c", R.CONV_CASES, ids=R.case_id)
def test_integer_cases_are_exact_in_every_type(c):
    inp = R.int_inputs(c)                                    # asserts the <= 256 condition
    s64, s32, sc32 = conv3x3.presum(inp, F64), conv3x3.presum(inp, F32), conv3x3.presum(inp, F32, R.conv_chunk)
    for act in (0, 1):
        for res in (False, "hi", True):
            ex, p32, c32 = (conv3x3.finish(s, inp, act, res, s.dtype) for s in (s64, s32, sc32))
            assert torch.equal(p32.to(F64), ex) and torch.equal(c32.to(F64), ex)
            for dt in R.OPERAND_DTYPES:
                assert torch.equal(ex.to(dt).to(F64), ex)


@pytest.mark.parametrize("c", R.STEM_CONV_CASES + R.STEM_FUSED_CASES, ids=R.stem_id)
def test_integer_stem_cases_are_exact_in_every_type(c):
    inp, ref = R.stem_int_inputs(c), R.stem_ref(c)
    ex = ref.exact(inp)
    assert torch.equal(ref.plain32(inp).to(F64), ex)
    for dt in R.OPERAND_DTYPES:
        assert torch.equal(ex.to(dt).to(F64), ex)


def test_gelu_fast_error():
    g = R.gelu_fast_error()
    print(f"G = {g:.3e}")
    assert 1e-5 < g <= R.GELU_DOCUMENTED


def test_layernorm2d_reference():
    for C, cv in R.LN2D_CASES:
        x, w, b, eps = R.ln2d_inputs(C, cv)
        ex, p32 = R.layernorm2d.exact(x, w, b, cv, eps), R.layernorm2d.plain32(x, w, b, cv, eps)
        assert torch.equal(ex[0], b[:cv].to(F64)) and R.worst_ratio(p32.half(), ex, p32, torch.float16) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# mutants of the reference
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _drop_channel_on_last_output(inp):
    """One (channel, output channel) product left out on the last output channel: the ragged N tile of Cout = 192."""
    out = conv3x3.presum(inp, F64)
    for ci in range(inp.cv):                                 # the first channel whose product with that output channel is not zero everywhere
        part = R.conv_plain(inp.x[..., ci:ci + 1], inp.w[0][-1:, ci:ci + 1], inp.stride, F64)[..., 0]
        if part.abs().sum() > 0:
            break
    out[..., -1] -= part
    return conv3x3.finish(out, inp, 0, False, F64)


INT_MUTANTS = {
    "one tap dropped at a corner pixel": (lambda c: True, lambda inp: conv3x3.exact(inp, conv=R.conv_shifted, conv_opt=dict(drop_tap_at_corner=True))),
    "one channel dropped on the ragged N tile": (lambda c: c.Co == 192, _drop_channel_on_last_output),
    "tap (ky, kx) transposed": (lambda c: (c.H, c.W) != (1, 1), lambda inp: conv3x3.exact(inp, conv=R.conv_shifted, conv_opt=dict(transpose_taps=True))),
    "H and W swapped in the border mask": (lambda c: c.H != c.W, lambda inp: conv3x3.exact(inp, conv=R.conv_shifted, conv_opt=dict(swap_mask=True))),
}


@pytest.mark.parametrize("name", INT_MUTANTS)
def test_integer_mutants_break_equality(name):
    applies, mutant = INT_MUTANTS[name]
    cases = [c for c in R.CONV_CASES if applies(c) and c.Ci <= 128]
    assert len(cases) >= 10
    for c in cases:
        inp = R.int_inputs(c)
        assert not torch.equal(mutant(inp), conv3x3.exact(inp)), R.case_id(c)


def _bad_gelu(t):
    return R.gelu_fast64(t, R.GELU_FAST_Q[:-1] + (R.GELU_FAST_Q[-1] + 1e-3,))


# name: (the cases it applies to, act, residual, the mutated exact)
VALUE_MUTANTS = {
    "stride-2 sampling offset by one": (lambda c: c.stride == 2, 0, False, dict(conv=R.conv_shifted, conv_opt=dict(offset=1))),
    "lo weight image skipped for the last 64 columns": (lambda c: c.terms == 2, 0, False, dict(skip_lo_cols=64)),
    "residual added before the activation": (lambda c: True, 1, True, dict(res_first=True)),
    "bias on the wrong side of the ReLU": (lambda c: True, 1, False, dict(bias_after_act=True)),
    "one GELU coefficient off by 1e-3": (lambda c: True, 2, False, dict(gelu=_bad_gelu)),
}


@pytest.mark.parametrize("name", VALUE_MUTANTS)
def test_value_mutants_exceed_the_bar(name):
    applies, act, res, mut = VALUE_MUTANTS[name]
    worst = 0.0
    for c in [c for c in R.VALUE_CASES if applies(c) and c.Ci <= 128][:8]:
        for dt in R.OPERAND_DTYPES:
            inp = R.value_inputs(c, dt)
            ex, p32 = conv3x3.exact(inp, act, res), conv3x3.plain32(inp, act, res)
            worst = max(worst, R.conv_ratio(conv3x3.exact(inp, act, res, **mut).to(dt), ex, p32, dt, act))
    print(f"{name}: {worst:.1f} x the bar")
    assert worst >= CATCH


def test_unrounded_stem_intermediate_exceeds_the_bar():
    worst = 0.0
    for c in [c for c in R.STEM_VALUE_CASES if c.kernel == "stem_fused"]:
        for dt in R.OPERAND_DTYPES:
            inp = R.stem_value_inputs(c, dt)
            ex, p32 = stem_fused.exact(inp), stem_fused.plain32(inp)
            worst = max(worst, R.conv_ratio(stem_fused.exact(inp, narrow=False).to(dt), ex, p32, dt, bar=stem_fused.bar(ex, p32, dt)))
    print(f"stem_fused's intermediate not rounded: {worst:.1f} x the bar")
    assert worst >= CATCH and math.isfinite(worst)
