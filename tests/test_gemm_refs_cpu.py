"""The CPU side of tests/test_gpu_gemm_exact.py (no GPU): the conditions under which the integer cases of tests/gemm_refs.py are exact in every
summation order, the teeth of those cases (each reference mutant changes at least one output of every case it applies to), and the F study behind
the rounding-level bar of the random cases.

Mutants (gemm_refs.accumulate / exact):
    drop_ktile           one 16 x 16 fragment misses one K tile
    a_col_wrong_term     the second term reads A column k instead of k - ka (x3 rows: the lo image)
    skip_last_colgroup   the last 16-column group is never stored
    pad_row_leak         a pad row of A (NaN in the buffers, zero here) stands in for the last valid row
    gamma_not_on_bias    gamma scales the accumulator but not the bias
    drop_lo_hi           the a_lo . w_hi product of K = 3 ka is dropped
    add_row_of_m         the add table is indexed by m instead of m % rows_per_image
    nan_dropped          the GELU epilogue holds its argument at XMIN with a maximum that drops a NaN operand (fmaxf): the NaN row comes back finite"""
import math

import pytest
import torch

from tests import gemm_refs as R
from tests.fused_block_refs import out16_bound, branch_bound, variant_ratios


@pytest.mark.parametrize("c", R.CASES + [a[0] for a in R.ADD_CASES], ids=R.case_id)
def test_integer_cases_are_exact_in_any_order(c):
    inp = R.int_inputs(c)
    for img in inp["a"]:
        assert set(img.unique().tolist()) <= {-1.0, 0.0, 1.0}
        nz = (img.view(c.M, -1, 64) != 0).sum(-1)
        assert nz.min().item() >= 4 and nz.max().item() <= max(4, 112 // c.nk)
    assert all(w.abs().max().item() <= 2 and (w == w.round()).all() for w in inp["w"])
    assert R.magnitude(c, inp, inp["bias"]) <= 256
    assert R.dead_blocks(c, inp) == 0
    # the GELU epilogue shares only the exact pre-activation: multiples of 1/8 of magnitude <= 256
    y = R.accumulate(c, inp) + inp["bias"].double() / 8
    assert (y * 8 == (y * 8).round()).all() and y.abs().max().item() <= 256
    # x0 + gamma * y: multiples of 1/2 below 2^10, exact in fp32
    x = R.exact(c, inp, 2)
    assert (x.float().double() == x).all() and x.abs().max().item() < 1024


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_two_term_output_is_exact(c, dt):
    inp = R.int_inputs(c, 32)
    assert max(w.abs().max().item() for w in inp["w"]) == 64
    assert 1000 < R.magnitude(c, inp, inp["bias"]) < 2 ** 15
    y = R.exact(c, inp, 0)
    hi, lo = R.two_term(y, dt)
    assert (lo.float().to(dt).double() == lo).all() and (hi + lo == y).all()
    bits = 11 if dt == torch.float16 else 8
    odd_beyond = (y.abs() >= 2 ** bits) & (y % 2 == 1)
    assert (lo != 0).any() or not odd_beyond.any()                # the lo image is zero only where no y needs it
    if dt == torch.bfloat16:
        assert (lo != 0).any()


def _differs(a, b):
    return not torch.equal(torch.nan_to_num(a, nan=1e30), torch.nan_to_num(b, nan=1e30))


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_mutants_change_an_output(c):
    inp = R.int_inputs(c)
    muts = ["drop_ktile", "skip_last_colgroup", "gamma_not_on_bias"] + (["pad_row_leak"] if c.M % 128 else []) + \
           (["a_col_wrong_term", "drop_lo_hi"] if c.terms == 3 else [])
    only = {"skip_last_colgroup": (0,), "gamma_not_on_bias": (2,)}
    for mut in muts:
        for epi in only.get(mut, (0, 1, 2)):
            want, bad = R.exact(c, inp, epi), R.exact(c, inp, epi, mut=mut)
            if epi == 1:      # the mutant's pre-activation differs somewhere by an integer: outside the interval of the true value for some output
                lo, hi = R.gelu_interval(R.accumulate(c, inp) + inp["bias"].double() / 8, torch.float16)
                badv = bad.float().half().float()
                assert ((badv < lo) | (badv > hi)).any(), (mut, epi)
            else:
                assert _differs(want, bad), (mut, epi)


@pytest.mark.parametrize("c,rpi,kind", R.ADD_CASES, ids=lambda v: R.case_id(v) if isinstance(v, R.Case) else str(v))
def test_add_table_cases(c, rpi, kind):
    inp = R.int_inputs(c)
    add, idx = R.add_inputs(c, rpi, kind)
    assert c.M % rpi != 0 and (add == add.round()).all()
    if idx is not None:
        assert (idx < 0).any() and (idx >= 0).any()
    want = R.exact(c, inp, 2, add=add, add_idx=idx, rpi=rpi)
    assert (want.float().double() == want).all()
    assert _differs(want, R.exact(c, inp, 2))                                                   # the table adds something
    assert _differs(want, R.exact(c, inp, 2, add=add, add_idx=idx, rpi=rpi, mut="add_row_of_m"))
    if idx is not None:
        assert _differs(want, R.exact(c, inp, 2, add=add, add_idx=None, rpi=rpi))             # ... through add_idx


def test_gelu_interval_holds_the_rounded_value():
    y = torch.arange(-2048, 2049).double() / 8
    for dt in R.OPERAND_DTYPES:
        for tt in (False, True):
            lo, hi = R.gelu_interval(y, dt, tt)
            mid = R.gelu64(y).float().to(dt).float()
            assert (lo <= mid).all() and (mid <= hi).all()
            # far from zero the interval is one value of T (or two neighbours): a wrong pre-activation cannot hide in it
            assert ((hi - lo) <= 2.02 * 5.4e-5 + torch.maximum(hi.abs(), lo.abs()) * 2.0 ** -6).all()


def test_f_study_of_the_random_cases(capsys):
    """F_max / F_rms of gemm_refs: twice the worst kblock16 / kblock32 ratio plus 2 %, rounded up to one decimal; F_max <= 4."""
    worst = {}
    e16s = []
    for case in R.RANDOM_CASES:
        for dt in R.OPERAND_DTYPES:
            for seed in R.STUDY_SEEDS:
                inp = R.random_inputs(case, dt, seed)
                ex, plain = R.random_value(inp, case[4]), R.random_value(inp, case[4], R.F32)
                e16s.append((plain.double() - ex).abs().max().item())
                for name, kb in (("kblock16", 16), ("kblock32", 32)):
                    rm, rr = variant_ratios(ex, plain, R.random_value(inp, case[4], R.F32, kb))
                    w = worst.setdefault(name, [0.0, 0.0])
                    w[0], w[1] = max(w[0], rm), max(w[1], rr)
                # the base itself passes the bar it defines, with room
                b = out16_bound(ex, plain, dt, R.F_MAX) if case[4] == 0 else branch_bound(ex, plain, inp["x0"], R.F_MAX)
                assert ((plain.double() - ex).abs() <= b).all()
    need_max = math.ceil((2 * max(w[0] for w in worst.values()) * 1.02) * 10 - 1e-9) / 10
    need_rms = math.ceil((2 * max(w[1] for w in worst.values()) * 1.02) * 10 - 1e-9) / 10
    with capsys.disabled():
        print(f"\ngemm F study: e16 {min(e16s):.2e} .. {max(e16s):.2e}; " + "; ".join(f"{k} max {v[0]:.3f} rms {v[1]:.3f}" for k, v in worst.items()) +
              f" -> needs F_max {need_max} F_rms {need_rms}; module has {R.F_MAX} / {R.F_RMS}")
    # F is the documented rounding-up of the study; on another CPU's matmul the ratios move in the third digit, the 2 % is that room
    assert 2 * max(w[0] for w in worst.values()) <= R.F_MAX <= 4.0 and 2 * max(w[1] for w in worst.values()) <= R.F_RMS <= 4.0


@pytest.mark.parametrize("c", R.NAN_CASES, ids=R.case_id)
def test_nan_case_poisons_exactly_one_row_and_a_nan_dropping_clamp_is_caught(c):
    inp, m0 = R.nan_inputs(c, R.int_inputs(c))
    assert 0 <= m0 < c.M and all((w != 0).all() for w in inp["w"])        # no zero weight: every output of the row meets the NaN
    for epi in (0, 1, 2):
        want = R.exact(c, inp, epi)
        nan = torch.isnan(want)
        assert nan[m0].all() and int(nan.sum()) == c.N
    # the mutant: max(y, XMIN) that returns the other operand for a NaN, then the GELU -- a finite, plausible row
    y = R.accumulate(c, inp) + inp["bias"].double() / 8
    bad = R.gelu64(torch.fmax(y, torch.tensor(R.GELU_FAST_XMIN, dtype=torch.float64)))
    assert torch.isfinite(bad[m0]).all() and (bad[m0].abs() < 1e-4).all()
    keep = R.gelu64(torch.where(y < R.GELU_FAST_XMIN, torch.tensor(R.GELU_FAST_XMIN, dtype=torch.float64), y))   # compare-and-select keeps it
    assert torch.isnan(keep[m0]).all()
