"""Every tile form of csrc/fvit_gemm.hip (gemm_kernel 64-row / 128-row / 8 waves / 256 x 256, gemm_pp_kernel with both ring depths, the x3 dual K
loop, split-K with splitk_reduce_kernel, the K-order stagger) through the C ABI on the cases of tests/gemm_refs.py:

  * integer cases: every partial sum is an integer of magnitude <= 256 (two-term output: < 2^15), exact in fp32, fp16 and bf16 in any order, so the
    output must EQUAL the reference (torch.equal on the values); the GELU epilogue must land between the T-roundings of gelu64(y) -+ d;
  * the add-table epilogue (fvit_gemm_residual_add) on the 64-row, 128-row and ping-pong forms;
  * random cases at the rounding level (fused_block_refs.out16_bound / branch_bound with gemm_refs.F_MAX / F_RMS).

Routes are forced with tests.util.tuned and confirmed by the launch name in _lib.prof_records(); operands carry NaN in their pad rows and behind K,
outputs NaN wherever the kernel must not write.  tests/test_gemm_refs_cpu.py holds the CPU side: the exactness conditions and the mutants."""
import contextlib

import pytest
import torch

from fastervit_amd import _lib
from tests import gemm_refs as R
from tests.fused_block_refs import branch_bound, out16_bound
from tests.util import tuned

pytestmark = pytest.mark.gpu
CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}
SPARE = 3            # rows behind the fp32 x


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _launch_names(out):
    _lib.prof_enable(True)
    try:
        yield
        out.extend(r["name"] for r in _lib.prof_records())
    finally:
        _lib.prof_enable(False)


def _isnan(t):
    return bool(torch.isnan(t.float()).all())


def _run(c, inp, dt, epi, wide, *, lo_out=False, gamma=True, add=None, add_idx=None, rpi=0, x0=None, bias=None):
    """One call of the entry point the case needs, on poisoned buffers.  Returns (out or x on the CPU, out_lo_off); the launch name is asserted here."""
    lib = _lib.lib()
    lda, ldw, ldo, lo_off = R.strides(c, wide, epi, lo_out)
    A, W = (t.cuda() for t in R.operands(c, inp, dt, lda, ldw))
    bias = (inp["bias"] / 8 if epi == 1 else inp["bias"]) if bias is None else bias
    bias = bias.cuda()
    gam = inp["gamma"].cuda() if (gamma and epi == 2) else None
    if epi == 2:
        out = torch.full((c.M + SPARE, ldo), R.NAN, dtype=torch.float32)
        out[:c.M, :c.N] = inp["x0"] if x0 is None else x0
    else:
        out = torch.full((R.pad128(c.M), ldo), R.NAN, dtype=dt)
    out = out.cuda()
    names, keep = [], []
    args = (CODE[dt], A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr())
    with _launch_names(names):
        if add is not None:
            add_d, idx_d = add.cuda(), (add_idx.cuda() if add_idx is not None else None)
            keep += [add_d, idx_d]
            rc = lib.fvit_gemm_residual_add(*args, _lib.ptr(gam), out.data_ptr(), ldo, c.M, c.N, c.K, add_d.data_ptr(), _lib.ptr(idx_d), rpi, _stream())
        elif c.route.startswith("sk_"):
            slab = torch.full((8 * c.M * c.N,), R.NAN, dtype=torch.float32, device="cuda")
            keep.append(slab)
            rc = lib.fvit_gemm_residual_splitk(*args, _lib.ptr(gam), out.data_ptr(), ldo, c.M, c.N, c.K, slab.data_ptr(), slab.numel() * 4, _stream())
        elif c.terms == 3 or lo_out:
            rc = lib.fvit_gemm_terms_lo(*args, _lib.ptr(gam), out.data_ptr(), ldo, lo_off, c.M, c.N, c.K, c.ka, epi, _stream())
        elif c.terms == 2:
            rc = lib.fvit_gemm_terms(*args, _lib.ptr(gam), out.data_ptr(), ldo, c.M, c.N, c.K, c.ka, epi, _stream())
        elif epi == 2:
            rc = lib.fvit_gemm_residual(*args, _lib.ptr(gam), out.data_ptr(), ldo, c.M, c.N, c.K, _stream())
        else:
            rc = lib.fvit_gemm_bias_act(*args, out.data_ptr(), ldo, c.M, c.N, c.K, epi, _stream())
        _lib.check(rc, "gemm")
        torch.cuda.synchronize()
    want_name = R.launch_name(c, epi)
    assert names == [want_name], (names, want_name)
    return out.cpu(), lo_off


def _check_equal(got, want, what):
    got = got.double()
    assert torch.equal(got, want), (what, int((got != want).sum()), (got - want).abs().max().item())


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_gemm_integer_case(c, dt):
    inp, inp64 = R.int_inputs(c), R.int_inputs(c, 32)
    M, N = c.M, c.N
    with tuned(**R.ROUTES[c.route][0]):
        for wide in (False, True):
            for epi in R.epilogues(c):
                gamma = not wide                                    # the wide-stride run passes gamma NULL
                out, _ = _run(c, inp, dt, epi, wide, gamma=gamma)
                what = (R.case_id(c), epi, wide)
                assert _isnan(out[M:]) and _isnan(out[:M, N:]), what
                got = out[:M, :N].float()
                if epi == 1:
                    lo, hi = R.gelu_interval(R.accumulate(c, inp) + inp["bias"].double() / 8, dt)
                    bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
                    assert not bad.any(), (what, int(bad.sum()))
                else:
                    _check_equal(got, R.exact(c, inp, epi, gamma=gamma), what)
        if 0 in R.epilogues(c):                                     # two-term output: hi == round_T(y), lo == y - hi, both exact
            out, lo_off = _run(c, inp64, dt, 0, True, lo_out=True)
            what = (R.case_id(c), "two-term")
            assert _isnan(out[M:]) and _isnan(out[:M, N:lo_off]) and _isnan(out[:M, lo_off + N:]), what
            hi, lo = R.two_term(R.exact(c, inp64, 0), dt)
            _check_equal(out[:M, :N].float(), hi, what)
            _check_equal(out[:M, lo_off:lo_off + N].float(), lo, what)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.TWO_TERM_GELU_CASES, ids=R.case_id)
def test_gemm_two_term_gelu_output(c, dt):
    """Epilogue 1 with a two-term output (gelu_erf, fvit_common.h): hi must lie between the T-roundings of gelu64(y) -+ d and lo between those of
    gelu64(y) -+ d - hi, with d = 1.5e-7 + 4 * 2^-24 |gelu64(y)|.  This test found gelu_erf at 1.45 d (y = -3.25; 1.0 .. 1.6 % of the lo terms outside)
    while it stood on the Abramowitz-Stegun erf, whose 1.5e-7 is an absolute ERF error that GELU multiplies by 0.5 |y|; on erfc without cancellation
    the worst |hi + lo - gelu64(y)| is 0.44 d in fp16 (in bf16 hi + lo is 16 bits wide and that figure says nothing: the two intervals are the test)."""
    inp = R.int_inputs(c)
    M, N = c.M, c.N
    with tuned(**R.ROUTES[c.route][0]):
        out, lo_off = _run(c, inp, dt, 1, True, lo_out=True)
    assert _isnan(out[M:]) and _isnan(out[:M, N:lo_off]) and _isnan(out[:M, lo_off + N:])
    ghi, glo = out[:M, :N].float(), out[:M, lo_off:lo_off + N].float()
    y = R.accumulate(c, inp) + inp["bias"].double() / 8
    lo, hi = R.gelu_interval(y, dt, two_term=True)
    gl = R.gelu64(y)
    d = R.GELU_ABS[True] + 4 * 2.0 ** -24 * gl.abs()
    lo2, hi2 = (gl - d - ghi.double()).float().to(dt).float(), (gl + d - ghi.double()).float().to(dt).float()
    bad_hi = (ghi < lo) | (ghi > hi) | ~torch.isfinite(ghi)
    bad_lo = (glo < lo2) | (glo > hi2) | ~torch.isfinite(glo)
    worst = ((ghi.double() + glo.double() - gl).abs() / d).max().item()
    print(f"{R.case_id(c)} {dt} two-term GELU: hi outside {int(bad_hi.sum())}, lo outside {int(bad_lo.sum())} of {M * N}; worst |hi + lo - gelu64| / d = {worst:.3f}")
    assert not bad_hi.any() and not bad_lo.any(), (int(bad_hi.sum()), int(bad_lo.sum()), worst)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.NAN_CASES, ids=R.case_id)
def test_gemm_nan_in_an_operand_comes_back_nan(c, dt):
    """One NaN in a valid element of A: its output row must be NaN in every epilogue -- the GELU epilogue holds its argument at -3 sqrt(2), and a hold that
    drops a NaN operand (fmaxf) would return a finite -2.2e-5 there -- and every other row is held as in the integer cases.  (This test also found the
    fp16 store turning NaN into -65504 in every epilogue: sat16 is a v_med3_f32; the GEMM epilogues now store through sat16_nan.)"""
    inp, m0 = R.nan_inputs(c, R.int_inputs(c))
    M, N = c.M, c.N
    others = torch.arange(M) != m0
    with tuned(**R.ROUTES[c.route][0]):
        for epi, lo_out in ((0, False), (1, False), (2, False), (1, True)):
            out, lo_off = _run(c, inp, dt, epi, True, lo_out=lo_out)
            what = (R.case_id(c), epi, lo_out)
            got = out[:M, :N].float()
            assert _isnan(got[m0]), (what, got[m0][:8])
            if lo_out:
                assert _isnan(out[m0, lo_off:lo_off + N]), what
            if epi == 1:
                lo, hi = R.gelu_interval(R.accumulate(c, inp) + inp["bias"].double() / 8, dt, two_term=lo_out)
                assert ((got >= lo) & (got <= hi))[others].all(), what
            else:
                _check_equal(got[others], R.exact(c, inp, epi)[others], what)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c,rpi,kind", R.ADD_CASES, ids=lambda v: R.case_id(v) if isinstance(v, R.Case) else str(v))
def test_gemm_residual_add_table(c, rpi, kind, dt):
    inp = R.int_inputs(c)
    add, idx = R.add_inputs(c, rpi, kind)
    with tuned(**R.ROUTES[c.route][0]):
        for wide in (False, True):
            out, _ = _run(c, inp, dt, 2, wide, gamma=not wide, add=add, add_idx=idx, rpi=rpi)
            assert _isnan(out[c.M:]) and _isnan(out[:c.M, c.N:])
            _check_equal(out[:c.M, :c.N], R.exact(c, inp, 2, gamma=not wide, add=add, add_idx=idx, rpi=rpi), (R.case_id(c), rpi, kind, wide))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=lambda v: "-".join(map(str, v)))
def test_gemm_random_case_at_the_rounding_level(case, dt):
    route, M, N, K, epi = case
    c = R.Case(route, M, N, K)
    rin = R.random_inputs(case, dt)
    inp = dict(a=[rin["A"]], w=[rin["W"]], bias=rin["bias"], gamma=rin["gamma"], x0=rin["x0"])
    with tuned(**R.ROUTES[route][0]):
        out, _ = _run(c, inp, dt, epi, True, bias=rin["bias"])
    exact, plain = R.random_value(rin, epi), R.random_value(rin, epi, R.F32)
    got = out[:M, :N].double()
    assert torch.isfinite(got).all() and _isnan(out[M:]) and _isnan(out[:M, N:])
    if epi == 0:
        bound, base = out16_bound(exact, plain, dt, R.F_MAX), plain.to(dt).double()
    else:
        got = got - rin["x0"].double()                                # the branch; recovering it costs 2^-23 max(|x0|, |x|), which the bar carries
        bound, base = branch_bound(exact, plain, rin["x0"], R.F_MAX), plain.double()
    err = got - exact
    rmax = (err.abs() / bound).max().item()
    rrms = (err.pow(2).mean().sqrt() / (R.F_RMS * (base - exact).pow(2).mean().sqrt())).item()
    print(f"gemm random {'-'.join(map(str, case))} {dt}: max ratio {rmax:.3f} rms ratio {rrms:.3f}")
    assert rmax <= 1.0 and rrms <= 1.0, (rmax, rrms)
