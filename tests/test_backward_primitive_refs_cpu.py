"""The references of tests/backward_primitive_refs.py checked against themselves, without a GPU: for every case of the table that
tests/test_gpu_backward_primitives.py runs on the kernels,

  * ``plain32`` (an ordinary fp32 evaluation), rounded to the output type, lies inside the bar -- so the bar is one the arithmetic can meet on these
    inputs, and a kernel that misses it is wrong rather than unlucky;
  * the written-out formula, evaluated in float64, agrees with float64 autograd -- so the formula the kernels are held to is the gradient."""
import pytest
import torch

from tests import backward_primitive_refs as R

F64 = torch.float64
FORMULA_RTOL = 1e-11      # two float64 evaluations of the same gradient: ~1e-13 relative to the tensor's largest entry on these shapes


def _inside(name, plain, exact, outputs):
    """``outputs``: {tensor name: output dtype}.  Returns the worst ratio per tensor; asserts plain32 rounded to that type is within the bar."""
    worst = {}
    for key, dt in outputs.items():
        got = plain[key].to(dt).to(F64)
        worst[key] = R.worst_ratio(got, exact[key], plain[key], dt)
        assert worst[key] <= 1.0, f"{name} {key}: plain32 rounded to {dt} is {worst[key]:.3f} x the bar"
    print(f"{name}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    return worst


def _agree(name, a, b, keys):
    for key in keys:
        peak = b[key].abs().max().item()
        err = (a[key].to(F64) - b[key].to(F64)).abs().max().item()
        assert err <= FORMULA_RTOL * max(peak, 1e-300), f"{name} {key}: formula vs autograd {err:.3e} (largest entry {peak:.3e})"


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES)
@pytest.mark.parametrize("C", R.SCALE_COLS_C)
@pytest.mark.parametrize("M", R.SCALE_COLS_M)
def test_scale_cols_reference(M, C, dt):
    for with_gamma in (True, False):
        dy, z, gamma = R.scale_cols_inputs(M, C, dt, with_gamma)
        exact, plain = R.scale_cols.exact(dy, z, gamma), R.scale_cols.plain32(dy, z, gamma)
        _inside(f"scale_cols M={M} C={C} {dt} gamma={with_gamma}", plain, exact,
                dict(dz=dt, part=torch.float32, dgamma=torch.float32, dbias=torch.float32))
        _agree("scale_cols", exact, R.scale_cols.autograd(dy, z, gamma), ("dz", "dgamma", "dbias"))
        assert exact["part"].shape == ((M + 63) // 64, 2, C)
        _agree("scale_cols part", dict(dgamma=exact["part"][:, 0].sum(0), dbias=exact["part"][:, 1].sum(0)), exact, ("dgamma", "dbias"))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES)
@pytest.mark.parametrize("H", R.GELU_H)
@pytest.mark.parametrize("M", R.GELU_M)
def test_gelu_references(M, H, dt):
    a, dh = R.gelu_inputs(M, H, dt)
    assert a[0, :9].tolist() == R.rounded(torch.tensor(R.GELU_EDGES), dt).tolist()
    exact, plain = R.gelu_fwd.exact(a), R.gelu_fwd.plain32(a)
    _inside(f"gelu M={M} H={H} {dt}", plain, exact, dict(out=dt))
    _agree("gelu", exact, R.gelu_fwd.autograd(a), ("out",))
    exact, plain = R.gelu_bwd.exact(a, dh), R.gelu_bwd.plain32(a, dh)
    _inside(f"gelu' M={M} H={H} {dt}", plain, exact, dict(out=dt, part=torch.float32, dbias=torch.float32))
    _agree("gelu'", R.gelu_bwd.formula(a, dh, F64), exact, ("out", "part", "dbias"))


@pytest.mark.parametrize("with_dy", [True, False])
@pytest.mark.parametrize("M,C", R.LAYERNORM_SHAPES)
def test_layernorm_reference(M, C, with_dy):
    x, dxn, dy, w, eps = R.layernorm_inputs(M, C)
    dy = dy if with_dy else None
    assert x[0].var(unbiased=False).item() == 0.0
    exact, plain = R.layernorm.exact(x, dxn, dy, w, eps), R.layernorm.plain32(x, dxn, dy, w, eps)
    assert exact["stats"][0, 1].item() == pytest.approx(eps ** -0.5, rel=1e-14)
    _inside(f"layernorm M={M} C={C} dy={with_dy}", plain, exact, {k: torch.float32 for k in ("dx", "stats", "part", "dw", "db")})
    formula = R.layernorm.formula(x, dxn, dy, w, eps, F64)
    _agree("layernorm", formula, exact, ("dx", "dw", "db"))
    _agree("layernorm part", dict(dw=formula["part"][:, 0].sum(0), db=formula["part"][:, 1].sum(0)), exact, ("dw", "db"))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES)
@pytest.mark.parametrize("N", R.COLSUM16_N)
@pytest.mark.parametrize("M", R.COLSUM16_M)
def test_colsum16_reference(M, N, dt):
    t = R.colsum16_inputs(M, N, dt)
    exact, plain = R.colsum16.exact(t), R.colsum16.plain32(t)
    _inside(f"colsum16 M={M} N={N} {dt}", plain, exact, dict(part=torch.float32, total=torch.float32))
    _agree("colsum16", exact, R.colsum16.autograd(t), ("total",))
    _agree("colsum16 part", dict(total=exact["part"].sum(0)), exact, ("total",))


@pytest.mark.parametrize("n", R.FINISH_N)
@pytest.mark.parametrize("blocks", R.FINISH_BLOCKS)
def test_colsum_finish_reference(blocks, n):
    part, out0 = R.finish_inputs(blocks, n)
    for base in (None, out0):
        exact, plain = R.colsum_finish.exact(part, base), R.colsum_finish.plain32(part, base)
        _inside(f"colsum_finish blocks={blocks} n={n} accumulate={base is not None}", plain, exact, dict(out=torch.float32))
        want = part.to(F64).sum(0) + (base.to(F64) if base is not None else 0.0)
        _agree("colsum_finish", exact, dict(out=want), ("out",))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES)
@pytest.mark.parametrize("variant", R.ATTENTION_VARIANTS)
@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=lambda c: "x".join(map(str, c)))
def test_attention_reference(case, variant, dt):
    q, k, v, do, scale, bias, mask = R.attention_inputs(case, dt, variant)
    assert (bias is None) == (variant == "nobias") and (mask is None) == (variant != "bias_drop")
    if mask is not None:
        assert set(mask.unique().tolist()) <= {0.0, 1.25} and torch.equal(R.rounded(mask, dt), mask)
    exact, plain = R.attention.exact(q, k, v, do, scale, bias, mask), R.attention.plain32(q, k, v, do, scale, bias, mask)
    _inside(f"attention {case} {variant} {dt}", plain, exact, dict(dq=dt, dk=dt, dv=dt, ds=torch.float32))
    _agree("attention", R.attention.formula(q, k, v, do, scale, bias, mask, F64), exact, ("dq", "dk", "dv", "ds"))
    if tuple(case) == R.ONE_HOT_CASE and bias is not None:      # the near one-hot head: its gradients sit far below the other head's
        assert exact["dq"][:, 1].abs().max().item() < 1e-9 * exact["dq"][:, 0].abs().max().item()


@pytest.mark.parametrize("case", R.ATTENTION_FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_attention_forward_cases_cover_every_head_padding(case):
    nwin, S, heads, d, D = case
    assert {c[4] for c in R.ATTENTION_FWD_CASES} == {32, 64, 96} and {c[1] for c in R.ATTENTION_FWD_CASES} == {1, 13, 49, 53, 64}
    q, k, v, _, scale, bias, mask = R.attention_inputs(case, torch.float16, "bias_drop", forward=True)
    ref = R.attention.forward(q, k, v, scale, bias, mask, F64)
    assert ref.shape == (nwin, heads, S, d) and torch.isfinite(ref).all()
    assert (ref - R.attention.forward(q, k, v, scale, bias, mask, torch.float32)).abs().max().item() < 1e-5 * max(ref.abs().max().item(), 1.0)
