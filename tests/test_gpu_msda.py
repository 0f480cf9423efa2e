"""Multi-scale deformable attention on the GPU (csrc/fvit_msda.hip through the C ABI, and fastervit_amd/ops.py on top of it), held to float64
(tests/msda_refs.py: the references, the case table and the bar; tests/test_msda_refs_cpu.py shows that ordinary fp32 evaluations meet half that
bar on these very inputs and that seven wrong answers do not meet it).

Conventions: ``value`` is a view inside a larger NaN-filled buffer, every output starts as NaN with a NaN tail behind it that must stay NaN, every
result must be finite.  Each value test prints its worst |err| / bound per tensor; 1.0 is the bar (profiles/msda_tests.log: a run on an MI355X)."""
import copy

import pytest
import torch

from fastervit_amd import _lib, ops
from tests import msda_refs as R

pytestmark = pytest.mark.gpu

CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
PAD = 64      # elements of NaN in front of and behind every buffer
DTS = pytest.mark.parametrize("dt", R.DTYPES, ids=R.DTYPE_IDS)
VALUE_CASES = pytest.mark.parametrize("case_id,far", R.value_case_params(), ids=[f"case{c}{'far' if f else ''}" for c, f in R.value_case_params()])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _embed(t, dt):
    """``t`` as a dense device tensor of type ``dt`` that is a view into the middle of a NaN-filled buffer."""
    buf = torch.full((t.numel() + 2 * PAD,), NAN, dtype=dt, device="cuda")
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t.to(dt))
    return view, buf


def _nan_out(shape, dt):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + PAD,), NAN, dtype=dt, device="cuda")
    return buf[:n].view(shape), buf


def _device_inputs(inp, dt):
    value, _ = _embed(inp["value"], dt)
    return dict(value=value, shapes=inp["shapes"].cuda(), starts=inp["starts"].cuda(), loc=inp["loc"].cuda(), attn=inp["attn"].cuda(),
                grad_out=inp["grad_out"].to(dt).cuda())


def _dims(d):
    N, S, M, D = d["value"].shape
    _, Lq, _, L, P, _ = d["loc"].shape
    return N, S, M, D, Lq, L, P


def _abi(d, dt, dims=None, code=None):
    """Both entry points on NaN outputs; returns (dict of the four tensors, return codes, the whole output buffers)."""
    lib = _lib.lib()
    N, S, M, D, Lq, L, P = dims or _dims(d)
    out, out_buf = _nan_out((d["loc"].shape[0], d["loc"].shape[1], d["value"].shape[2] * d["value"].shape[3]), dt)
    gv, gv_buf = _nan_out(tuple(d["value"].shape), F32)
    gl, gl_buf = _nan_out(tuple(d["loc"].shape), F32)
    ga, ga_buf = _nan_out(tuple(d["attn"].shape), F32)
    code = CODE[dt] if code is None else code
    rc_f = lib.fvit_msda_forward(code, d["value"].data_ptr(), d["shapes"].data_ptr(), d["starts"].data_ptr(), d["loc"].data_ptr(), d["attn"].data_ptr(),
                                 out.data_ptr(), N, S, M, D, Lq, L, P, _stream())
    rc_b = lib.fvit_msda_backward(code, d["value"].data_ptr(), d["shapes"].data_ptr(), d["starts"].data_ptr(), d["loc"].data_ptr(), d["attn"].data_ptr(),
                                  d["grad_out"].data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), N, S, M, D, Lq, L, P, _stream())
    torch.cuda.synchronize()
    return dict(out=out, grad_value=gv, grad_sampling_loc=gl, grad_attn_weight=ga), (rc_f, rc_b), (out_buf, gv_buf, gl_buf, ga_buf)


def _function(d):
    value, loc, attn = (d[k].detach().requires_grad_(True) for k in ("value", "loc", "attn"))      # value stays the view into its NaN buffer
    out = ops.MSDeformAttnFunction.apply(value, d["shapes"], d["starts"], loc, attn, 64)
    out.backward(d["grad_out"])      # the reference's positions: value, None, None, locations, weights, None (autograd checks each shape)
    return dict(out=out.detach(), grad_value=value.grad, grad_sampling_loc=loc.grad, grad_attn_weight=attn.grad)


def _under_bar(name, got, ex, p32, out_dtypes):
    for k in R.TENSORS:
        assert got[k].dtype == out_dtypes[k], (k, got[k].dtype)
        assert torch.isfinite(got[k].float()).all(), f"{name} {k}: a non-finite result"
    worst = R.ratios({k: v.float().reshape(ex[k].shape) for k, v in got.items()}, ex, p32, out_dtypes)
    print(f"{name}: worst |err|/bound " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"{name} {k}: {v:.3f} x the bar"


@DTS
@VALUE_CASES
def test_value_cases_through_the_c_abi(case_id, far, dt):
    inp, ex, p32 = R.references(case_id, dt, far)
    got, rcs, bufs = _abi(_device_inputs(inp, dt), dt)
    assert rcs == (0, 0), _lib.lib().fvit_last_error()
    for buf in bufs:
        assert torch.isnan(buf[-PAD:].float()).all(), "an output was written past its end"
    _under_bar(f"abi case {case_id}{' far' if far else ''} {dt}", got, ex, p32, dict(out=dt, grad_value=F32, grad_sampling_loc=F32, grad_attn_weight=F32))


@DTS
@VALUE_CASES
def test_value_cases_through_the_autograd_function(case_id, far, dt):
    inp, ex, p32 = R.references(case_id, dt, far)
    got = _function(_device_inputs(inp, dt))
    _under_bar(f"function case {case_id}{' far' if far else ''} {dt}", got, ex, p32,
               dict(out=dt, grad_value=dt, grad_sampling_loc=F32, grad_attn_weight=F32))


@DTS
@pytest.mark.parametrize("D", R.EXACT_D)
def test_exact_cases_are_reproduced_exactly(D, dt):
    """Integers and dyadic fractions: every product and partial sum is exact in fp32 in any order, so one mis-addressed corner or level, a wrong
    weight or the other one-sided derivative at an integer coordinate breaks equality."""
    inp, ex = R.exact_references(D, dt)
    d = _device_inputs(inp, dt)
    got, rcs, _ = _abi(d, dt)
    assert rcs == (0, 0), _lib.lib().fvit_last_error()
    fn = _function(d)
    for k in R.TENSORS:
        assert torch.equal(got[k].cpu(), ex[k].reshape(got[k].shape).to(got[k].dtype)), f"abi {k}"
        assert torch.equal(fn[k].cpu(), ex[k].reshape(fn[k].shape).to(fn[k].dtype)), f"function {k}"


@DTS
@pytest.mark.parametrize("case_id", [3, 7])
def test_two_calls_repeat_bitwise_except_grad_value(case_id, dt):
    inp, ex, p32 = R.references(case_id, dt)
    d = _device_inputs(inp, dt)
    a, rcs_a, _ = _abi(d, dt)
    b, rcs_b, _ = _abi(d, dt)
    assert rcs_a == (0, 0) and rcs_b == (0, 0)
    for k in ("out", "grad_sampling_loc", "grad_attn_weight"):
        assert torch.equal(a[k], b[k]), f"{k} differs between two calls"
    for got in (a, b):      # grad_value: float atomics, the last bits depend on arrival order -- held to the bar only
        assert R.worst_ratio(got["grad_value"], ex["grad_value"], p32["grad_value"], F32) <= 1.0


def test_unsupported_calls_are_refused_by_name_before_a_launch():
    lib = _lib.lib()
    inp, _, _ = R.references(1, F32)
    d = _device_inputs(inp, F32)
    N, S, M, D, Lq, L, P = _dims(d)
    for dims, code, word in (((N, S, M, 24, Lq, L, P), None, b"D=24"), ((N, S, M, D, Lq, 9, P), None, b"L=9"), ((N, S, M, D, Lq, L, 17), None, b"P=17"),
                             ((N, S, M, D, Lq, L, P), 3, b"dtype"), ((N, S, M, D, Lq, L, P), 7, b"fp64")):
        got, rcs, bufs = _abi(d, F32, dims=dims, code=code)
        assert rcs == (-1, -1) and word in lib.fvit_last_error(), (rcs, lib.fvit_last_error())
        for buf in bufs:
            assert torch.isnan(buf).all(), f"{word}: something was launched"
    args = (d["value"], d["shapes"], d["starts"], d["loc"], d["attn"])
    with pytest.raises(RuntimeError, match="float64"):
        ops.ms_deform_attn(args[0].double(), *args[1:])
    with pytest.raises(RuntimeError, match="float64"):
        ops.ms_deform_attn(*args[:3], args[3].double(), args[4])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ms_deform_attn(args[0].cpu(), *args[1:])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.MSDeformAttnFunction.apply(*args[:4], args[4].cpu(), 64)
    value24 = torch.zeros(1, S, 2, 24, device="cuda")
    with pytest.raises(RuntimeError, match="D=24"):
        ops.ms_deform_attn(value24, *args[1:])
    loc9 = torch.zeros(1, 2, 2, 9, 2, 2, device="cuda")
    with pytest.raises(RuntimeError, match="L=9"):
        ops.ms_deform_attn(d["value"], torch.ones(9, 2, dtype=torch.int64), torch.zeros(9, dtype=torch.int64), loc9, loc9[..., 0])


def test_forward_is_capturable_and_replays_bitwise():
    inp, ex, p32 = R.references(3, torch.float16)
    d = _device_inputs(inp, torch.float16)
    args = (d["value"], d["shapes"], d["starts"], d["loc"], d["attn"])
    with torch.no_grad():
        eager = ops.ms_deform_attn(*args).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.ms_deform_attn(*args)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = ops.ms_deform_attn(*args)
        for _ in range(3):
            static_out.fill_(NAN)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, eager)
    assert R.worst_ratio(eager.float().reshape(ex["out"].shape), ex["out"], p32["out"], torch.float16) <= 1.0


# ---- the module ------------------------------------------------------------------------------------------------------------------------------
MOD = dict(d_model=256, n_levels=4, n_heads=8, n_points=4)
MOD_LEVELS = R.CASES[3]["levels"]


def _module_and_inputs(ref_dim, seed=11):
    g = R.gen(7200 + seed)
    torch.manual_seed(seed)
    m = ops.MSDeformAttn(**MOD)
    with torch.no_grad():        # the zero-initialised layers would make every query sample alike
        m.sampling_offsets.weight.copy_(torch.randn(m.sampling_offsets.weight.shape, generator=g) * 0.05)
        m.attention_weights.weight.copy_(torch.randn(m.attention_weights.weight.shape, generator=g) * 0.1)
        m.value_proj.bias.copy_(torch.randn(256, generator=g) * 0.1)
    shapes, starts, S = R.level_tensors(MOD_LEVELS)
    N, Lq = 2, 50
    query = torch.randn(N, Lq, 256, generator=g)
    src = torch.randn(N, S, 256, generator=g)
    mask = torch.rand(N, S, generator=g) < 0.1
    centre = torch.rand(N, Lq, 4, 2, generator=g)
    ref = centre if ref_dim == 2 else torch.cat([centre, 0.05 + 0.3 * torch.rand(N, Lq, 4, 2, generator=g)], -1)
    return m, (query, ref, src, shapes, starts, mask)


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_module_forward_against_float64(ref_dim):
    """The core's output (what output_proj receives) under the bar, on the very value / locations / weights the module handed to the kernel; those
    inputs and the final output against a float64 copy of the module, to fp32 Linear-layer rounding."""
    m, inputs = _module_and_inputs(ref_dim)
    m64 = copy.deepcopy(m).double()
    query, ref, src, shapes, starts, mask = inputs
    m = m.cuda()
    seen = {}
    m.output_proj.register_forward_hook(lambda mod, args, out: seen.update(core=args[0].detach()))
    dev = [t.cuda() for t in inputs]
    with torch.no_grad():
        got = m(*dev)
        value, loc, attn = m.sampling_inputs(dev[0], dev[1], dev[2], dev[3], dev[5])
        value64, loc64, attn64 = m64.sampling_inputs(query.double(), ref.double(), src.double(), shapes, mask)
    assert torch.isfinite(got).all() and got.shape == query.shape
    for name, a, b in (("value", value, value64), ("locations", loc, loc64), ("weights", attn, attn64)):
        err = (a.cpu().double() - b).abs().max().item()
        print(f"module ref{ref_dim} {name}: max |fp32 - float64| = {err:.1e}")
        assert err <= 1e-4 * max(1.0, b.abs().max().item())          # K = 256 fp32 dot products
    assert mask.any() and not value.cpu()[mask].any()                # padded positions carry zero values
    kernel_inputs = dict(value=value.cpu(), shapes=shapes, starts=starts, loc=loc.float().cpu(), attn=attn.float().cpu(),
                         grad_out=torch.zeros(got.shape))
    ex, p32 = R.exact(kernel_inputs), R.plain32(kernel_inputs)
    ratio = R.worst_ratio(seen["core"].float(), ex["out"], p32["out"], F32)
    print(f"module ref{ref_dim} core output: worst |err|/bound = {ratio:.3f}")
    assert ratio <= 1.0
    with torch.no_grad():
        want = m64.output_proj(R.forward(value64, shapes, starts, loc64, attn64, F64))
    assert (got.cpu().double() - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())


def test_module_passes_a_16_bit_value_to_the_kernel_under_autocast():
    m, inputs = _module_and_inputs(2)
    m = m.cuda()
    seen = {}
    m.output_proj.register_forward_hook(lambda mod, args, out: seen.update(core=args[0].detach()))
    dev = [t.cuda() for t in inputs]
    with torch.no_grad():
        full = m(*dev)
        with torch.autocast("cuda", dtype=torch.float16):
            half = m(*dev)
    assert seen["core"].dtype == torch.float16 and torch.isfinite(half).all()
    assert (half.float() - full).abs().max().item() <= 2e-2 * full.abs().max().item()     # fp16 Linear layers around an fp16 gather


def test_module_trains_eight_sgd_steps_reduce_the_loss():
    m, inputs = _module_and_inputs(4)
    teacher, _ = _module_and_inputs(4, seed=12)
    m, teacher = m.cuda(), teacher.cuda()
    dev = [t.cuda() for t in inputs]
    with torch.no_grad():
        target = teacher(*dev)
    opt = torch.optim.SGD(m.parameters(), lr=2e-3)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = (m(*dev) - target).square().sum(-1).mean()
        loss.backward()
        for name, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert m.sampling_offsets.weight.grad.abs().max() > 0 and m.attention_weights.weight.grad.abs().max() > 0
        opt.step()
        losses.append(loss.item())
    print("module SGD losses: " + " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0]
