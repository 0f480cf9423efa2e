"""References, inputs and the case table of multi-scale deformable attention (csrc/fvit_msda.hip, fastervit_amd/ops.py), shared by
tests/test_msda_refs_cpu.py (no GPU: the proof that the bar and the inputs are fair), tests/test_gpu_msda.py (the kernels) and
tests/golden/make_msda_golden.py (the reference's own ms_deform_attn_core_pytorch on the same inputs).  Plain PyTorch on the CPU, nothing else.

    out[n, q, m, :] = sum_l sum_p  w[n, q, m, l, p] * bilinear(value_l[n, :, m, :], loc[n, q, m, l, p])

``evaluate`` is the written-out form: pixel coordinate x = loc_x W - 0.5, y = loc_y H - 0.5, floor, the four corners, a floating-point bounds mask per
corner (zero padding), weights (1 - lx)(1 - ly) ...; torch.autograd supplies the three gradients (floor is piecewise constant, so the gradient in a
location is the one-sided derivative towards +1 at an integer coordinate).  ``exact`` is its float64 evaluation, ``plain32`` the fp32 one, both on the
inputs the kernel gets (a 16-bit value already rounded, fp32 locations and weights).  The bar is ``bound`` / ``worst_ratio`` of
tests/backward_primitive_refs.py, per output tensor.  ``VARIANTS`` are other legitimate fp32 evaluations (they must stay far under the bar), ``MUTANTS``
wrong answers (each must exceed it somewhere and break equality on the exact cases)."""
import torch

from tests.backward_primitive_refs import F32, F64, bound, gen, rounded, worst_ratio  # noqa: F401  (re-exported: the one bar)

TENSORS = ("out", "grad_value", "grad_sampling_loc", "grad_attn_weight")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DTYPE_IDS = ["f32", "f16", "bf16"]

# the smallest shapes with a tail in every split of the kernels (lanes per item, items per wave, waves per block)
CASES = {
    1: dict(N=1, M=2, D=16, Lq=2, levels=[(6, 4), (3, 2)], P=2),                          # the reference's own test shape
    2: dict(N=2, M=3, D=32, Lq=37, levels=[(7, 5), (4, 3), (2, 2), (1, 1)], P=4),         # odd heads, a 1x1 level, a ragged last wave
    3: dict(N=1, M=8, D=32, Lq=100, levels=[(13, 21), (7, 11), (4, 6), (2, 3)], P=4),     # the DINO geometry, shrunk
    4: dict(N=2, M=1, D=64, Lq=5, levels=[(1, 9), (5, 1)], P=3),                          # one-row and one-column maps, odd P
    5: dict(N=1, M=2, D=128, Lq=3, levels=[(3, 3)], P=1),                                 # L = 1, P = 1
    6: dict(N=1, M=2, D=32, Lq=9, levels=[(6, 5), (5, 4), (4, 3), (3, 3), (2, 2)], P=2),  # L = 5
    7: dict(N=1, M=1, D=32, Lq=300, levels=[(4, 4)], P=1, same_location=True),            # 300 adders per grad_value row
}
FAR_CASE, FAR_COUNT, FAR = 3, 8, 1e9      # case 3 also runs with eight of its locations at +-1e9
GOLDEN_CASES = (1, 2, 4)
EXACT_LEVELS, EXACT_P, EXACT_D = [(8, 4), (2, 2), (1, 1)], 2, (16, 32)
FRAC_LO, FRAC_HI, MARGIN = 0.07, 0.93, 0.05


def level_tensors(levels):
    shapes = torch.tensor(levels, dtype=torch.int64)
    sizes = shapes[:, 0] * shapes[:, 1]
    return shapes, torch.cat([sizes.new_zeros(1), sizes.cumsum(0)[:-1]]), int(sizes.sum())


def _locations(g, lead, levels, P, fracs=None):
    """(*lead, L, P, 2) fp32: per axis loc = (cell + frac + 0.5) / n, cell uniform in -2 .. n (fully outside, partly outside, inside), frac in
    [FRAC_LO, FRAC_HI] or drawn from ``fracs``."""
    per_level = []
    for H, W in levels:
        axes = []
        for n in (W, H):                                                    # (x, y)
            cell = torch.randint(-2, n + 1, (*lead, P), generator=g).to(F64)
            if fracs is None:
                frac = FRAC_LO + (FRAC_HI - FRAC_LO) * torch.rand(*lead, P, generator=g, dtype=F64)
            else:
                frac = torch.tensor(fracs, dtype=F64)[torch.randint(0, len(fracs), (*lead, P), generator=g)]
            axes.append((cell + frac + 0.5) / n)
        per_level.append(torch.stack(axes, -1))
    return torch.stack(per_level, -3).to(F32)


def make_inputs(case_id, dt, far=False):
    """dict(value, shapes, starts, loc, attn, grad_out), CPU; value and grad_out fp32 holding values of ``dt``, loc and attn fp32."""
    c = CASES[case_id]
    N, M, D, Lq, P, levels = c["N"], c["M"], c["D"], c["Lq"], c["P"], c["levels"]
    L = len(levels)
    shapes, starts, S = level_tensors(levels)
    g = gen(7000 + case_id)
    value = rounded(torch.randn(N, S, M, D, generator=g), dt)
    grad_out = rounded(torch.randn(N, Lq, M * D, generator=g), dt)
    attn = torch.randn(N, Lq, M, L * P, generator=g).softmax(-1).view(N, Lq, M, L, P)
    if c.get("same_location"):
        loc = torch.empty(N, Lq, M, L, P, 2)
        loc[..., 0] = (1 + 0.5 + 0.5) / levels[0][1]                         # pixel (1.5, 2.3): four corners inside, every query adds to the same four rows
        loc[..., 1] = (2 + 0.3 + 0.5) / levels[0][0]
    else:
        loc = _locations(g, (N, Lq, M), levels, P)
    if far:
        flat = loc.view(-1, 2)
        idx = torch.randperm(flat.shape[0], generator=g)[:FAR_COUNT]
        for j, i in enumerate(idx.tolist()):                                  # +1e9 and -1e9 in turn: three in x, three in y, two in both
            far_value = FAR if j % 2 == 0 else -FAR
            if j < 3:
                flat[i, 0] = far_value
            elif j < 6:
                flat[i, 1] = far_value
            else:
                flat[i] = far_value
    return dict(value=value, shapes=shapes, starts=starts, loc=loc, attn=attn, grad_out=grad_out)


def make_exact_inputs(D, dt):
    """Small integers and dyadic fractions: every location, coordinate, bilinear weight, product and partial sum is exact in fp32 in any order."""
    N, M, Lq, P, levels = 2, 2, 21, EXACT_P, EXACT_LEVELS
    L = len(levels)
    shapes, starts, S = level_tensors(levels)
    g = gen(7100 + D)
    value = torch.randint(-4, 5, (N, S, M, D), generator=g).to(F32)
    grad_out = torch.randint(-4, 5, (N, Lq, M * D), generator=g).to(F32)
    attn = torch.randint(0, 3, (N, Lq, M, L, P), generator=g).to(F32) / 8.0   # multiples of 1/8, at most 6 * 2/8 <= 2 per head
    loc = _locations(g, (N, Lq, M), levels, P, fracs=[0.0, 0.25, 0.5, 0.75])
    assert rounded(value, dt).equal(value) and rounded(grad_out, dt).equal(grad_out)
    return dict(value=value, shapes=shapes, starts=starts, loc=loc, attn=attn, grad_out=grad_out)


def fraction_margin(inp):
    """The smallest distance of any pixel coordinate's fractional part from 0 or 1, in float64 on the fp32 locations the kernel receives."""
    worst = 1.0
    for l, (H, W) in enumerate(inp["shapes"].tolist()):
        for axis, n in ((0, W), (1, H)):
            pix = inp["loc"][..., l, :, axis].to(F64) * n - 0.5
            frac = pix - pix.floor()
            worst = min(worst, frac.min().item(), (1.0 - frac).min().item())
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("corners_reversed", "coordinate_2n", "levels_reversed")
MUTANTS = ("align_corners", "xy_swapped", "hw_swapped_in_row", "border_clamp", "weight_of_next_point", "start_of_next_level", "mask_dropped_on_one_corner")


def forward(value, shapes, starts, loc, attn, dt, how=None):
    """The written-out op in dtype ``dt`` (differentiable in value, loc, attn); ``how`` = one of VARIANTS / MUTANTS or None."""
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    value, loc, attn = value.to(dt), loc.to(dt), attn.to(dt)
    n_idx = torch.arange(N).view(N, 1, 1, 1)
    m_idx = torch.arange(M).view(1, 1, M, 1)
    out = torch.zeros(N, Lq, M, D, dtype=dt)
    corners = [(0, 0), (0, 1), (1, 0), (1, 1)]                               # (dy, dx)
    if how == "corners_reversed":
        corners = corners[::-1]
    for l in (range(L - 1, -1, -1) if how == "levels_reversed" else range(L)):
        H, W = (int(v) for v in shapes[l])
        start = int(starts[(l + 1) % L] if how == "start_of_next_level" else starts[l])
        lx_, ly_ = loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1]              # (N, Lq, M, P)
        if how == "xy_swapped":
            lx_, ly_ = ly_, lx_
        if how == "align_corners":
            x, y = lx_ * (W - 1), ly_ * (H - 1)
        elif how == "coordinate_2n":
            x, y = (2 * lx_ * W - 1) / 2, (2 * ly_ * H - 1) / 2
        else:
            x, y = lx_ * W - 0.5, ly_ * H - 0.5
        x0, y0 = x.detach().floor(), y.detach().floor()
        lx, ly = x - x0, y - y0
        w_l = attn[:, :, :, l, :]
        if how == "weight_of_next_point":
            w_l = w_l.roll(-1, -1)
        acc = torch.zeros(N, Lq, M, P, D, dtype=dt)
        for dy, dx in corners:
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)       # in floating point: +-1e9 is simply outside
            if how == "border_clamp" or (how == "mask_dropped_on_one_corner" and (dy, dx) == (1, 1)):
                ok = torch.ones_like(ok)
            yi, xi = yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()
            rows = start + yi * (H if how == "hw_swapped_in_row" else W) + xi
            v = value[n_idx, rows.clamp(0, S - 1), m_idx]                    # (N, Lq, M, P, D); the clamp only matters for the mutants
            wgt = (ly if dy else 1 - ly) * (lx if dx else 1 - lx)
            acc = acc + torch.where(ok, wgt, torch.zeros_like(wgt)).unsqueeze(-1) * v
        out = out + (w_l.unsqueeze(-1) * acc).sum(3)
    return out.reshape(N, Lq, M * D)


def evaluate(inp, dt, how=None):
    """dict of the four tensors of TENSORS in dtype ``dt``."""
    value, loc, attn = (inp[k].to(dt).clone().requires_grad_(True) for k in ("value", "loc", "attn"))
    out = forward(value, inp["shapes"], inp["starts"], loc, attn, dt, how)
    out.backward(inp["grad_out"].to(dt))
    return dict(out=out.detach(), grad_value=value.grad, grad_sampling_loc=loc.grad, grad_attn_weight=attn.grad)


def exact(inp, how=None):
    return evaluate(inp, F64, how)


def plain32(inp, how=None):
    return evaluate(inp, F32, how)


_CACHE = {}


def references(case_id, dt, far=False):
    """(inputs, exact, plain32) of a value case, computed once per process and shared: do not modify."""
    key = (case_id, dt, far)
    if key not in _CACHE:
        inp = make_inputs(case_id, dt, far)
        _CACHE[key] = (inp, exact(inp), plain32(inp))
    return _CACHE[key]


def exact_references(D, dt):
    key = ("exact", D, dt)
    if key not in _CACHE:
        inp = make_exact_inputs(D, dt)
        _CACHE[key] = (inp, exact(inp))
    return _CACHE[key]


def value_case_params():
    """(case_id, far) of every value case."""
    return [(c, False) for c in CASES] + [(FAR_CASE, True)]


def ratios(got, ex, p32, out_dtypes):
    """{tensor: worst |err| / bound}; ``out_dtypes`` {tensor: dtype of the output as produced}."""
    return {k: worst_ratio(got[k], ex[k], p32[k], out_dtypes[k]) for k in TENSORS}
