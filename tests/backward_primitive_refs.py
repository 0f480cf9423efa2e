"""References for the backward primitives of csrc/fvit_bwd.hip, shared by tests/test_backward_primitive_refs_cpu.py (the proof that the inputs and
the bar are fair, no GPU) and tests/test_gpu_backward_primitives.py (the kernels through the C ABI).  Plain PyTorch on the CPU, nothing else.

Every primitive is a small class with two static functions over the SAME inputs -- the values the kernel gets, i.e. already rounded to 16 bits where
the kernel's operand is 16-bit, and scalars (eps, scale) already rounded to fp32 as the C ABI passes them:

    exact(...)    float64.  torch.autograd where the operation has a forward (LayerNorm, GELU', the attention core); the written-out formula otherwise.
    plain32(...)  the written-out formula in float32 with ordinary PyTorch operations: a second, independent rounding of the same arithmetic.

Both return a dict of named output tensors.  ``formula(..., dtype)`` is the written-out form itself; the CPU test checks its float64 evaluation
against autograd wherever ``exact`` is autograd, and against an autograd statement of the same gradient where ``exact`` is the formula.

The one bar of all value comparisons (``bound``), per output tensor:

    bound[i] = u_T * |exact[i]| + sub_T + 8 * e32 + 2^-24 * max|exact|          e32 = max_i |plain32[i] - exact[i]|
    u_T = 2^-11 (fp16 output), 2^-8 (bf16), 0 (fp32);   sub_T = 2^-24 (fp16: the subnormal spacing), else 0

The first two terms are one correct rounding to the output type.  The third gives the kernel's fp32 arithmetic 8 x the error a plain fp32 evaluation
of the same formula makes: room for another summation order (64 sequential terms or a wave tree against PyTorch's vectorised sums) and for the
device's few-ulp erff / expf / rsqrtf.  The last keeps the bar above zero where plain32 happens to be exact.  The bar is measured against the
reference and never against what a kernel returns."""
import torch
import torch.nn.functional as F

BWD_ROWS = 64          # rows per block of the column-sum kernels (fvit_bwd_blocks)
E32_FACTOR = 8.0
U_T = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
SUB_T = {torch.float16: 2.0 ** -24, torch.bfloat16: 0.0, torch.float32: 0.0}
F64, F32 = torch.float64, torch.float32


def f32_scalar(v: float) -> float:
    """The value a C ``float`` argument carries (eps, scale)."""
    return torch.tensor(v, dtype=F32).item()


def bound(exact: torch.Tensor, plain32: torch.Tensor, out_dtype) -> torch.Tensor:
    exact = exact.to(F64)
    e32 = (plain32.to(F64) - exact).abs().max().item() if exact.numel() else 0.0
    peak = exact.abs().max().item() if exact.numel() else 0.0
    return U_T[out_dtype] * exact.abs() + (SUB_T[out_dtype] + E32_FACTOR * e32 + 2.0 ** -24 * peak)


def worst_ratio(got: torch.Tensor, exact: torch.Tensor, plain32: torch.Tensor, out_dtype) -> float:
    """max_i |got[i] - exact[i]| / bound[i]; inf when ``got`` holds a non-finite value."""
    got = got.detach().cpu().to(F64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - exact.to(F64)).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound(exact, plain32, out_dtype))    # an all-zero tensor has a zero bar: only 0 meets it
    return ratio.max().item() if ratio.numel() else 0.0


def block_sums(t: torch.Tensor, rows: int = BWD_ROWS) -> torch.Tensor:
    """[M][...] -> [ceil(M / rows)][...]: the sum over each block of ``rows`` consecutive rows (the last block may be ragged)."""
    return torch.stack([c.sum(0) for c in t.split(rows, 0)])


# ------------------------------------------------------------------------------------------------------------------------------------------------
class scale_cols:
    """dz = gamma * dy; part[b][0] = sum over block b of dy * z, part[b][1] = of gamma * dy.  Backward of y = x + gamma * z in gamma and z."""

    @staticmethod
    def formula(dy, z, gamma, dtype):
        dy, z = dy.to(dtype), z.to(dtype)
        v = dy * gamma.to(dtype) if gamma is not None else dy
        part = torch.stack([block_sums(dy * z), block_sums(v)], 1)          # [blocks][2][C]
        return dict(dz=v, part=part, dgamma=(dy * z).sum(0), dbias=v.sum(0))

    @staticmethod
    def exact(dy, z, gamma):
        return scale_cols.formula(dy, z, gamma, F64)

    @staticmethod
    def plain32(dy, z, gamma):
        return scale_cols.formula(dy, z, gamma, F32)

    @staticmethod
    def autograd(dy, z, gamma):
        """dgamma, dz and the gradient of a bias inside z, from y = gamma * (z + b) differentiated in float64."""
        zl = z.to(F64).clone().requires_grad_(True)
        gl = (gamma.to(F64).clone() if gamma is not None else torch.ones(z.shape[1], dtype=F64)).requires_grad_(True)
        bl = torch.zeros(z.shape[1], dtype=F64, requires_grad=True)
        (gl * (zl + bl)).backward(dy.to(F64))
        return dict(dz=zl.grad, dgamma=gl.grad, dbias=bl.grad)


class gelu_fwd:
    """h = GELU(a), erf form."""

    @staticmethod
    def formula(a, dtype):
        a = a.to(dtype)
        return dict(out=0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752)))

    @staticmethod
    def exact(a):
        return gelu_fwd.formula(a, F64)

    @staticmethod
    def plain32(a):
        return gelu_fwd.formula(a, F32)

    @staticmethod
    def autograd(a):
        return dict(out=F.gelu(a.to(F64)))


class gelu_bwd:
    """da = dh * GELU'(a); part[b] = the column sums of the unrounded da over block b."""

    @staticmethod
    def formula(a, dh, dtype):
        a, dh = a.to(dtype), dh.to(dtype)
        da = dh * (0.5 * (1.0 + torch.erf(a * 0.70710678118654752)) + a * 0.3989422804014327 * torch.exp(-0.5 * a * a))
        return dict(out=da, part=block_sums(da), dbias=da.sum(0))

    @staticmethod
    def exact(a, dh):
        al = a.to(F64).clone().requires_grad_(True)
        F.gelu(al).backward(dh.to(F64))
        da = al.grad
        return dict(out=da, part=block_sums(da), dbias=da.sum(0))

    @staticmethod
    def plain32(a, dh):
        return gelu_bwd.formula(a, dh, F32)


class layernorm:
    """Backward of xn = LayerNorm(x) * w + b given dxn, plus the skip connection's dy:  dx = dy + rstd * (g - mean(g) - xhat * mean(g * xhat)),
    g = dxn * w; stats = (mean, rstd) per row; part[b][0] = block sums of dxn * xhat (-> dw), part[b][1] = of dxn (-> db)."""

    @staticmethod
    def formula(x, dxn, dy, w, eps, dtype):
        x, dxn, w = x.to(dtype), dxn.to(dtype), w.to(dtype)
        mean = x.mean(-1, keepdim=True)
        xc = x - mean
        rstd = ((xc * xc).mean(-1, keepdim=True) + eps).rsqrt()
        xh = xc * rstd
        g = dxn * w
        dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        if dy is not None:
            dx = dy.to(dtype) + dx
        part = torch.stack([block_sums(dxn * xh), block_sums(dxn)], 1)
        return dict(dx=dx, stats=torch.cat([mean, rstd], 1), part=part, dw=(dxn * xh).sum(0), db=dxn.sum(0))

    @staticmethod
    def exact(x, dxn, dy, w, eps):
        out = layernorm.formula(x, dxn, dy, w, eps, F64)               # stats and the per-block partial sums have no autograd form
        xl, wl = x.to(F64).clone().requires_grad_(True), w.to(F64).clone().requires_grad_(True)
        bl = torch.zeros_like(wl).requires_grad_(True)
        F.layer_norm(xl, (x.shape[1],), wl, bl, eps).backward(dxn.to(F64))
        out.update(dx=xl.grad + dy.to(F64) if dy is not None else xl.grad, dw=wl.grad, db=bl.grad)
        return out

    @staticmethod
    def plain32(x, dxn, dy, w, eps):
        return layernorm.formula(x, dxn, dy, w, eps, F32)


class colsum16:
    """part[b] = the column sums of a 16-bit matrix over block b (-> a bias gradient)."""

    @staticmethod
    def formula(t, dtype):
        t = t.to(dtype)
        return dict(part=block_sums(t), total=t.sum(0))

    @staticmethod
    def exact(t):
        return colsum16.formula(t, F64)

    @staticmethod
    def plain32(t):
        return colsum16.formula(t, F32)

    @staticmethod
    def autograd(t):
        """The gradient of b in (x + b) under the upstream gradient t."""
        bl = torch.zeros(t.shape[1], dtype=F64, requires_grad=True)
        (torch.zeros(t.shape, dtype=F64) + bl).backward(t.to(F64))
        return dict(total=bl.grad)


class colsum_finish:
    """out (+)= the sum over the blocks of part[b], in block order."""

    @staticmethod
    def formula(part, out0, dtype):
        s = torch.zeros(part.shape[1], dtype=dtype)
        for b in range(part.shape[0]):
            s = s + part[b].to(dtype)
        return dict(out=s if out0 is None else out0.to(dtype) + s)

    @staticmethod
    def exact(part, out0=None):
        return colsum_finish.formula(part, out0, F64)

    @staticmethod
    def plain32(part, out0=None):
        return colsum_finish.formula(part, out0, F32)


class attention:
    """The windowed attention core, q / k / v / dO (nwin, heads, S, d), bias (heads, S, S) or None, attn_drop mask (nwin, heads, S, S) or None:
        P = softmax(q k^T * scale + bias),  O = (P . mask) v
        dV = (P . mask)^T dO,  dP = (dO v^T) . mask,  dS = P * (dP - rowsum(dP * P)),  dq = scale * dS k,  dk = scale * dS^T q,  dbias[win] = dS."""

    @staticmethod
    def forward(q, k, v, scale, bias, mask, dtype):
        q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
        att = (q @ k.transpose(-1, -2)) * scale
        if bias is not None:
            att = att + bias.to(dtype)
        p = att.softmax(-1)
        return (p * mask.to(dtype) if mask is not None else p) @ v

    @staticmethod
    def formula(q, k, v, do, scale, bias, mask, dtype):
        q, k, v, do = q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype)
        att = (q @ k.transpose(-1, -2)) * scale
        if bias is not None:
            att = att + bias.to(dtype)
        att = att - att.amax(-1, keepdim=True)
        e = att.exp()
        p = e / e.sum(-1, keepdim=True)
        dp = do @ v.transpose(-1, -2)
        pm = p
        if mask is not None:
            dp, pm = dp * mask.to(dtype), p * mask.to(dtype)
        ds = p * (dp - (dp * p).sum(-1, keepdim=True))
        return dict(dq=(ds @ k) * scale, dk=(ds.transpose(-1, -2) @ q) * scale, dv=pm.transpose(-1, -2) @ do, ds=ds)

    @staticmethod
    def exact(q, k, v, do, scale, bias=None, mask=None):
        ql, kl, vl = (t.to(F64).clone().requires_grad_(True) for t in (q, k, v))
        sl = torch.zeros(q.shape[0], q.shape[1], q.shape[2], q.shape[2], dtype=F64, requires_grad=True)   # per-window score leaf: its gradient is dS
        att = (ql @ kl.transpose(-1, -2)) * scale + sl
        if bias is not None:
            att = att + bias.to(F64)
        p = att.softmax(-1)
        ((p * mask.to(F64) if mask is not None else p) @ vl).backward(do.to(F64))
        return dict(dq=ql.grad, dk=kl.grad, dv=vl.grad, ds=sl.grad)

    @staticmethod
    def plain32(q, k, v, do, scale, bias=None, mask=None):
        return attention.formula(q, k, v, do, scale, bias, mask, F32)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the case table: shapes, and the inputs of each case from a seeded CPU generator (the same tensors on the CPU self-check and on the GPU)
# ------------------------------------------------------------------------------------------------------------------------------------------------
OPERAND_DTYPES = [torch.float16, torch.bfloat16]
TRANSPOSE_SHAPES = [(1, 1), (63, 65), (64, 64), (65, 200), (130, 16)]
SCALE_COLS_M, SCALE_COLS_C = [1, 63, 64, 65, 130], [16, 272, 784]
GELU_M, GELU_H = [1, 65, 130], [64, 320]
GELU_EDGES = [-9.0, -6.0, -3.0, -1e-3, 0.0, 1e-3, 3.0, 6.0, 9.0]
LAYERNORM_SHAPES = [(1, 16), (5, 80), (65, 272), (130, 784)]
LAYERNORM_EPS = 1e-5
COLSUM16_M, COLSUM16_N = [1, 64, 65, 200], [1, 257, 768]
FINISH_BLOCKS, FINISH_N = [1, 4], [1, 257]
# (nwin, S, heads, real head_dim d, padded head_dim D)
ATTENTION_CASES = [(2, 1, 1, 32, 32), (3, 17, 2, 49, 64), (2, 53, 3, 24, 32), (3, 49, 2, 32, 32), (2, 16, 2, 72, 96), (1, 64, 1, 80, 96)]
ATTENTION_VARIANTS = ["nobias", "bias", "bias_nopart", "bias_drop"]
ONE_HOT_CASE = (3, 49, 2, 32, 32)      # this case's bias gets +40 on the diagonal of head 1: a near one-hot softmax, gradients almost zero
ATTENTION_FWD_CASES = [(2, 1, 1, 32, 32), (3, 13, 2, 24, 32), (2, 49, 2, 49, 64), (2, 53, 2, 80, 96), (2, 64, 3, 32, 32)]
DROP_KEEP = 0.8                         # the mask's entries 0 and 1 / keep = 1.25 are exact in fp16 and bf16


def gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def rounded(t: torch.Tensor, dt) -> torch.Tensor:
    """fp32 values representable in ``dt``: what a 16-bit operand buffer holds."""
    return t.to(dt).float()


def scale_cols_inputs(M, C, dt, with_gamma):
    g = gen(1000 + M * 7 + C)
    dy = torch.randn(M, C, generator=g)
    z = rounded(torch.randn(M, C, generator=g) * 1.5, dt)
    gamma = (torch.rand(C, generator=g) + 0.5) if with_gamma else None
    return dy, z, gamma


def gelu_inputs(M, H, dt):
    g = gen(2000 + M * 3 + H)
    a = torch.randn(M, H, generator=g) * 2.5
    a[0, :len(GELU_EDGES)] = torch.tensor(GELU_EDGES)
    dh = torch.randn(M, H, generator=g)
    return rounded(a, dt), rounded(dh, dt)


def layernorm_inputs(M, C):
    g = gen(3000 + M * 5 + C)
    x = torch.randn(M, C, generator=g) * 1.3 + 0.2
    x[0] = 0.5                                                   # variance exactly 0: rstd = eps^-1/2
    if M > 1:
        x[1] = 3.0 + 1e-3 * torch.randn(C, generator=g)          # small variance
    dxn = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g)
    w = 1.0 + 0.3 * torch.randn(C, generator=g)
    return x, dxn, dy, w, f32_scalar(LAYERNORM_EPS)


def colsum16_inputs(M, N, dt):
    return rounded(torch.randn(M, N, generator=gen(4000 + M * 11 + N)), dt)


def finish_inputs(blocks, n):
    g = gen(5000 + blocks * 13 + n)
    return torch.randn(blocks, n, generator=g), torch.randn(n, generator=g) * 3.0 + 1.0


def attention_inputs(case, dt, variant="bias", forward=False):
    """q, k, v, dO as 16-bit-representable fp32 (nwin, heads, S, d); scale as the C float; bias (heads, S, S) or None; mask (nwin, heads, S, S) or None."""
    nwin, S, heads, d, D = case
    g = gen(6000 + S * 7 + heads * 3 + d)
    q, k, v, do = (rounded(torch.randn(nwin, heads, S, d, generator=g), dt) for _ in range(4))
    bias = mask = None
    if variant != "nobias":
        bias = torch.randn(heads, S, S, generator=g) * (2.0 if forward else 1.0)
        if tuple(case) == ONE_HOT_CASE and not forward:
            bias[1] += 40.0 * torch.eye(S)
    if variant == "bias_drop":
        mask = torch.empty(nwin, heads, S, S).bernoulli_(DROP_KEEP, generator=g) / DROP_KEEP
    return q, k, v, do, f32_scalar(d ** -0.5), bias, mask
