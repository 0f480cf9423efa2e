"""References for the fused HAT block kernels (csrc/fvit_attnblk.hip, fvit_attnblk2.hip, fvit_winblk.hip, fvit_ctblk.hip, fvit_mlp.hip, fvit_winmlp.hip,
fvit_lngemm.hip), shared by tests/test_fused_block_refs_cpu.py (the proof that the references and the bar are fair and have teeth, no GPU) and
tests/test_gpu_fused_blocks_branch.py (the kernels through the C ABI).  Plain PyTorch on the CPU, nothing else.

Four chains, each a class with two static functions over the SAME inputs -- the values the kernel receives: weights already rounded to the operand
type T, eps and scale already rounded to fp32 as the C ABI passes them:

    exact(inp)              float64, nothing rounded in between.
    plain16(inp, **opt)     float32 arithmetic, rounded to T at exactly the points where the kernels narrow (below).  ``opt`` selects another legitimate
                            way to do the same arithmetic (VARIANTS) or a deliberate error (the mutants of the CPU test).

attn_block, ct_block and mlp return ``(branch, xin)``: the kernels compute out = xin + branch in fp32 and the branch is what they are tested on
(in place: got - x0; out of place: got - xin with xin the gathered row; recovering it costs at most 2^-23 * max(|xin|, |out|)).  ln_gemm returns
``(out, xin)``: the pre-narrowing fp32 result of the GEMM epilogue and the gathered rows the kernel copies to x_out.

Where the kernels narrow to T (the same list in every work split of a chain):

    xn   LayerNorm output      fvit_attnblk.hip:234  fvit_attnblk2.hip:197  fvit_winblk.hip:211  fvit_ctblk.hip:193,599  fvit_mlp.hip:181
                               fvit_winmlp.hip:253  fvit_lngemm.hip:152-153
    q k  after their bias      fvit_attnblk.hip:318-319  fvit_attnblk2.hip:283-284,321-322  fvit_winblk.hip:254-255  fvit_ctblk.hip:238-239,642-643
    v    after its bias        fvit_attnblk.hip:329  fvit_attnblk2.hip:290-293  fvit_winblk.hip:265-266  fvit_ctblk.hip:245,649
    P    exp(score - max), NOT yet normalised; the row sum is taken over the unrounded fp32 values
                               fvit_attnblk.hip:381-382  fvit_attnblk2.hip:363-364  fvit_winblk.hip:306-307  fvit_ctblk.hip:271,677
    o    (P v) * (1 / sum)     fvit_attnblk.hip:393-394  fvit_attnblk2.hip:377-378  fvit_winblk.hip:315-316  fvit_ctblk.hip:279,685
    h    GELU(fc1 + b)         fvit_ctblk.hip:367,780  fvit_mlp.hip:300,373  fvit_winmlp.hip:333,418
    out  ln_gemm's result      fvit_lngemm.hip:223   (the test's bar carries this rounding as u_T * |exact| + sub_T, plain16 stops before it)

Everything else stays fp32 in the kernels: the gathered row (src + add), the LayerNorm statistics (two passes: mean, then centred squares), the MFMA
accumulators, scores, the softmax sum, proj / fc2 results, ct_block's intermediate residual ct1 (the second LayerNorm reads the fp32 rows), the
residual add.

The bar, per output tensor (``branch_bound`` / ``out16_bound`` / ``ratios``):

    bound[i] = F_max * e16 + 2^-23 * max(|xin[i]|, |exact_out[i]|)      e16 = max_i |plain16[i] - exact[i]|      (fp32 outputs: the branch)
    bound[i] = u_T * |exact[i]| + sub_T + F_max * e16                                                              (ln_gemm's 16-bit output)
    and   rms(got - exact) <= F_rms * rms(plain16 - exact)            (ln_gemm: plain16 rounded to T here, since got is)

F_max and F_rms come from the reference alone: tests/test_fused_block_refs_cpu.py evaluates every entry of VARIANTS (P rounded after the
normalisation instead of before it; every K loop accumulated in blocks of 16 and of 32 instead of one matmul -- the MFMA K steps; LayerNorm sums as a
pairwise tree and as a sequential loop) on every case of the tables below and seeds 0..3, and F is twice the largest ratio of a variant's error to the
base plain16 error of the same case, plus 2 % and rounded up to one decimal (the study's own matmuls move the ratios by 0.15 % between 1, 3, 8 and 32 CPU
threads).  The factor two is for what the study leaves out -- the kernels' __expf, 1.0f / sum, the erf polynomial of gelu_fast (fvit_common.h:180) and
rsqrtf, all orders below a 16-bit rounding, and the spread of a maximum over seeds not drawn.  Measured, worst variant over all cases, both operand
types, 4 seeds (e16 itself: 5e-4 .. 2.3e-3 in fp16, 4e-3 .. 2.5e-2 in bf16):

    chain        max ratio  (variant, case)                        rms ratio  (variant)       F_max  F_rms
    attn_block   1.298      p_after_norm, C 256 S 49 nwin 1 fp16   1.096      p_after_norm    2.7    2.3
    ct_block     1.449      p_after_norm, batch 2 G 4 fp16         1.115      p_after_norm    3.0    2.3
    mlp          1.459      ln_seq, M 17 C 256 fp16                1.212      ln_seq          3.0    2.5
    ln_gemm      1.005      ln_seq, M 130 C 512 fp16               1.002      ln_seq          2.1    2.1

    per variant (max / rms):  attn_block  p_after_norm 1.30 / 1.10  kblock16 1.08 / 1.00  kblock32 1.05 / 1.00  ln_tree 1.06 / 1.00  ln_seq 1.14 / 1.01
                              ct_block    p_after_norm 1.45 / 1.12  kblock16 1.12 / 1.01  kblock32 1.13 / 1.01  ln_tree 1.08 / 1.04  ln_seq 1.15 / 1.03
                              mlp         kblock16 1.02 / 1.00  kblock32 1.03 / 1.00  ln_tree 1.29 / 1.08  ln_seq 1.46 / 1.21
                              ln_gemm     kblock16 1.00 / 1.00  kblock32 1.00 / 1.00  ln_tree 1.00 / 1.00  ln_seq 1.00 / 1.00

No constant here comes from a kernel's output.  tanh-GELU in place of the erf form is below this suite's resolution and is recorded, not asserted, by
the CPU test (see its docstring for the figures)."""
import torch

from tests.backward_primitive_refs import F32, F64, SUB_T, U_T, f32_scalar, gen, rounded

OPERAND_DTYPES = [torch.float16, torch.bfloat16]
LN_EPS = 1e-5
CHAINS = ("attn_block", "ct_block", "mlp", "ln_gemm")
# twice the worst variant ratio of the study (module docstring), plus 2 %, rounded up to one decimal; F_max <= 4 is a condition of the suite: a study
# that wants more says plain16 lacks a rounding point
F_MAX = {"attn_block": 2.7, "ct_block": 3.0, "mlp": 3.0, "ln_gemm": 2.1}
F_RMS = {"attn_block": 2.3, "ct_block": 2.3, "mlp": 2.5, "ln_gemm": 2.1}
STUDY_SEEDS = (0, 1, 2, 3)
VARIANTS = {
    "p_after_norm": dict(p_after_norm=True),       # attention chains only
    "kblock16": dict(kblock=16),
    "kblock32": dict(kblock=32),
    "ln_tree": dict(ln_sum="tree"),
    "ln_seq": dict(ln_sum="seq"),
}

# (C, S, nwin, tables): the smallest window counts at which each work split has a tail (S = 16: four windows per workgroup; the two-window forms: odd nwin)
ATTN_CASES = [(256, 16, 5, True), (256, 49, 1, False), (256, 53, 3, True), (256, 64, 2, False), (512, 49, 3, False), (512, 53, 2, True),
              (512, 64, 1, False)]
# (batch, G, add, gamma)
CT_CASES = [(1, 16, True, True), (3, 9, True, False), (5, 1, False, True), (2, 4, True, True)]
CT_C, CT_HEADS, CT_HIDDEN, CT_ROWS_A = 256, 8, 1024, 37
MLP_M, MLP_C = [1, 17, 64, 65, 129, 300], [256, 512]
# (M, C, N, act, gather)
LN_GEMM_CASES = [(17, 256, 768, 0, True), (65, 256, 1024, 1, False), (130, 512, 2048, 1, False)]
SPARE = 3               # rows behind every row buffer: finite garbage behind inputs, NaN behind outputs
SRCB_ROWS, ADD_ROWS = 7, 11
HOT_MEAN = 300.0        # one row per case has this mean and standard deviation 1: a one-pass variance would lose it


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the arithmetic: float64 and nothing rounded (dt None), or float32 with the kernels' narrowing points
# ------------------------------------------------------------------------------------------------------------------------------------------------
class Arith:
    def __init__(self, dt, **opt):
        self.dt, self.ft, self.opt = dt, (F64 if dt is None else F32), opt

    def __call__(self, t):
        return None if t is None else t.to(self.ft)

    def narrow(self, t):
        return t if self.dt is None else t.to(self.dt).to(F32)

    def mm(self, a, w):
        """a [..., K] times w [..., N, K] transposed; with opt kblock the K range is accumulated block by block, as MFMA K steps are."""
        wt, kb = w.transpose(-1, -2), self.opt.get("kblock")
        if not kb:
            return a @ wt
        acc = None
        for k0 in range(0, a.shape[-1], kb):
            part = a[..., k0:k0 + kb] @ wt[..., k0:k0 + kb, :]
            acc = part if acc is None else acc + part
        return acc

    def rowsum(self, t):
        how = self.opt.get("ln_sum")
        if how == "seq":
            acc = t[..., 0].clone()
            for c in range(1, t.shape[-1]):
                acc = acc + t[..., c]
            return acc
        if how == "tree":
            assert t.shape[-1] & (t.shape[-1] - 1) == 0
            while t.shape[-1] > 1:
                t = t[..., 0::2] + t[..., 1::2]
            return t[..., 0]
        return t.sum(-1)

    def layernorm(self, x, w, b, eps):
        C = x.shape[-1]
        d = x - (self.rowsum(x) / C)[..., None]
        rstd = (self.rowsum(d * d) / C + eps).rsqrt()
        return self.narrow(d * rstd[..., None] * self(w) + self(b))

    def gelu(self, a):
        if self.opt.get("gelu") == "tanh":
            return 0.5 * a * (1.0 + torch.tanh(0.7978845608028654 * (a + 0.044715 * a * a * a)))
        return 0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752))


def spad(S):
    """fvit_attention_spad for the window lengths of these cases (S <= 64): the bias table's padded side."""
    assert 1 <= S <= 64
    return (S + 15) // 16 * 16


def _tile_without(b, tile):
    b = b.clone()
    b[tile * 16:tile * 16 + 16] = 0.0
    return b


def _loudest_tile(b):
    return int(b.view(-1, 16).abs().sum(1).argmax())


def _gather(A, inp):
    """xin [rows][C] = srcA or srcB row by src_idx (+ the add row by add_idx), image by image: the row selection of fvit_gather_layernorm."""
    srcA, nimg, rpi, C = A(inp["srcA"]), inp["nimg"], inp["rows_per_image"], inp["C"]
    si, ai = inp.get("src_idx"), inp.get("add_idx")
    if si is None:
        x = srcA[:nimg * rpi]
    else:
        rowsA, rowsB = inp["rowsA"], inp["rowsB"]
        a = srcA[:nimg * rowsA].view(nimg, rowsA, C)[:, si.clamp(min=0)]
        if (si < 0).any():
            bi = (-si - 1).clamp(min=0) + (1 if A.opt.get("mut") == "neg_src_neighbour" else 0)
            a = torch.where((si >= 0)[None, :, None], a, A(inp["srcB"])[:nimg * rowsB].view(nimg, rowsB, C)[:, bi])
        x = a.reshape(nimg * rpi, C)
    if inp.get("add") is not None:
        ai = torch.arange(rpi) if ai is None else ai
        addv = torch.where((ai >= 0)[:, None], A(inp["add"])[ai.clamp(min=0)], torch.zeros((), dtype=A.ft))
        addv = addv[None].expand(nimg, rpi, C).clone()
        if A.opt.get("mut") == "add_ignored_one_row":
            addv[0, int((ai >= 0).nonzero()[-1])] = 0.0
        x = x + addv.reshape(nimg * rpi, C)
    return x


def _rows_in(A, xin):
    """The rows the chain computes from: xin itself, or (mutant) the last row computed from the row before it."""
    if A.opt.get("mut") == "last_row_from_prev":
        xin = xin.clone()
        xin[-1] = xin[-2]
    return xin


def _attention(A, xn, wqkv, bqkv, bias, scale, heads):
    """xn [nwin][S][C] -> o [nwin][S][C] (narrowed): q / k / v narrowed after their bias, P narrowed before the normalisation, o after it."""
    nwin, S, C = xn.shape
    d, mut = C // heads, A.opt.get("mut")
    qkv = A.narrow(A.mm(xn, A(wqkv)) + A(bqkv))
    q, k, v = qkv.view(nwin, S, 3, heads, d).permute(2, 0, 3, 1, 4)          # each [nwin][heads][S][d]
    b = A(bias)
    if mut == "head_bias_shift":
        b = b.roll(1, 0)
    elif mut == "bias_transposed":
        b = b.transpose(-1, -2)
    sc = A.mm(q, k) * scale + b
    if mut == "drop_last_key":
        sc, v = sc[..., :-1], v[..., :-1, :]
    elif mut == "leak_key":               # one padded key enters at score 0 (no mask bias) with the next window's first V row
        sc = torch.cat([sc, torch.zeros_like(sc[..., :1])], -1)
        v = torch.cat([v, v.roll(-1, 0)[..., :1, :]], -2)
    e = (sc - sc.amax(-1, keepdim=True)).exp()
    total = e.sum(-1, keepdim=True)
    if A.opt.get("p_after_norm"):
        o = A.narrow(A.mm(A.narrow(e / total), v.transpose(-1, -2)))
    else:
        o = A.narrow(A.mm(A.narrow(e), v.transpose(-1, -2)) * (1.0 / total))
    return o.transpose(1, 2).reshape(nwin, S, C)


def _attn_branch(A, inp, x, S):
    """gamma * (proj(attention(LayerNorm(x))) + b_proj) over windows of S rows of x."""
    mut, C = A.opt.get("mut"), inp["C"]
    xn = A.layernorm(x.view(-1, S, C), inp["ln_w"], inp["ln_b"], inp["eps"])
    o = _attention(A, xn, inp["wqkv"], inp["bqkv"], inp["bias"], inp["scale"], inp["heads"])
    bproj = _tile_without(inp["bproj"], _loudest_tile(inp["bproj"])) if mut == "proj_bias_tile" else inp["bproj"]
    y = (A.mm(o, A(inp["wproj"])) + A(bproj)).reshape(-1, C)
    return _scaled(A, y, inp.get("gamma"), "gamma_one")


def _scaled(A, y, gamma, mut_name):
    if gamma is None:
        return y
    gamma = A(gamma)
    if A.opt.get("mut") == mut_name:
        gamma = gamma.clone()
        gamma[int((gamma - 1.0).abs().argmax())] = 1.0
    return gamma * y


def _mlp_branch(A, inp, x, pre=""):
    """gamma * (fc2(GELU(fc1(LayerNorm(x)) + b1)) + b2), h narrowed after GELU."""
    mut = A.opt.get("mut")
    xn = A.layernorm(x, inp[pre + "ln_w"], inp[pre + "ln_b"], inp["eps"])
    b1 = _tile_without(inp["b1"], _loudest_tile(inp["b1"])) if mut == "fc1_bias_tile" else inp["b1"]
    b2 = inp["b2"]
    if mut == "fc2_bias_channel":
        b2 = b2.clone()
        b2[int(b2.abs().argmax())] = 0.0
    h = A.narrow(A.gelu(A.mm(xn, A(inp["w1"])) + A(b1)))
    return _scaled(A, A.mm(h, A(inp["w2"])) + A(b2), inp.get(pre + "gamma"), "gamma2_one" if pre else "gamma_one")


class attn_block:
    """x_out = xin + gamma * proj(softmax(q k^T * scale + bias) v),  [q|k|v] = qkv(LayerNorm(xin)),  xin gathered by src_idx / add_idx / add."""

    @staticmethod
    def run(A, inp):
        xin = _gather(A, inp)
        return _attn_branch(A, inp, _rows_in(A, xin), inp["S"]), xin

    @staticmethod
    def exact(inp):
        return attn_block.run(Arith(None), inp)

    @staticmethod
    def plain16(inp, **opt):
        return attn_block.run(Arith(inp["dt"], **opt), inp)


class ct_block:
    """The carrier branch: ct0 = X[src_idx] (+ add); ct1 = ct0 + gamma1 * attention sub-block over the image's G tokens;
    out = ct1 + gamma2 * fc2(GELU(fc1(LayerNorm2(ct1)))).  The branch is out - ct0."""

    @staticmethod
    def run(A, inp):
        ct0 = _gather(A, inp)
        x = _rows_in(A, ct0)
        b1 = _attn_branch(A, inp, x, inp["S"])
        ct1 = x + b1
        b2 = _mlp_branch(A, inp, x if A.opt.get("mut") == "ln2_pre_residual" else ct1, pre="ln2_")
        return b1 + b2, ct0

    @staticmethod
    def exact(inp):
        return ct_block.run(Arith(None), inp)

    @staticmethod
    def plain16(inp, **opt):
        return ct_block.run(Arith(inp["dt"], **opt), inp)


class mlp:
    """x += gamma * fc2(GELU(fc1(LayerNorm(x)))), in place."""

    @staticmethod
    def run(A, inp):
        xin = A(inp["srcA"])[:inp["nimg"]]
        return _mlp_branch(A, inp, _rows_in(A, xin)), xin

    @staticmethod
    def exact(inp):
        return mlp.run(Arith(None), inp)

    @staticmethod
    def plain16(inp, **opt):
        return mlp.run(Arith(inp["dt"], **opt), inp)


class ln_gemm:
    """out = act(LayerNorm(xin) W^T + bias) before its rounding to T; xin gathered as in attn_block (the kernel's x_out)."""

    @staticmethod
    def run(A, inp):
        xin = _gather(A, inp)
        xn = A.layernorm(_rows_in(A, xin), inp["ln_w"], inp["ln_b"], inp["eps"])
        bias = _tile_without(inp["bias"], _loudest_tile(inp["bias"])) if A.opt.get("mut") == "fc1_bias_tile" else inp["bias"]
        y = A.mm(xn, A(inp["W"])) + A(bias)
        return (A.gelu(y) if inp["act"] else y), xin

    @staticmethod
    def exact(inp):
        return ln_gemm.run(Arith(None), inp)

    @staticmethod
    def plain16(inp, **opt):
        return ln_gemm.run(Arith(inp["dt"], **opt), inp)


CHAIN = {"attn_block": attn_block, "ct_block": ct_block, "mlp": mlp, "ln_gemm": ln_gemm}


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the bar
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _rms(t):
    return t.to(F64).pow(2).mean().sqrt().item()


def branch_bound(exact, plain, xin, f_max):
    exact, xin = exact.to(F64), xin.to(F64)
    e16 = (plain.to(F64) - exact).abs().max().item()
    return f_max * e16 + 2.0 ** -23 * torch.maximum(xin.abs(), (xin + exact).abs())


def out16_bound(exact, plain, dt, f_max):
    exact = exact.to(F64)
    e16 = (plain.to(F64) - exact).abs().max().item()
    return U_T[dt] * exact.abs() + (SUB_T[dt] + f_max * e16)


def ratios(chain, got, exact, plain, xin, dt):
    """(max_i |got - exact| / bound[i],  rms(got - exact) / (F_rms * rms(plain16 - exact))): both must be <= 1.  ``got`` is the branch of the fp32
    chains and the 16-bit output of ln_gemm; inf when it holds a non-finite value."""
    got, exact = got.detach().cpu().to(F64), exact.to(F64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    if not torch.isfinite(got).all():
        return float("inf"), float("inf")
    if chain == "ln_gemm":
        bound, base = out16_bound(exact, plain, dt, F_MAX[chain]), rounded(plain, dt)
    else:
        bound, base = branch_bound(exact, plain, xin, F_MAX[chain]), plain
    err = got - exact
    return (err.abs() / bound).max().item(), _rms(err) / (F_RMS[chain] * _rms(base.to(F64) - exact))


def variant_ratios(exact, plain, variant):
    """(max, rms) error of another legitimate evaluation relative to the base plain16's: what F is twice the largest of."""
    exact = exact.to(F64)
    ev, eb = variant.to(F64) - exact, plain.to(F64) - exact
    return ev.abs().max().item() / eb.abs().max().item(), _rms(ev) / _rms(eb)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the case tables' inputs, from a seeded CPU generator: the same tensors on the CPU self-check and on the GPU
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _rows(g, n, C):
    return torch.randn(n, C, generator=g) * 1.3 + 0.2


def _garbage(g, n, C):
    return torch.randn(n, C, generator=g) * 1e3


def _hot(g, C):
    return HOT_MEAN + torch.randn(C, generator=g)


def _weight(g, n, k, dt):
    return rounded(torch.randn(n, k, generator=g) / k ** 0.5, dt)


def _vec(g, n):
    return torch.randn(n, generator=g) * 0.3


def _ln_w(g, C):
    return torch.rand(C, generator=g) + 0.5


def _bias_table(g, heads, S):
    return torch.randn(heads, S, S, generator=g) * 2.0 - 8.0


def _attn_weights(g, C, dt, use_gamma):
    return dict(ln_w=_ln_w(g, C), ln_b=_vec(g, C), wqkv=_weight(g, 3 * C, C, dt), bqkv=_vec(g, 3 * C), wproj=_weight(g, C, C, dt), bproj=_vec(g, C),
                gamma=_ln_w(g, C) if use_gamma else None, eps=f32_scalar(LN_EPS), scale=f32_scalar(32 ** -0.5))


def _gather_tables(g, inp, nimg, rpi, C):
    """The tables of test_attn_block_fused: row 1 of every image comes from srcB row 2, row 5 repeats the image's last row, rows 2.. get an add row.
    Every srcA / srcB row that no index names holds garbage."""
    si = torch.arange(rpi)
    si[1] = -3
    si[5 % rpi] = rpi - 1
    ai = torch.full((rpi,), -1, dtype=torch.int64)
    ai[2:] = torch.arange(rpi - 2) % ADD_ROWS
    srcB = _garbage(g, nimg * SRCB_ROWS + SPARE, C)
    srcB[2:nimg * SRCB_ROWS:SRCB_ROWS] = _rows(g, nimg, C)
    named = torch.zeros(rpi, dtype=torch.bool)
    named[si[si >= 0]] = True
    srcA = inp["srcA"]
    for r in (~named).nonzero().flatten().tolist():
        srcA[r:nimg * rpi:rpi] = _garbage(g, nimg, C)
    add = torch.cat([torch.randn(ADD_ROWS, C, generator=g), _garbage(g, SPARE, C)])
    inp.update(srcB=srcB, rowsB=SRCB_ROWS, src_idx=si, add_idx=ai, add=add)


def attn_inputs(case, dt, seed=0):
    C, S, nwin, tables = case
    g = gen(seed * 7919 + 11000 + C + S * 131 + nwin)
    rows = nwin * S
    srcA = torch.cat([_rows(g, rows, C), _garbage(g, SPARE, C)])
    srcA[3] = _hot(g, C)
    inp = dict(chain="attn_block", dt=dt, C=C, S=S, heads=C // 32, nimg=nwin, rows_per_image=S, rowsA=S, rowsB=0, srcA=srcA,
               bias=_bias_table(g, C // 32, S), **_attn_weights(g, C, dt, use_gamma=nwin > 1))
    if tables:
        _gather_tables(g, inp, nwin, S, C)
    return inp


def ct_inputs(case, dt, seed=0):
    batch, G, use_add, use_gamma = case
    C, hid, rowsA = CT_C, CT_HIDDEN, CT_ROWS_A
    g = gen(seed * 7919 + 12000 + batch * 17 + G)
    si = torch.randperm(rowsA, generator=g)[:G]
    srcA = _garbage(g, batch * rowsA + SPARE, C)                      # only the G carrier rows of every image are real
    for r in si.tolist():
        srcA[r:batch * rowsA:rowsA] = _rows(g, batch, C)
    srcA[int(si[0])] = _hot(g, C)
    inp = dict(chain="ct_block", dt=dt, C=C, S=G, heads=CT_HEADS, hidden=hid, nimg=batch, rows_per_image=G, rowsA=rowsA, rowsB=0, srcA=srcA, src_idx=si,
               bias=_bias_table(g, CT_HEADS, G), **_attn_weights(g, C, dt, use_gamma))
    if use_add:
        inp["add"] = torch.cat([torch.randn(G, C, generator=g), _garbage(g, SPARE, C)])
    inp.update(ln2_ln_w=_ln_w(g, C), ln2_ln_b=_vec(g, C), w1=_weight(g, hid, C, dt), b1=_vec(g, hid), w2=_weight(g, C, hid, dt), b2=_vec(g, C),
               ln2_gamma=_ln_w(g, C) if use_gamma else None)
    return inp


def mlp_inputs(M, C, use_gamma, dt, seed=0):
    g = gen(seed * 7919 + 13000 + M * 3 + C + int(use_gamma))
    hid = 4 * C
    srcA = torch.cat([_rows(g, M, C), _garbage(g, SPARE, C)])         # in place: the spare rows must come back bit for bit
    srcA[M // 2] = _hot(g, C)
    return dict(chain="mlp", dt=dt, C=C, hidden=hid, nimg=M, rows_per_image=1, srcA=srcA, ln_w=_ln_w(g, C), ln_b=_vec(g, C), w1=_weight(g, hid, C, dt), b1=_vec(g, hid),
                w2=_weight(g, C, hid, dt), b2=_vec(g, C), gamma=_ln_w(g, C) if use_gamma else None, eps=f32_scalar(LN_EPS))


def ln_gemm_inputs(case, dt, seed=0):
    M, C, N, act, gather = case
    g = gen(seed * 7919 + 14000 + M + C + N)
    inp = dict(chain="ln_gemm", dt=dt, C=C, N=N, act=act, ln_w=_ln_w(g, C), ln_b=_vec(g, C), W=_weight(g, N, C, dt), bias=_vec(g, N), eps=f32_scalar(LN_EPS))
    if gather:
        rpi = M                                                        # one image of M rows, through the tables
        srcA = torch.cat([_rows(g, rpi, C), _garbage(g, SPARE, C)])
        inp.update(nimg=1, rows_per_image=rpi, rowsA=rpi, srcA=srcA)
        _gather_tables(g, inp, 1, rpi, C)
    else:
        inp.update(nimg=M, rows_per_image=1, rowsA=0, rowsB=0, srcA=torch.cat([_rows(g, M, C), _garbage(g, SPARE, C)]))
    inp["srcA"][3] = _hot(g, C)
    return inp


def all_cases(dts=OPERAND_DTYPES):
    """(id, chain, maker(seed)) of every case of the GPU test."""
    out = []
    for dt in dts:
        tn = "f16" if dt == torch.float16 else "bf16"
        for c in ATTN_CASES:
            out.append((f"attn_block-{c[0]}-{c[1]}-{c[2]}-{int(c[3])}-{tn}", "attn_block", lambda seed, c=c, dt=dt: attn_inputs(c, dt, seed)))
        for c in CT_CASES:
            out.append((f"ct_block-{c[0]}-{c[1]}-{int(c[2])}-{int(c[3])}-{tn}", "ct_block", lambda seed, c=c, dt=dt: ct_inputs(c, dt, seed)))
        for C in MLP_C:
            for M in MLP_M:
                for ug in (True, False):
                    out.append((f"mlp-{M}-{C}-{int(ug)}-{tn}", "mlp", lambda seed, M=M, C=C, ug=ug, dt=dt: mlp_inputs(M, C, ug, dt, seed)))
        for c in LN_GEMM_CASES:
            out.append((f"ln_gemm-{c[0]}-{c[1]}-{c[2]}-{c[3]}-{int(c[4])}-{tn}", "ln_gemm", lambda seed, c=c, dt=dt: ln_gemm_inputs(c, dt, seed)))
    return out
