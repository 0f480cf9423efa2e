"""References and case tables for the unit window-attention kernels -- csrc/fvit_attn.hip (attn_kernel<T, SB, DP, TT>, the dense in-register kernel)
and csrc/fvit_attnlong.hip (attn_long_kernel<T, DP, TT>, online softmax over 32-key tiles) -- shared by tests/test_attention_refs_cpu.py (conditions,
F study, mutants; no GPU) and tests/test_gpu_attention_exact.py (the kernels through the C ABI).  Plain PyTorch on the CPU; no constant here comes
from a kernel's output.

SELECTOR CASES (the output must torch.equal a gathered V).  With exactly one key at score 0 after the row maximum is taken off and every other score
<= -110 (``selector_gap``), exp of the others is 0 in fp32 under any denormal mode (e^-110 < 2^-158), the row sum is 1, P is one-hot and out[q] is
V[sel(q)] bit for bit.  V is random with full 16-bit mantissas, its pad channels d .. dpad-1 are zero and must come back exactly 0.

    table selector   Q = K = 0; bias[h][q][perm_h(q)] = 0 and -1000 on every other key of a valid row; key columns >= S hold FVIT_MASK_BIAS, query
                     rows >= S hold 0 (FvitAttnWeights.bias); another permutation per head.  Checks the bias indexing at stride Spad, the V^T slot
                     order, the P layout, the output channel map and the window / head offsets.
    QK selector      bias 0 on valid keys, scale 1.0; k_j = c_j, q_i = 64 c_perm(i) with c_j in {-1, +1}^d = the 8-bit index of j followed by d - 8
                     hashed bits (``codes``): distinct codes differ in at least one position, so the gap is >= 128.  Checks every Q / K row and
                     8-column chunk address.
    long kernel      Q = K = 0; the compact table holds 0 at ONE displacement (dy, dx) -- the four corners of qbase - kpos: (0, 0), (w-1, w-1),
                     (-(w-1), 0), (0, -(w-1)) -- and -1000 elsewhere.  A query whose row has one key at the maximum must return that V row exactly;
                     the others (n_g carrier keys at bias 0, or no target inside the window: all keys equal) see several equal scores and are
                     compared with the rounding-level bar against the fp64 mean.

Two-term entries (fvit_window_attention_terms / _long_terms): proper splits lo = round_T(x32 - hi) with x32 on a 2^-20 grid below 4, so hi + lo is
exact in fp32 (``v_two_term``); out_hi == v_hi and out_lo == v_lo.  fvit_window_attention_drop: an all-ones mask reproduces the no-mask bits, a mask
that zeroes the selected key of a row gives exactly 0 there.

The table-in-global branch of launch_long_t (tab_in_lds == 0, fvit_attnlong.hip:274-277) needs fixed + (2w-1)^2 * 4 > 150 KiB, i.e. w >= 95 at
these sizes (S >= 9025): out of reach at small S and not tested here.  dpad 96 with S = 129 is handed from launch_attention to the long kernel
(fvit_attn.hip: launch_attention's first line) with the compact table of the STAGE path; the long kernel takes no dense table, so every dense unit
entry point (plain, drop, terms) refuses that geometry -- which is what the GPU test asserts (NOT_DENSE) -- and the hand-off itself stays with the
whole-model tests of the head_dim 80 models.  The long kernel at dpad 96 is covered by its own selector cases.

Rows of a long selector case with n > 1 keys at the same score return the mean of n V rows.  For the two-term entry ``equal_rows_lo_interval`` holds lo
to it: the kernel's fp32 value y is within e = (n + 4) 2^-24 mean |v| of the exact mean (n products of P = 1 summed in fp32 in any order, the
rescale, 1 / sum and the product: the standard worst-case bound, no constant from a kernel), so lo must lie between the T-roundings of
exact -+ e - hi.

RANDOM CASES at the rounding level.  ``attention(.., dt=None)`` is float64; with dt it is float32 arithmetic narrowed to T where the kernels narrow:

    P   exp(score - max), NOT yet normalised; the row sum takes the unrounded fp32 values     fvit_attn.hip:199-201, 227-228   fvit_attnlong.hip:217-220
    o   (P v) * (1 / sum), the 16-bit store                                                  fvit_attn.hip:254, 267            fvit_attnlong.hip:260-262

The bar:  bound[i] = u_T |exact[i]| + sub_T + F_max e16, e16 = max |plain16 - exact|, and rms(got - exact) <= F_rms rms(plain16 - exact).  F = twice the
worst ratio of a variant's error to the base plain16 error of the same case over seeds 0..3, plus 2 %, rounded up to one decimal; F_max <= 4 is a
condition.  Variants: P rounded after the normalisation (dense kernel only), P v accumulated in 32-key blocks, and for the long kernel an online
softmax over 32-key tiles with rescale.  p_after_norm is no variant of the long kernel: an online softmax narrows a tile's P before the row's
normalisation constant exists, so no form of that kernel can round P after it (measured there it would ask 2.47 / 1.31 -> F_max 5.1, past the
condition; without it the long kernel's bar is the TIGHTER one).  Measured by tests/test_attention_refs_cpu.py over RANDOM_DENSE / RANDOM_LONG, both
operand types (e16 itself 5.2e-4 .. 1.0e-3 in fp16, 3.9e-3 .. 8.1e-3 in bf16):

    kernel   p_after_norm (max / rms)   pv_block32      online32        F_max  F_rms
    dense    1.772 / 1.332              1.000 / 1.000   --              3.7    2.8
    long     --                         1.000 / 1.000   1.033 / 0.988   2.2    2.1

A third figure, ``bias_ratio``: that bar is one output rounding wide, and a P that is TRUNCATED instead of rounded stays at 0.2 .. 0.6 of it (the CPU
test shows it).  What truncation does is pull every output towards zero by about a third of an ulp of T.  T = sum err sign(exact) / sum |exact|
measures exactly that, its standard error under zero-mean rounding is se = rms(err) / (sqrt(n) mean |exact|), and the random cases ask
|T(got)| <= |T(plain16)| + 6 se(plain16): the reference's own statistic plus six of its standard errors.  Truncated P: 4 .. 15 x that.
"""
import functools
from typing import NamedTuple

import torch

from tests.backward_primitive_refs import F32, F64, SUB_T, U_T, f32_scalar, gen

OPERAND_DTYPES = [torch.float16, torch.bfloat16]
MASK_BIAS = -30000.0          # FVIT_MASK_BIAS
OFF = -1000.0                 # the bias of a key that must not be selected
GAP = 110.0
F_MAX = {"dense": 3.7, "long": 2.2}
F_RMS = {"dense": 2.8, "long": 2.1}
STUDY_SEEDS = (0, 1, 2, 3)
NWIN, HEADS = 3, 3            # 9 items: a tail for 4 (single-term) and for 2 (two-term) items per workgroup
VARIANTS = {"dense": {"p_after_norm": dict(p_after_norm=True), "pv_block32": dict(pv_block=32)},
            "long": {"pv_block32": dict(pv_block=32), "online32": dict(online=32)}}


def spad(S):
    """fvit_attention_spad (fvit_api.hip): the instance SB the dense kernel runs and the side of its bias table."""
    sb = (S + 15) // 16
    sb = 10 if sb == 9 else 13 if sb in (11, 12) else sb
    return sb * 16


class Dense(NamedTuple):
    S: int
    dpad: int
    d: int


def dense_id(c):
    return f"S{c.S}-sb{spad(c.S) // 16}-dp{c.dpad}-d{c.d}"


# every instance SB in {1..8, 10, 13}: S = 16 SB and 16 (SB - 1) + 1; the remaps 9 -> 10 (129, 144) and 11, 12 -> 13 (161, 192)
DENSE_S = sorted({16 * sb for sb in (1, 2, 3, 4, 5, 6, 7, 8, 10, 13)} | {16 * (sb - 1) + 1 for sb in (1, 2, 3, 4, 5, 6, 7, 8, 10, 13)} | {129, 144, 161, 192})
DENSE_CASES = [Dense(S, dp, d) for dp, d in ((32, 32), (32, 24), (64, 49), (96, 80)) for S in DENSE_S if dp < 96 or S <= 128]
NOT_DENSE = Dense(129, 96, 80)        # dpad 96 beyond 128 tokens: the long kernel's geometry, refused by every dense unit entry point


class Long(NamedTuple):
    S: int
    w: int
    ng: int


# S % 64 in {0, 1, 17, 33}, S % 32 in {0, 1, 17}; at most NWIN_LONG x HEADS_LONG = 4 items
LONG_CASES = [Long(1, 1, 0), Long(33, 5, 8), Long(64, 8, 0), Long(65, 8, 1), Long(209, 14, 13), Long(257, 16, 1), Long(289, 17, 0)]
LONG_DP = [(32, 32), (64, 49), (96, 80)]
NWIN_LONG, HEADS_LONG = 2, 2
# rounding-level cases: three S per kernel from the lists above
RANDOM_DENSE = [Dense(49, 32, 32), Dense(129, 64, 49), Dense(113, 96, 80)]
RANDOM_LONG = [(Long(65, 8, 1), 32, 32), (Long(209, 14, 13), 64, 49), (Long(289, 17, 0), 96, 80)]


def long_id(c):
    return f"S{c.S}-w{c.w}-ng{c.ng}"


def corners(w):
    return [(0, 0), (w - 1, w - 1), (-(w - 1), 0), (0, -(w - 1))]


# ------------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------------------
def rand_v(g, shape, dt):
    """Random values of T with full mantissas (float32 tensor)."""
    return (torch.randn(shape, generator=g) * 1.5).to(dt).float()


def v_two_term(g, shape, dt):
    """(hi, lo) of a random x32 on a 2^-20 grid with |x32| < 4: hi = round_T(x32), lo = round_T(x32 - hi); hi + lo is exact in fp32."""
    x = ((torch.randn(shape, generator=g) * 1.2).clamp(-3.9, 3.9) * 2 ** 20).round() / 2 ** 20
    hi = x.to(dt).float()
    lo = (x - hi).to(dt).float()
    # a lo that rounded up to exactly half an ulp of hi would make round_T(hi + lo) a tie: those elements carry x32 = hi (lo = 0) instead
    lo = torch.where((hi + lo).to(dt).float() == hi, lo, torch.zeros(()))
    return hi, lo


def perms(g, nwin, heads, S):
    """[heads][S]: another permutation of the keys per head (shared by the windows, as the bias table is)."""
    return torch.stack([torch.randperm(S, generator=g) for _ in range(heads)])


def table_bias(perm, S, sp):
    """[heads][sp][sp] f32: 0 at (q, perm[h][q]), OFF on the other valid keys, MASK_BIAS on key columns >= S, 0 on query rows >= S."""
    heads = perm.shape[0]
    b = torch.full((heads, sp, sp), OFF)
    b[:, :, S:] = MASK_BIAS
    b[:, S:, :] = 0.0
    b[torch.arange(heads)[:, None], torch.arange(S)[None, :], perm] = 0.0
    return b


def zero_bias(heads, S, sp):
    b = torch.zeros(heads, sp, sp)
    b[:, :S, S:] = MASK_BIAS
    return b


def codes(S, d):
    """[S][d] of -1 / +1: the 8 bits of the index, then d - 8 hashed bits."""
    assert S <= 256 and d >= 8
    j = torch.arange(S)
    bits = [(j >> b) & 1 for b in range(8)] + [((j * 2654435761 + 40503 * (b + 1) * (j + 7)) >> (5 + b % 11)) & 1 for b in range(d - 8)]
    return torch.stack(bits, 1).float() * 2 - 1


def qk_selector(perm, S, d):
    """q [heads][S][d] = 64 c_perm(i), k [S][d] = c_j."""
    c = codes(S, d)
    return 64.0 * c[perm], c


def selector_gap(q, k, bias, scale, S):
    """Smallest distance between the best and the second-best score of a valid query row, over all the keys the kernel sums (bias [heads][>= S][nk],
    q / k [nwin][heads][S][d]; keys >= S have k = 0)."""
    nk = bias.shape[-1]
    k = torch.cat([k.double(), torch.zeros(*k.shape[:-2], nk - S, k.shape[-1], dtype=F64)], -2)
    s = (q.double() @ k.transpose(-1, -2)) * scale + bias[:, :S, :].double()
    if nk == 1:
        return float("inf")
    top = s.topk(2, -1).values
    return (top[..., 0] - top[..., 1]).min().item()


def rel_dense(tab, w, ng, S):
    """[heads][S][S] bias the way the reference gathers the compact table (FV:243-258, 276-299): token ng + y w + x; 0 on the ng leading tokens."""
    heads, tw = tab.shape[0], 2 * w - 1
    l = torch.arange(S - ng)
    y, x = l // w, l % w
    idx = (y[:, None] - y[None, :] + w - 1) * tw + (x[:, None] - x[None, :] + w - 1)
    b = torch.zeros(heads, S, S, dtype=tab.dtype)
    b[:, ng:, ng:] = tab[:, idx]
    return b


def disp_table(w, disps):
    """[len(disps)][(2w-1)^2]: 0 at each head's displacement (dy, dx) = (yq - yk, xq - xk), OFF elsewhere."""
    tw = 2 * w - 1
    t = torch.full((len(disps), tw * tw), OFF)
    for h, (dy, dx) in enumerate(disps):
        t[h, (dy + w - 1) * tw + dx + w - 1] = 0.0
    return t


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _narrow(t, dt, trunc=False):
    if dt is None:
        return t
    r = t.to(dt)
    if trunc:       # towards zero (the values are >= 0): one step down wherever rounding went up
        i16 = r.view(torch.int16)
        r = torch.where(r.float() > t, (i16 - 1), i16).view(dt)
    return r.float()


def attention(q, k, v, bias, scale, dt=None, *, p_after_norm=False, pv_block=None, online=None, mut=None):
    """q, k, v [nwin][heads][S][d] (values of T), bias [heads][S][>= S] over the keys that take part (a dense table's pad columns may be included:
    their k and v rows are then zero).  dt None: float64, nothing rounded.  Otherwise float32 with P and then o narrowed to dt."""
    ft = F64 if dt is None else F32
    q, k, v, bias = q.to(ft), k.to(ft), v.to(ft), bias.to(ft)
    nk = bias.shape[-1]
    if nk > k.shape[-2]:
        pad = torch.zeros(*k.shape[:-2], nk - k.shape[-2], k.shape[-1], dtype=ft)
        k, v = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
    s = (q @ k.transpose(-1, -2)) * scale + bias
    trunc = mut == "p_trunc"
    if online:
        m = torch.full(s.shape[:-1], -3.0e38, dtype=ft)
        lsum = torch.zeros_like(m)
        o = torch.zeros(*s.shape[:-1], v.shape[-1], dtype=ft)
        for k0 in range(0, nk, online):
            st = s[..., k0:k0 + online]
            mn = torch.maximum(m, st.max(-1).values)
            alpha = torch.exp(m - mn)
            e = torch.exp(st - mn[..., None])
            lsum = lsum * alpha + e.sum(-1)
            o = (o if mut == "no_rescale" else o * alpha[..., None]) + _narrow(e, dt, trunc) @ v[..., k0:k0 + online, :]
            m = mn
        return _narrow(o * (1.0 / lsum)[..., None], dt)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    rs = e.sum(-1, keepdim=True)
    p = _narrow(e / rs, dt, trunc) if p_after_norm else _narrow(e, dt, trunc)
    if pv_block:
        o = sum(p[..., k0:k0 + pv_block] @ v[..., k0:k0 + pv_block, :] for k0 in range(0, nk, pv_block))
    else:
        o = p @ v
    return _narrow(o if p_after_norm else o * (1.0 / rs), dt)


def bound16(exact, plain, dt, f_max):
    exact = exact.to(F64)
    e16 = (plain.to(F64) - exact).abs().max().item()
    return U_T[dt] * exact.abs() + (SUB_T[dt] + f_max * e16)


def _rms(t):
    return t.to(F64).pow(2).mean().sqrt().item()


def ratios(kernel, got, exact, plain, dt):
    """(max |got - exact| / bound, rms(got - exact) / (F_rms rms(round_T(plain16) - exact))): both must be <= 1."""
    got, exact = got.to(F64), exact.to(F64)
    if not torch.isfinite(got).all():
        return float("inf"), float("inf")
    err = got - exact
    base = _rms(plain.to(F64) - exact)
    return (err.abs() / bound16(exact, plain, dt, F_MAX[kernel])).max().item(), _rms(err) / (F_RMS[kernel] * base)


def signed_bias(got, exact):
    """(T, se): T = sum_i err_i sign(exact_i) / sum_i |exact_i|, the systematic relative error of the output, and its standard error under zero-mean
    independent errors, rms(err) / (sqrt(n) mean |exact|).  A P that is truncated instead of rounded scales every output towards zero by about a
    third of an ulp of T: invisible to a per-element bar one rounding wide, but tens of standard errors in T."""
    got, exact = got.to(F64), exact.to(F64)
    err = got - exact
    return (err * exact.sign()).sum().item() / exact.abs().sum().item(), _rms(err) / (err.numel() ** 0.5 * exact.abs().mean().item())


def bias_ratio(got, exact, plain):
    """|T(got)| / (|T(plain16)| + 6 se(plain16)): must be <= 1 (six standard errors of the reference's own statistic, plus its own value)."""
    tg, _ = signed_bias(got, exact)
    tp, se = signed_bias(plain, exact)
    return abs(tg) / (abs(tp) + 6 * se)


def variant_ratios(exact, plain, var):
    ev, eb = var.to(F64) - exact.to(F64), plain.to(F64) - exact.to(F64)
    return ev.abs().max().item() / eb.abs().max().item(), _rms(ev) / _rms(eb)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# case inputs
# ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_selector(c, dt, family, nwin=NWIN, heads=HEADS):
    """q, k, v [nwin][heads][S][d] and lo images (two-term splits), the padded bias table, the selected key per (head, query)."""
    g = gen(30000 + c.S * 11 + c.d + (0 if family == "table" else 5))
    sp = spad(c.S)
    perm = perms(g, nwin, heads, c.S)
    v, v_lo = v_two_term(g, (nwin, heads, c.S, c.d), dt)
    v1 = rand_v(g, (nwin, heads, c.S, c.d), dt)
    if family == "table":
        q = k = torch.zeros(nwin, heads, c.S, c.d)
        bias, scale = table_bias(perm, c.S, sp), f32_scalar(c.d ** -0.5)
    else:
        qh, kc = qk_selector(perm, c.S, c.d)
        q, k = qh[None].expand(nwin, heads, c.S, c.d).contiguous(), kc[None, None].expand(nwin, heads, c.S, c.d).contiguous()
        bias, scale = zero_bias(heads, c.S, sp), 1.0
    return dict(q=q, k=k, v=v1, v_hi=v, v_lo=v_lo, bias=bias, scale=scale, perm=perm, sp=sp)


def gathered(v, perm):
    """out[w][h][q] = v[w][h][perm[h][q]]."""
    return torch.stack([v[:, h, perm[h]] for h in range(perm.shape[0])], 1)


@functools.lru_cache(maxsize=None)
def long_selector(c, d, dt, pair, nwin=NWIN_LONG, heads=HEADS_LONG):
    """pair 0 / 1: the heads take corners (0, 1) / (2, 3).  Returns v (and its two-term split), the compact table, the dense bias, and the fp64 result
    with ``onehot`` [heads][S] marking the queries whose row has a single key at the maximum."""
    g = gen(31000 + c.S * 13 + d + pair)
    disps = corners(c.w)[2 * pair:2 * pair + heads]
    tab = disp_table(c.w, disps)
    bias = rel_dense(tab, c.w, c.ng, c.S)
    v_hi, v_lo = v_two_term(g, (nwin, heads, c.S, d), dt)
    v = rand_v(g, (nwin, heads, c.S, d), dt)
    atmax = bias == bias.max(-1, keepdim=True).values
    return dict(v=v, v_hi=v_hi, v_lo=v_lo, tab=tab, bias=bias, onehot=atmax.sum(-1) == 1, scale=f32_scalar(d ** -0.5), disps=disps)


def equal_rows_lo_interval(v, bias, hi, dt):
    """(lo_min, lo_max, exact) for every row of a long selector case run through the two-term entry: v = v_hi + v_lo [nwin][heads][S][d] (exact in
    fp32), hi the kernel's hi image.  e = (n + 4) 2^-24 mean |v| over the n keys at the row's maximum (module docstring)."""
    atmax = (bias == bias.max(-1, keepdim=True).values).to(F64)                     # [heads][S][S]
    n = atmax.sum(-1, keepdim=True)
    exact = (atmax / n) @ v.to(F64)                                                   # [nwin][heads][S][d]
    e = (n + 4) * 2.0 ** -24 * ((atmax / n) @ v.to(F64).abs())
    lo_min = (exact - e - hi.to(F64)).to(F32).to(dt).float()
    lo_max = (exact + e - hi.to(F64)).to(F32).to(dt).float()
    return lo_min, lo_max, exact


def random_dense(c, dt, seed=0, nwin=NWIN, heads=HEADS):
    g = gen(seed * 7919 + 32000 + c.S * 3 + c.d)
    q, k, v = (torch.randn(nwin, heads, c.S, c.d, generator=g).to(dt).float() for _ in range(3))
    sp = spad(c.S)
    bias = torch.zeros(heads, sp, sp)
    bias[:, :c.S, :c.S] = torch.randn(heads, c.S, c.S, generator=g) * 2
    bias[:, :, c.S:] = MASK_BIAS
    bias[:, c.S:, :] = 0.0
    return dict(q=q, k=k, v=v, bias=bias, scale=f32_scalar(c.d ** -0.5), sp=sp)


def random_long(case, dt, seed=0, nwin=NWIN_LONG, heads=HEADS_LONG):
    c, dpad, d = case
    g = gen(seed * 7919 + 33000 + c.S * 3 + d)
    q, k, v = (torch.randn(nwin, heads, c.S, d, generator=g).to(dt).float() for _ in range(3))
    tab = torch.randn(heads, (2 * c.w - 1) ** 2, generator=g) * 2
    return dict(q=q, k=k, v=v, tab=tab, bias=rel_dense(tab, c.w, c.ng, c.S), scale=f32_scalar(d ** -0.5))
