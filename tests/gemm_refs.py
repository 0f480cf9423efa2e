"""References and case tables for the unit GEMM kernels of csrc/fvit_gemm.hip (gemm_kernel, gemm_pp_kernel, splitk_reduce_kernel), shared by
tests/test_gemm_refs_cpu.py (the conditions under which the cases are exact, and the mutants they catch; no GPU) and tests/test_gpu_gemm_exact.py (the
kernels through the C ABI).  Plain PyTorch on the CPU, nothing else; no constant here comes from a kernel's output.

INTEGER CASES (CASES, ADD_CASES; compared with torch.equal).  A holds {-1, 0, 1}, W {-2 .. 2}, the bias integers with |b| <= 32, and

    max_{m, n} ( sum_k |A[m][k]| |W[n][k]| + |bias[n]| ) <= 256                                                   (``magnitude``)

so every partial sum in ANY order is an integer of magnitude <= 256: exact in fp32, fp16 and bf16.  The recipe: floor(112 / nk) non-zeros (at least
4) per row of A inside each of the nk 64-wide K tiles of the contraction.  K-concatenated terms count as K tiles of their own: K = 2 ka is
a.w_hi + a.w_lo, K = 3 ka the literal three-product sum a_hi.w_hi + a_hi.w_lo + a_lo.w_hi over INDEPENDENT integer images (a swapped or dropped term
changes an integer).  Second condition (``dead_blocks``): every (16 rows x 16 columns x one K tile) block adds a non-zero amount to at least one of its
outputs, so a fragment that misses one K step cannot go unnoticed.

    epilogue 0   16-bit out == the integer result
    epilogue 2   x0 integer, gamma in {0.5, 1, 2, -1} or NULL: the fp32 result is exact; with the add table (fvit_gemm_residual_add) integer rows
    epilogue 1   bias in multiples of 1/8 -> the pre-activation y is exact; out must lie between the T-roundings of gelu64(y) -+ d,
                 d = 5.4e-5 + 4 * 2^-24 * |gelu64(y)|  (5.4e-5: the bound of gelu_fast, fvit_common.h:176, reproduced by scripts/fit_gelu.py;
                 two-term output, gelu_erf: 1.5e-7 in its place)                                                  (``gelu_interval``)
    two-term out W scaled to {-64 .. 64}: |y| reaches thousands and stays < 2^15; hi == round_T(y), lo == y - hi, both exact (``two_term``)

Split-K and the K-order stagger only reorder integer sums and stay equal to the same reference.  Buffers (``operands``): pad rows M .. pad128(M)-1 of
A and N .. pad128(N)-1 of W, and the columns behind K in lda / ldw, hold NaN (the kernels clamp rows to the padded operand and never read behind K);
outputs are NaN wherever the kernel must not write.

RANDOM CASES (RANDOM_CASES; randn operands, epilogues 0 and 2 -- the GELU epilogue's polynomial is held by the interval above).  ``exact`` is float64,
``plain16`` float32 arithmetic with the one narrowing the kernel has (the 16-bit store, fvit_gemm.hip:356 / :586; the bar carries it as
u_T |exact| + sub_T and plain16 stops before it).  The bar is fused_block_refs.out16_bound (epilogue 0) / branch_bound (epilogue 2) with the chain
"gemm": F_max and F_rms are twice the worst ratio of a variant's error (K accumulated in blocks of 16 / of 32: the MFMA K steps) to the base plain16
error of the same case over seeds 0..3, plus 2 %, rounded up to one decimal.  Measured by tests/test_gemm_refs_cpu.py over RANDOM_CASES, both
operand types (e16 itself 9.1e-7 .. 4.4e-6; the same figures with 1 and 8 CPU threads):

    variant    max ratio   rms ratio
    kblock16   1.363       1.078
    kblock32   1.009       0.877         ->  F_max 2.8, F_rms 2.2       (F_max <= 4 is a condition)
"""
import functools
from typing import NamedTuple

import torch

from tests.backward_primitive_refs import F32, F64, gen

OPERAND_DTYPES = [torch.float16, torch.bfloat16]
F_MAX, F_RMS = 2.8, 2.2
STUDY_SEEDS = (0, 1, 2, 3)
NAN = float("nan")
GELU_ABS = {False: 5.4e-5, True: 1.5e-7}     # gelu_fast (fvit_common.h) / gelu_erf, the two-term output
GAMMAS = (0.5, 1.0, 2.0, -1.0)

# route -> (knobs for tests.util.tuned, the launch name prof_records must show with the epilogue number in place of E; a case with K = 3 ka on a route
# that takes the dual K loop appends " x3": ``launch_name``).  The name carries every choice of fvit_gemm.hip's launch_t.
ROUTES = {
    "small":     (dict(gemm256_min_tiles=0), "gemm_kernel<E> 64-row"),
    "row128":    (dict(gemm256_min_tiles=0, gemm_bm64_max_grid=0), "gemm_kernel<E> 128-row"),
    "nw8_64":    (dict(gemm256_min_tiles=0, gemm_nw8_max_grid=400), "gemm_kernel<E> 64-row nw8"),
    "nw8_128":   (dict(gemm256_min_tiles=0, gemm_nw8_max_grid=400, gemm_bm64_max_grid=0), "gemm_kernel<E> 128-row nw8"),
    "big256":    (dict(gemm256_min_tiles=1, gemm_pp=0), "gemm_kernel<E> 256x256"),
    "pp3":       (dict(gemm256_min_tiles=1, gemm_pp=1, gemm_pp_xring=3), "gemm_pp_kernel<E> 256x256"),
    "pp2":       (dict(gemm256_min_tiles=1, gemm_pp=1, gemm_pp_xring=2), "gemm_pp_kernel<E> 256x256 xr2"),
    "x3cat_64":  (dict(gemm256_min_tiles=0, gemm_x3_dual=0), "gemm_kernel<E> 64-row"),
    "sk_64":     (dict(gemm256_min_tiles=0, gemm_splitk=1), "gemm_kernel<2> 64-row split-K"),
    "sk_128":    (dict(gemm256_min_tiles=0, gemm_splitk=1, gemm_bm64_max_grid=0), "gemm_kernel<2> 128-row split-K"),
    "stag_64":   (dict(gemm256_min_tiles=0, gemm_stagger=1), "gemm_kernel<E> 64-row stagger"),
    "stag_128":  (dict(gemm256_min_tiles=0, gemm_stagger=1, gemm_bm64_max_grid=0), "gemm_kernel<E> 128-row stagger"),
}


class Case(NamedTuple):
    route: str
    M: int
    N: int
    ka: int          # activation columns of one term
    terms: int = 1   # K = terms * ka: 1 plain, 2 = a.[w_hi | w_lo], 3 = [a_hi | a_lo] against [w_hi | w_lo | w_hi]

    @property
    def K(self):
        return self.terms * self.ka

    @property
    def nk(self):
        return self.K // 64


def launch_name(c, epilogue):
    """The name launch_t gives the call: the route's, with " x3" where K = 3 ka takes the dual K loop (not with gemm_x3_dual = 0; the ping-pong form
    then runs its two-deep ring whatever gemm_pp_xring says, so " xr2" goes)."""
    name = ROUTES[c.route][1].replace("E", str(epilogue))
    if c.terms == 3 and c.route != "x3cat_64":
        name = name.replace(" xr2", "") + " x3"
    return name


def case_id(c):
    return f"{c.route}-{c.M}-{c.N}-{c.ka}x{c.terms}"


# The smallest shapes that reach each branch.  Rows of the issue's table that provably select the same instance are merged: for a given route the
# instance depends on (operand type, epilogue, terms == 3) only; M, N, K move the grid, the tails and the K loop's trip count.
CASES = [
    # 64-row: M tail inside the first fragment (1, 17), exactly one tile (64), one row in the second (65); N % 64 == 16 column-group skip (16, 80, 144);
    # a single K tile (64: the prologue is the whole loop)
    Case("small", 1, 16, 64), Case("small", 17, 80, 256), Case("small", 64, 144, 64), Case("small", 65, 16, 256), Case("small", 65, 144, 128, 2),
    # 128-row: the clamped residual load min(m, M - 1)
    Case("row128", 127, 48, 128), Case("row128", 129, 272, 576), Case("row128", 300, 48, 576), Case("row128", 129, 272, 64, 2),
    # 8 waves
    Case("nw8_64", 65, 80, 256), Case("nw8_128", 129, 272, 256), Case("nw8_64", 129, 272, 256),
    # 256 x 256 two-stage: a second tile row with one row (257); a wave group wholly beyond M (384 = 256 + 128)
    Case("big256", 257, 272, 256), Case("big256", 384, 272, 832),
    # ping-pong, both activation-ring depths: nk = 4 (the shortest K the route accepts), 5 (odd), 13
    Case("pp3", 257, 272, 256), Case("pp3", 384, 528, 320), Case("pp3", 300, 272, 832),
    Case("pp2", 257, 272, 256), Case("pp2", 384, 528, 320), Case("pp2", 300, 272, 832),
    # x3 dual K loop on the 64-row, 128-row and ping-pong forms, and the K-concatenated walk (gemm_x3_dual = 0)
    Case("small", 65, 144, 64, 3), Case("row128", 300, 272, 64, 3), Case("pp3", 300, 272, 256, 3), Case("pp2", 65, 144, 256, 3),
    Case("x3cat_64", 65, 144, 64, 3), Case("x3cat_64", 300, 272, 256, 3),
    # split-K with uneven K ranges: nk 9 -> 2 splits of 4 + 5 tiles, nk 13 -> 3 splits of 4 + 4 + 5
    Case("sk_64", 70, 144, 576), Case("sk_64", 300, 144, 832), Case("sk_128", 70, 144, 832), Case("sk_128", 300, 144, 576),
    # stagger: rot = (tn * per + tm) % nk wraps (nk 9; 3 column tiles x up to 5 row tiles)
    Case("stag_64", 300, 272, 576), Case("stag_128", 300, 272, 576),
]
# the two-term GELU epilogue once per tile form: its instance depends on (route, operand type, terms == 3) only
TWO_TERM_GELU_CASES = [Case("small", 17, 80, 256), Case("row128", 129, 272, 576), Case("nw8_64", 65, 80, 256), Case("nw8_128", 129, 272, 256),
                       Case("big256", 257, 272, 256), Case("pp3", 257, 272, 256), Case("pp2", 257, 272, 256), Case("small", 65, 144, 64, 3),
                       Case("row128", 300, 272, 64, 3), Case("pp3", 300, 272, 256, 3), Case("x3cat_64", 65, 144, 64, 3)]
# a NaN inside a VALID operand element must come back as NaN in its whole output row, in every epilogue: one case per tile form.  The row's
# other pre-activations are integers as everywhere, so rows around it are still held to equality / the GELU interval.
NAN_CASES = [Case("small", 65, 144, 256), Case("row128", 129, 272, 576), Case("pp3", 257, 272, 256), Case("small", 65, 144, 64, 3)]
GELU_FAST_XMIN = -4.2426405   # fvit_common.h: where the unit GEMM's GELU epilogue holds its argument


def nan_inputs(c, inp):
    """(inputs with A[m0][k0] = NaN in the first image, m0): a row in the last 16-row fragment, a column in the last K tile."""
    m0, k0 = c.M - 1 - (c.M - 1) % 16 // 2, c.ka - 5
    a = [t.clone() for t in inp["a"]]
    a[0][m0, k0] = NAN
    return dict(inp, a=a), m0


# (case, rows_per_image, add_idx kind): rows_per_image does not divide M; add_idx None (row p of the table) or a table with negative (skip) entries
ADD_CASES = [(Case("small", 65, 144, 256), 7, "idx"), (Case("small", 65, 80, 64), 9, None), (Case("row128", 300, 272, 128), 49, "idx"),
             (Case("row128", 129, 48, 128), 50, None), (Case("pp3", 300, 272, 256), 53, "idx"), (Case("pp3", 257, 272, 320), 64, None)]
# (route, M, N, K, epilogue): randn operands
RANDOM_CASES = [("small", 65, 144, 256, 0), ("row128", 300, 272, 576, 2), ("pp3", 300, 528, 832, 0), ("sk_128", 300, 144, 832, 2)]


def epilogues(c):
    return (2,) if c.route.startswith("sk_") else (0, 1, 2)


def pad128(n):
    return (n + 127) // 128 * 128


# ------------------------------------------------------------------------------------------------------------------------------------------------
# integer inputs
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _sparse_signs(g, rows, ka, per_tile):
    """[rows][ka] of {-1, 0, 1} with exactly per_tile non-zeros inside each 64-wide K tile of every row."""
    a = torch.zeros(rows, ka // 64, 64)
    pos = torch.rand(rows, ka // 64, 64, generator=g).argsort(-1)[..., :per_tile]
    sign = torch.randint(0, 2, pos.shape, generator=g).float() * 2 - 1
    a.scatter_(-1, pos, sign)
    return a.view(rows, ka)


def _nonzero_ints(g, shape, lim):
    """Integers in -lim .. lim without 0."""
    v = torch.randint(1, lim + 1, shape, generator=g).float()
    return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


@functools.lru_cache(maxsize=None)
def int_inputs(c, wscale=1):
    """The integer images of a case (float32 tensors holding integers).  a / w: lists of the term images; wscale 32 = the two-term-output cases."""
    g = gen(20000 + c.M * 7 + c.N * 3 + c.K + c.terms * 1000 + len(c.route))
    per = max(4, min(112 // c.nk, 48))
    assert per * c.nk <= 112
    a = [_sparse_signs(g, c.M, c.ka, per) for _ in range(2 if c.terms == 3 else 1)]
    w = [_nonzero_ints(g, (c.N, c.ka), 2) * wscale for _ in range(1 if c.terms == 1 else 2)]
    return dict(a=a, w=w, bias=torch.randint(-32, 33, (c.N,), generator=g).float(), x0=torch.randint(-32, 33, (c.M, c.N), generator=g).float(),
                gamma=torch.tensor(GAMMAS)[torch.randint(0, 4, (c.N,), generator=g)])


def products(c, inp):
    """[(A image, W image)] of the contraction, in K order: the segments of the K-concatenated weight row and the activation columns they meet."""
    a, w = inp["a"], inp["w"]
    return [(a[0], w[0])] if c.terms == 1 else [(a[0], w[0]), (a[0], w[1])] if c.terms == 2 else [(a[0], w[0]), (a[0], w[1]), (a[1], w[0])]


def magnitude(c, inp, bias):
    """max_{m, n} sum_k |A| |W| + |bias|: the bound on every partial sum in any order."""
    return (sum(pa.abs().double() @ pw.abs().double().t() for pa, pw in products(c, inp)) + bias.abs().double()).max().item()


def ktile_contributions(c, inp):
    """[nk][M][N]: what each 64-wide K tile of the contraction adds to each output."""
    return torch.stack([pa[:, k:k + 64].double() @ pw[:, k:k + 64].double().t() for pa, pw in products(c, inp) for k in range(0, c.ka, 64)])


def dead_blocks(c, inp):
    """Number of (16 rows x 16 columns x K tile) blocks that add zero to every one of their outputs."""
    t = ktile_contributions(c, inp)
    nk, M, N = t.shape
    Mp = (M + 15) // 16 * 16
    t = torch.cat([t, torch.zeros(nk, Mp - M, N, dtype=t.dtype)], 1).view(nk, Mp // 16, 16, N // 16, 16)
    # a block with rows beyond M only counts its valid rows: the row block always holds at least one
    return int(((t != 0).sum((2, 4)) == 0).sum())


def accumulate(c, inp, mut=None):
    """float64 [M][N] sum over the products, no bias.  Mutants: see tests/test_gemm_refs_cpu.py."""
    pr = products(c, inp)
    if mut == "a_col_wrong_term":        # the second term reads A column k instead of k - ka: the lo image of an x3 row
        pr[1] = (inp["a"][1], pr[1][1])
    elif mut == "drop_lo_hi":
        pr = pr[:2]
    acc = sum(pa.double() @ pw.double().t() for pa, pw in pr)
    if mut == "drop_ktile":              # the last 16 x 16 fragment misses the last K tile
        t = ktile_contributions(c, inp)[-1]
        r0, c0 = (c.M - 1) // 16 * 16, c.N - 16
        acc[r0:, c0:] -= t[r0:, c0:]
    elif mut == "pad_row_leak":          # the last valid row of A is read from the (zero-treated) pad row behind it
        acc[c.M - 1] = 0.0
    return acc


def gelu64(y):
    y = y.double()
    return 0.5 * y * (1.0 + torch.erf(y * 0.70710678118654752440))


def exact(c, inp, epilogue, *, gamma=True, add=None, add_idx=None, rpi=1, mut=None):
    """float64 result of one call on the integer images: epilogue 0 / 1 the value before the 16-bit store (1: gelu64 of bias / 8), 2 the new x."""
    acc = accumulate(c, inp, mut)
    if epilogue == 1:
        return gelu64(acc + inp["bias"].double() / 8)
    if epilogue == 0:
        out = acc + inp["bias"].double()
        if mut == "skip_last_colgroup":
            out[:, -16:] = NAN
        return out
    gam = inp["gamma"].double() if gamma else torch.ones(c.N, dtype=F64)
    out = inp["x0"].double() + (gam * acc + inp["bias"].double() if mut == "gamma_not_on_bias" else gam * (acc + inp["bias"].double()))
    if add is not None:
        p = torch.arange(c.M) if mut == "add_row_of_m" else torch.arange(c.M) % rpi
        if mut == "add_row_of_m":
            p = p.clamp(max=(add_idx.numel() if add_idx is not None else add.shape[0]) - 1)
        ai = p if add_idx is None else add_idx[p]
        out = out + torch.where((ai >= 0)[:, None], add.double()[ai.clamp(min=0)], torch.zeros((), dtype=F64))
    return out


def add_inputs(c, rpi, kind):
    g = gen(21000 + c.M + c.N + rpi)
    rows = rpi + 3
    add = torch.randint(-16, 17, (rows, c.N), generator=g).float()
    idx = None
    if kind == "idx":
        idx = torch.randperm(rows, generator=g)[:rpi].int()
        idx[torch.randperm(rpi, generator=g)[:max(1, rpi // 4)]] = -1
        idx[0] = -3                       # any negative value means "none"
    return add, idx


def gelu_interval(y, dt, two_term=False):
    """(lo, hi) float32 tensors of T values: the T-roundings of gelu64(y) -+ d."""
    gl = gelu64(y)
    d = GELU_ABS[two_term] + 4 * 2.0 ** -24 * gl.abs()
    return (gl - d).to(F32).to(dt).float(), (gl + d).to(F32).to(dt).float()


def two_term(y, dt):
    """(hi, lo) of an exact float64 y: hi = round_T(y), lo = y - hi (asserted representable by the CPU test)."""
    hi = y.to(F32).to(dt).double()
    return hi, y - hi


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the buffers of one call
# ------------------------------------------------------------------------------------------------------------------------------------------------
def strides(c, wide, epilogue, lo_out=False):
    """(lda, ldw, ldo, out_lo_off): the minimum, or (wide) lda = K + 8, ldw = K + 16, ldo = N + 8 (16-bit) / N + 4 (fp32)."""
    acols = (2 if c.terms == 3 else 1) * c.ka
    lda, ldw = (acols + 8, c.K + 16) if wide else (acols, c.K)
    if epilogue == 2:
        return lda, ldw, c.N + 4 if wide else c.N, 0
    if lo_out:
        off = c.N + 8 if wide else c.N
        return lda, ldw, off + c.N + (8 if wide else 0), off
    return lda, ldw, c.N + 8 if wide else c.N, 0


def operands(c, inp, dt, lda, ldw):
    """(A [pad128(M)][lda], W [pad128(N)][ldw]) in the operand type, NaN in the pad rows and behind the valid columns."""
    A = torch.full((pad128(c.M), lda), NAN, dtype=dt)
    W = torch.full((pad128(c.N), ldw), NAN, dtype=dt)
    for i, img in enumerate(inp["a"]):
        A[:c.M, i * c.ka:(i + 1) * c.ka] = img.to(dt)
    wimgs = inp["w"] if c.terms < 3 else [inp["w"][0], inp["w"][1], inp["w"][0]]
    for i, img in enumerate(wimgs):
        W[:c.N, i * c.ka:(i + 1) * c.ka] = img.to(dt)
    return A, W


# ------------------------------------------------------------------------------------------------------------------------------------------------
# random-value cases
# ------------------------------------------------------------------------------------------------------------------------------------------------
def random_inputs(case, dt, seed=0):
    route, M, N, K, epilogue = case
    g = gen(seed * 7919 + 22000 + M + N * 3 + K)
    return dict(dt=dt, A=torch.randn(M, K, generator=g).to(dt).float(), W=(torch.randn(N, K, generator=g) / K ** 0.5).to(dt).float(),
                bias=torch.randn(N, generator=g), gamma=torch.rand(N, generator=g) + 0.5, x0=torch.randn(M, N, generator=g) * 1.3)


def random_value(inp, epilogue, dtype=F64, kblock=None):
    """The epilogue's value before any 16-bit store -- epilogue 0: A W^T + bias; 2: the branch gamma * (A W^T + bias) -- in float64 (``exact``) or in
    float32 (``plain16``), optionally with K accumulated block by block."""
    A, Wt = inp["A"].to(dtype), inp["W"].to(dtype).t()
    if kblock:
        acc = None
        for k0 in range(0, A.shape[1], kblock):
            part = A[:, k0:k0 + kblock] @ Wt[k0:k0 + kblock]
            acc = part if acc is None else acc + part
    else:
        acc = A @ Wt
    y = acc + inp["bias"].to(dtype)
    return y if epilogue == 0 else inp["gamma"].to(dtype) * y
