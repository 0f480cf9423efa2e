"""Every memory-bound backward primitive of csrc/fvit_bwd.hip, the short attention backward, the train-mode attention forward and the two GEMM forms
only the backward uses -- each called on its own through the C ABI (needs an MI355X) and held to float64 (tests/backward_primitive_refs.py: the
references, the case table and the one bar ``bound``; tests/test_backward_primitive_refs_cpu.py shows that an ordinary fp32 evaluation meets that bar
on these very inputs).

Conventions of this file: every OUTPUT buffer is larger than what the kernel may write (spare rows, pad columns up to the stride) and starts as NaN;
after the call everything outside the documented written region must still be NaN.  Every INPUT's pad columns (logical width .. stride) are NaN, so
a kernel that reads them poisons its result -- except the bias table and the attn_drop mask, whose pad region the callers define (FVIT_MASK_BIAS /
zero, as hat_backward fills them) and the head-padding channels d .. D-1 of qkv / dO, which the layout defines as zero.  Each value test prints its
worst |err| / bound per tensor; 1.0 is the bar."""
import ctypes

import pytest
import torch

from fastervit_amd import _lib
from tests import backward_primitive_refs as R
from tests.test_gpu_backward_long import LONG_BAR, LONG_BIAS_BAR

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 1, torch.bfloat16: 2}
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
DTS = pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=["f16", "bf16"])


def _rup(x, m):
    return (x + m - 1) // m * m


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _embed(t, ld, dt, rows=None):
    """The 2-D values ``t`` as a [rows][ld] device buffer of type ``dt``; everything outside t's extent is NaN."""
    buf = _nan((rows or t.shape[0], ld), dt)
    buf[:t.shape[0], :t.shape[1]] = t.to(dt).cuda()
    return buf


def _untouched(buf, rows, cols, what):
    """Only buf[:rows] -- and of a 2-D buffer with ``cols`` given only buf[:rows, :cols] -- may have been written."""
    b = buf.float()
    assert torch.isnan(b[rows:]).all(), f"{what}: rows beyond {rows} were written"
    if cols is not None:
        assert torch.isnan(b[:rows, cols:]).all(), f"{what}: columns beyond {cols} were written"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _under_bar(name, checks):
    """checks: [(tensor name, kernel output, exact, plain32, output dtype)].  Prints the worst |err| / bound of each tensor, then asserts them all."""
    worst = [(key, R.worst_ratio(got, exact, plain, odt)) for key, got, exact, plain, odt in checks]
    print(f"{name}: worst |err|/bound " + " ".join(f"{k}={v:.3f}" for k, v in worst))
    for key, v in worst:
        assert v <= 1.0, f"{name} {key}: {v:.3f} x the bar"
    return max(v for _, v in worst)


def _finish(lib, part_ptr, blocks, stride, out, n, accumulate):
    _lib.check(lib.fvit_bwd_colsum_finish(part_ptr, blocks, stride, out.data_ptr(), n, accumulate, _stream()), "colsum_finish")


# ------------------------------------------------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("M,N", R.TRANSPOSE_SHAPES)
def test_transpose16_is_bitwise_and_zero_fills_its_pad_columns(M, N, dt):
    lib = _lib.lib()
    src = R.rounded(torch.randn(M, N, generator=R.gen(M * 31 + N)), dt)
    for ld_in in (_rup(N, 8), _rup(N, 8) + 24):
        for ld_out in (_rup(M, 64), _rup(M, 64) + 64):
            a = _embed(src, ld_in, dt)
            out = _nan((N + 3, ld_out), dt)
            _lib.check(lib.fvit_bwd_transpose16(CODE[dt], a.data_ptr(), ld_in, out.data_ptr(), ld_out, M, N, _stream()), "transpose16")
            torch.cuda.synchronize()
            what = f"transpose16 M={M} N={N} ld_in={ld_in} ld_out={ld_out}"
            assert torch.equal(_bits(out[:N, :M]), _bits(a[:M, :N].t())), what
            assert (_bits(out[:N, M:]) == 0).all(), f"{what}: columns M .. ld_out-1 of the written rows must be +0"
            _untouched(out, N, ld_out, what)


@DTS
@pytest.mark.parametrize("C", R.SCALE_COLS_C)
@pytest.mark.parametrize("M", R.SCALE_COLS_M)
def test_scale_cols(M, C, dt):
    lib = _lib.lib()
    blocks = lib.fvit_bwd_blocks(M)
    assert blocks == (M + 63) // 64
    wide = _rup(C, 64) + 64
    for with_gamma, ldz, lddz in ((True, C, wide), (False, wide, C), (True, wide, wide), (False, C, C)):
        dy, z, gamma = R.scale_cols_inputs(M, C, dt, with_gamma)
        exact, plain = R.scale_cols.exact(dy, z, gamma), R.scale_cols.plain32(dy, z, gamma)
        zb, dz = _embed(z, ldz, dt), _nan((M + 2, lddz), dt)
        part = _nan((blocks + 1, 2, C), F32)
        gd = gamma.cuda() if with_gamma else None
        _lib.check(lib.fvit_bwd_scale_cols(CODE[dt], dy.cuda().data_ptr(), zb.data_ptr(), ldz, _p(gd), dz.data_ptr(), lddz, part.data_ptr(), M, C, _stream()),
                   "scale_cols")
        dgamma, dbias = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        _finish(lib, part.data_ptr(), blocks, 2 * C, dgamma, C, 1)
        _finish(lib, part.data_ptr() + 4 * C, blocks, 2 * C, dbias, C, 1)
        torch.cuda.synchronize()
        what = f"scale_cols M={M} C={C} {dt} gamma={with_gamma} ldz={ldz} lddz={lddz}"
        # one correctly rounded fp32 product and one round-to-nearest conversion on both sides
        assert torch.equal(_bits(dz[:M, :C].cpu()), _bits(plain["dz"].to(dt))), f"{what}: dz is not (gamma * dy in fp32) rounded to the operand type"
        _untouched(dz, M, C, what + " dz")
        _untouched(part, blocks, None, what + " part")
        _under_bar(what, [("part", part[:blocks], exact["part"], plain["part"], F32), ("dgamma", dgamma, exact["dgamma"], plain["dgamma"], F32),
                          ("dbias", dbias, exact["dbias"], plain["dbias"], F32)])


@DTS
@pytest.mark.parametrize("H", R.GELU_H)
@pytest.mark.parametrize("M", R.GELU_M)
def test_gelu_forward_and_backward(M, H, dt):
    lib = _lib.lib()
    blocks = lib.fvit_bwd_blocks(M)
    a, dh = R.gelu_inputs(M, H, dt)
    f_exact, f_plain = R.gelu_fwd.exact(a), R.gelu_fwd.plain32(a)
    b_exact, b_plain = R.gelu_bwd.exact(a, dh), R.gelu_bwd.plain32(a, dh)
    for ld in (H, H + 64):
        ab, dhb = _embed(a, ld, dt), _embed(dh, ld, dt)
        h, da = _nan((M + 2, ld), dt), _nan((M + 2, ld), dt)
        part = _nan((blocks + 1, H), F32)
        _lib.check(lib.fvit_bwd_gelu(CODE[dt], ab.data_ptr(), ld, None, 0, h.data_ptr(), ld, None, M, H, _stream()), "gelu")
        _lib.check(lib.fvit_bwd_gelu(CODE[dt], ab.data_ptr(), ld, dhb.data_ptr(), ld, da.data_ptr(), ld, part.data_ptr(), M, H, _stream()), "gelu_bwd")
        torch.cuda.synchronize()
        what = f"gelu M={M} H={H} {dt} ld={ld}"
        _untouched(h, M, H, what + " out")
        _untouched(da, M, H, what + " da")
        _untouched(part, blocks, None, what + " part")
        _under_bar(what, [("gelu", h[:M, :H], f_exact["out"], f_plain["out"], dt), ("da", da[:M, :H], b_exact["out"], b_plain["out"], dt),
                          ("part", part[:blocks], b_exact["part"], b_plain["part"], F32)])


@pytest.mark.parametrize("with_dy", [True, False], ids=["dy", "nody"])
@pytest.mark.parametrize("M,C", R.LAYERNORM_SHAPES)
def test_layernorm_backward(M, C, with_dy):
    lib = _lib.lib()
    blocks = lib.fvit_bwd_blocks(M)
    x, dxn, dy, w, eps = R.layernorm_inputs(M, C)
    dy = dy if with_dy else None
    exact, plain = R.layernorm.exact(x, dxn, dy, w, eps), R.layernorm.plain32(x, dxn, dy, w, eps)
    dx, stats, part = _nan((M + 2, C), F32), _nan((M + 2, 2), F32), _nan((blocks + 1, 2, C), F32)
    xd, dxnd, wd, dyd = x.cuda(), dxn.cuda(), w.cuda(), (dy.cuda() if with_dy else None)
    _lib.check(lib.fvit_bwd_layernorm(xd.data_ptr(), dxnd.data_ptr(), _p(dyd), wd.data_ptr(), ctypes.c_float(eps), dx.data_ptr(), stats.data_ptr(),
                                      part.data_ptr(), M, C, _stream()), "layernorm_bwd")
    dw, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    _finish(lib, part.data_ptr(), blocks, 2 * C, dw, C, 1)
    _finish(lib, part.data_ptr() + 4 * C, blocks, 2 * C, db, C, 1)
    torch.cuda.synchronize()
    what = f"layernorm M={M} C={C} dy={with_dy}"
    for buf, name in ((dx, "dx"), (stats, "stats"), (part, "part")):
        _untouched(buf, blocks if name == "part" else M, None, f"{what} {name}")
    _under_bar(what, [("dx", dx[:M], exact["dx"], plain["dx"], F32), ("stats", stats[:M], exact["stats"], plain["stats"], F32),
                      ("part", part[:blocks], exact["part"], plain["part"], F32), ("dw", dw, exact["dw"], plain["dw"], F32),
                      ("db", db, exact["db"], plain["db"], F32)])


@DTS
@pytest.mark.parametrize("N", R.COLSUM16_N)
@pytest.mark.parametrize("M", R.COLSUM16_M)
def test_colsum16(M, N, dt):
    lib = _lib.lib()
    blocks = lib.fvit_bwd_blocks(M)
    t = R.colsum16_inputs(M, N, dt)
    exact, plain = R.colsum16.exact(t), R.colsum16.plain32(t)
    for ld in (_rup(N, 8), _rup(N, 8) + 64):
        tb = _embed(t, ld, dt)
        part = _nan((blocks + 1, N), F32)
        _lib.check(lib.fvit_bwd_colsum16(CODE[dt], tb.data_ptr(), ld, part.data_ptr(), M, N, _stream()), "colsum16")
        total = torch.zeros(N, device="cuda")
        _finish(lib, part.data_ptr(), blocks, N, total, N, 1)
        torch.cuda.synchronize()
        what = f"colsum16 M={M} N={N} {dt} ld={ld}"
        _untouched(part, blocks, None, what)
        _under_bar(what, [("part", part[:blocks], exact["part"], plain["part"], F32), ("total", total, exact["total"], plain["total"], F32)])


@pytest.mark.parametrize("n", R.FINISH_N)
@pytest.mark.parametrize("blocks", R.FINISH_BLOCKS)
def test_colsum_finish_sets_or_accumulates(blocks, n):
    lib = _lib.lib()
    part, out0 = R.finish_inputs(blocks, n)
    for stride in (n, 2 * n + 3):
        pb = _embed(part, stride, F32)                                      # NaN between n and the stride
        results = []
        for _ in range(2):
            fresh = _nan((n + 5,), F32)                                     # accumulate = 0 must not read what is there
            acc = _nan((n + 5,), F32)
            acc[:n] = out0.cuda()
            _finish(lib, pb.data_ptr(), blocks, stride, fresh, n, 0)
            _finish(lib, pb.data_ptr(), blocks, stride, acc, n, 1)
            torch.cuda.synchronize()
            results.append((fresh.clone(), acc.clone()))
        (fresh, acc), (fresh2, acc2) = results
        what = f"colsum_finish blocks={blocks} n={n} stride={stride}"
        assert torch.isnan(fresh[n:]).all() and torch.isnan(acc[n:]).all(), f"{what}: entries beyond n were written"
        assert torch.equal(fresh[:n], fresh2[:n]) and torch.equal(acc[:n], acc2[:n]), f"{what}: not bit-reproducible"
        _under_bar(what, [("set", fresh[:n], R.colsum_finish.exact(part)["out"], R.colsum_finish.plain32(part)["out"], F32),
                          ("accumulate", acc[:n], R.colsum_finish.exact(part, out0)["out"], R.colsum_finish.plain32(part, out0)["out"], F32)])


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the attention core
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _rows_of(t, D):
    """(nwin, heads, S, d) -> [nwin * S][heads][D] with zero head-padding channels."""
    nwin, heads, S, d = t.shape
    out = torch.zeros(nwin * S, heads, D)
    out[:, :, :d] = t.permute(0, 2, 1, 3).reshape(nwin * S, heads, d)
    return out


def _pack_qkv(q, k, v, D, ld, dt):
    rows = q.shape[0] * q.shape[2]
    return _embed(torch.stack([_rows_of(t, D) for t in (q, k, v)], 1).reshape(rows, -1), ld, dt, rows=_rup(rows, 128))


def _pack_o(do, D, ldo, dt):
    rows = do.shape[0] * do.shape[2]
    return _embed(_rows_of(do, D).reshape(rows, -1), ldo, dt, rows=_rup(rows, 128))


def _bias_table(lib, bias, heads, S):
    """[heads][spad][spad] as hat_backward._Core fills it: the bias, FVIT_MASK_BIAS on key columns >= S, zero elsewhere."""
    spad = lib.fvit_attention_spad(S)
    assert spad >= S
    tab = torch.zeros(heads, spad, spad)
    if bias is not None:
        tab[:, :S, :S] = bias
    tab[:, :, S:] = _lib.FVIT_MASK_BIAS
    return tab.cuda(), spad


def _mask_buffer(mask, spad, dt):
    """[nwin * heads][S][spad], pad columns zero (hat_backward.drop_path_masks draws it at the padded stride)."""
    nwin, heads, S, _ = mask.shape
    buf = torch.zeros(nwin * heads, S, spad)
    buf[:, :, :S] = mask.reshape(nwin * heads, S, S)
    return buf.to(dt).cuda()


def _unpack(buf, nwin, S, heads, D, d, sections):
    """[rows][ld] -> ``sections`` tensors (nwin, heads, S, d); the head-padding channels d .. D-1 must be exactly zero."""
    t = buf[:nwin * S, :sections * heads * D].float().cpu().contiguous().view(nwin, S, sections, heads, D)
    assert torch.isfinite(t).all()
    assert (t[..., d:] == 0).all(), "head-padding channels must receive exactly zero"
    return [t[:, :, i, :, :d].permute(0, 2, 1, 3) for i in range(sections)]


@DTS
@pytest.mark.parametrize("variant", R.ATTENTION_VARIANTS)
@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=lambda c: "x".join(map(str, c)))
def test_short_attention_backward(case, variant, dt):
    lib = _lib.lib()
    nwin, S, heads, d, D = case
    rows = nwin * S
    q, k, v, do, scale, bias, mask = R.attention_inputs(case, dt, variant)
    exact, plain = R.attention.exact(q, k, v, do, scale, bias, mask), R.attention.plain32(q, k, v, do, scale, bias, mask)
    btab, spad = (None, 0) if bias is None else _bias_table(lib, bias, heads, S)
    mbuf = None
    if mask is not None:
        mbuf = _mask_buffer(mask, spad, dt)
    want_part = variant != "bias_nopart"
    for ld, ldo in ((3 * heads * D, heads * D), (_rup(3 * heads * D, 64) + 64, _rup(heads * D, 64) + 64)):
        qkv, dO = _pack_qkv(q, k, v, D, ld, dt), _pack_o(do, D, ldo, dt)
        dqkv = _nan((rows + 2, ld), dt)
        part = _nan((nwin + 1, heads, S, S), F32) if want_part else None
        if mbuf is None:      # the entry point without a mask argument
            rc = lib.fvit_bwd_window_attention(CODE[dt], qkv.data_ptr(), ld, dO.data_ptr(), ldo, _p(btab), spad, ctypes.c_float(scale), dqkv.data_ptr(),
                                               _p(part), nwin, S, heads, D, _stream())
        else:
            rc = lib.fvit_bwd_window_attention_drop(CODE[dt], qkv.data_ptr(), ld, dO.data_ptr(), ldo, _p(btab), spad, ctypes.c_float(scale), dqkv.data_ptr(),
                                                    _p(part), nwin, S, heads, D, mbuf.data_ptr(), _stream())
        _lib.check(rc, "fvit_bwd_window_attention")
        torch.cuda.synchronize()
        what = f"attention backward {case} {variant} {dt} ld={ld} ldo={ldo}"
        _untouched(dqkv, rows, 3 * heads * D, what)
        gq, gk, gv = _unpack(dqkv, nwin, S, heads, D, d, 3)
        checks = [(n, g, exact[n], plain[n], dt) for n, g in (("dq", gq), ("dk", gk), ("dv", gv))]
        if want_part:
            _untouched(part, nwin, None, what + " dbias_part")
            checks.append(("dbias_part", part[:nwin], exact["ds"], plain["ds"], F32))     # every [window][head] slab, not their sum
        _under_bar(what, checks)


@DTS
@pytest.mark.parametrize("case", R.ATTENTION_FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_train_mode_attention_forward(case, dt):
    lib = _lib.lib()
    nwin, S, heads, d, D = case
    rows = nwin * S
    q, k, v, _, scale, bias, mask = R.attention_inputs(case, dt, "bias_drop", forward=True)
    ref = R.attention.forward(q, k, v, scale, bias, mask, F64)
    btab, spad = _bias_table(lib, bias, heads, S)
    mbuf = _mask_buffer(mask, spad, dt)
    bar = (4e-3 if dt == torch.float16 else 2.5e-2) * max(ref.abs().max().item(), 1.0)     # test_window_attention's: this kernel rounds P to 16 bits
    for ldq, ldo in ((3 * heads * D, heads * D), (_rup(3 * heads * D, 64) + 64, _rup(heads * D, 64) + 64)):
        qkv = _pack_qkv(q, k, v, D, ldq, dt)
        out, plain_drop, plain_fwd = (_nan((rows + 2, ldo), dt) for _ in range(3))
        _lib.check(lib.fvit_window_attention_drop(CODE[dt], qkv.data_ptr(), ldq, out.data_ptr(), ldo, btab.data_ptr(), nwin, S, heads, D, ctypes.c_float(scale),
                                                  mbuf.data_ptr(), _stream()), "attention_drop")
        _lib.check(lib.fvit_window_attention_drop(CODE[dt], qkv.data_ptr(), ldq, plain_drop.data_ptr(), ldo, btab.data_ptr(), nwin, S, heads, D,
                                                  ctypes.c_float(scale), None, _stream()), "attention_drop without a mask")
        _lib.check(lib.fvit_window_attention(CODE[dt], qkv.data_ptr(), ldq, plain_fwd.data_ptr(), ldo, btab.data_ptr(), nwin, S, heads, D, ctypes.c_float(scale),
                                             _stream()), "attention")
        torch.cuda.synchronize()
        what = f"attention forward with attn_drop {case} {dt} ldq={ldq} ldo={ldo}"
        for buf in (out, plain_drop, plain_fwd):
            _untouched(buf, rows, heads * D, what)
        (got,) = _unpack(out, nwin, S, heads, D, d, 1)
        err = (got.double() - ref).abs().max().item()
        print(f"{what}: max |err| {err:.3e}, bar {bar:.3e}")
        assert err < bar, what
        assert torch.equal(_bits(plain_drop[:rows, :heads * D]), _bits(plain_fwd[:rows, :heads * D])), f"{what}: drop_mask = NULL must be fvit_window_attention"


@DTS
def test_long_attention_backward_at_the_product_strides_of_one_head(dt):
    """nwin 2, S 65, one head of 32: ld = pad64(96) = 128 and ldo = pad64(32) = 64, what hat_backward passes.  Same metric and bars as
    tests/test_gpu_backward_long.py (max-abs error over the reference's largest entry), here against float64."""
    lib = _lib.lib()
    case = (2, 65, 1, 32, 32)
    nwin, S, heads, d, D = case
    rows, ld, ldo = nwin * S, 128, 64
    q, k, v, do, scale, bias, _ = R.attention_inputs(case, dt, "bias")
    exact = R.attention.exact(q, k, v, do, scale, bias)
    btab, spad = _bias_table(lib, bias, heads, S)
    qkv, dO = _pack_qkv(q, k, v, D, ld, dt), _pack_o(do, D, ldo, dt)
    dqkv = _nan((rows + 2, ld), dt)
    dbias = torch.zeros(heads, S, S, device="cuda")
    nbytes = lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, D, 0)
    ws = torch.empty(nbytes // 4, dtype=F32, device="cuda")
    _lib.check(lib.fvit_bwd_window_attention_long(CODE[dt], qkv.data_ptr(), ld, dO.data_ptr(), ldo, btab.data_ptr(), spad, None, 0, 0, ctypes.c_float(scale),
                                                  dqkv.data_ptr(), dbias.data_ptr(), ws.data_ptr(), nbytes, nwin, S, heads, D, _stream()), "attention_bwd (long)")
    torch.cuda.synchronize()
    _untouched(dqkv, rows, 3 * heads * D, "long attention backward")
    errs = {n: (g.double() - exact[n]).abs().max().item() / exact[n].abs().max().item() for n, g in zip(("dq", "dk", "dv"), _unpack(dqkv, nwin, S, heads, D, d, 3))}
    rb = exact["ds"].sum(0)
    errs["dbias"] = (dbias.cpu().double() - rb).abs().max().item() / rb.abs().max().item()
    print(f"long attention backward {case} {dt} ld={ld} ldo={ldo}: " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    for n, e in errs.items():
        bar = LONG_BIAS_BAR[dt] if n == "dbias" else LONG_BAR[dt]
        assert e < bar, f"{n}: {e:.3e} of the reference's largest entry (bar {bar:.1e})"


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the GEMM forms only the backward uses
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _zero_padded(t, rows, cols, dt):
    out = torch.zeros(rows, cols, dtype=dt, device="cuda")
    out[:t.shape[0], :t.shape[1]] = t.to(dt).cuda()
    return out


GEMM_SHAPES = [(48, 80, 64), (272, 1024, 192), (1024, 272, 64)]


@DTS
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bias_act_without_a_bias(M, N, K, dt):
    lib = _lib.lib()
    g = R.gen(M + N + K)
    A = R.rounded(torch.randn(M, K, generator=g), dt)
    W = R.rounded(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    Ap, Wp = _zero_padded(A, _rup(M, 128), K, dt), _zero_padded(W, _rup(N, 128), K, dt)
    ldo = _rup(N, 64)
    out = _nan((_rup(M, 128), ldo), dt)
    _lib.check(lib.fvit_gemm_bias_act(CODE[dt], Ap.data_ptr(), K, Wp.data_ptr(), K, None, out.data_ptr(), ldo, M, N, K, 0, _stream()), "gemm without a bias")
    torch.cuda.synchronize()
    ref = A.double() @ W.double().t()
    got = out[:M, :N].double().cpu()
    tol = (4e-3 if dt == torch.float16 else 2e-2) * max(ref.abs().max().item(), 1.0)      # test_gemm_bias_act's
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"gemm_bias_act bias=NULL M={M} N={N} K={K} {dt}: max |err| {err:.3e}, bar {tol:.3e}")
    assert err < tol
    _untouched(out, M, N, "gemm_bias_act")


@DTS
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_residual_accumulates_without_bias_and_gamma(M, N, K, dt):
    lib = _lib.lib()
    g = R.gen(M * 3 + N + K)
    A = R.rounded(torch.randn(M, K, generator=g), dt)
    W = R.rounded(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    x0 = torch.randn(M, N, generator=g)
    Ap, Wp = _zero_padded(A, _rup(M, 128), K, dt), _zero_padded(W, _rup(N, 128), K, dt)
    x = _embed(x0, N, F32, rows=M + 3)
    _lib.check(lib.fvit_gemm_residual(CODE[dt], Ap.data_ptr(), K, Wp.data_ptr(), K, None, None, x.data_ptr(), N, M, N, K, _stream()), "accumulating gemm")
    torch.cuda.synchronize()
    ref = x0.double() + A.double() @ W.double().t()
    tol = 2e-4 * max(ref.abs().max().item(), 1.0) * (K / 256) ** 0.5                       # test_gemm_residual's
    err = (x[:M].double().cpu() - ref).abs().max().item()
    print(f"gemm_residual bias=gamma=NULL M={M} N={N} K={K} {dt}: max |err| {err:.3e}, bar {tol:.3e}")
    assert err < tol
    _untouched(x, M, N, "gemm_residual")


@DTS
@pytest.mark.parametrize("M", [1, 63, 65])
def test_weight_gradient_chain_from_nan_prefilled_transposes(M, dt):
    """gw += dout^T act exactly as hat_backward._linear_backward issues it, except that the two transposed operands start as NaN instead of zero: the
    GEMM contracts over all pad64(M) columns, so this fails unless fvit_bwd_transpose16 zero-fills columns M .. pad64(M) - 1 itself."""
    lib = _lib.lib()
    n, ka, ldo, lda, Mk = 200, 80, 256, 128, _rup(M, 64)
    g = R.gen(M * 17 + 5)
    dout = R.rounded(torch.randn(M, n, generator=g), dt)
    act = R.rounded(torch.randn(M, ka, generator=g), dt)
    gw0 = torch.randn(n, ka, generator=g)
    doutb, actb = _embed(dout, ldo, dt), _embed(act, lda, dt)
    doutT, actT = _nan((_rup(n, 128), Mk), dt), _nan((_rup(ka, 128), Mk), dt)
    gw = _embed(gw0, ka, F32, rows=n + 3)
    _lib.check(lib.fvit_bwd_transpose16(CODE[dt], doutb.data_ptr(), ldo, doutT.data_ptr(), Mk, M, n, _stream()), "dout^T")
    _lib.check(lib.fvit_bwd_transpose16(CODE[dt], actb.data_ptr(), lda, actT.data_ptr(), Mk, M, ka, _stream()), "act^T")
    _lib.check(lib.fvit_gemm_residual(CODE[dt], doutT.data_ptr(), Mk, actT.data_ptr(), Mk, None, None, gw.data_ptr(), ka, n, ka, Mk, _stream()), "gw")
    torch.cuda.synchronize()
    ref = gw0.double() + dout.double().t() @ act.double()
    got = gw[:n].double().cpu()
    assert torch.isfinite(got).all(), "the transposes left NaN in columns the GEMM contracts over"
    tol = 2e-4 * max(ref.abs().max().item(), 1.0) * (Mk / 256) ** 0.5                      # test_gemm_residual's
    err = (got - ref).abs().max().item()
    print(f"weight gradient chain M={M} {dt}: max |err| {err:.3e}, bar {tol:.3e}")
    assert err < tol
    _untouched(gw, n, ka, "gw")
