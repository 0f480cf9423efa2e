"""The fused HAT block kernels through the C ABI (needs an MI355X), held to the reference's own rounding error: what is compared is the BRANCH
(got - xin), not xin + branch whose size the residual stream sets, against the float64 chain of tests/fused_block_refs.py, with the bar that module
derives from a plain 16-bit evaluation of the same chain (F x its error; tests/test_fused_block_refs_cpu.py proves that bar fair and that one leaked
key, one shifted bias row, one dropped bias tile ... are 2 x .. 100 x over it).

Inputs, every case: rows 1.3 randn + 0.2 with one row of mean 300; LayerNorm weights U(0.5, 1.5); biases 0.3 randn; the attention bias table
2 randn - 8 on real keys, FVIT_MASK_BIAS on key columns >= S and 0 on query rows >= S as hat_runtime builds it (so a leaked padded key outweighs every
real one); 3 spare rows of finite 1e3 randn behind every input row buffer and in every srcA / srcB / add row no index names; every output buffer NaN
with 3 spare rows that must stay NaN (in place: the spare garbage rows must come back bit for bit).  Every route the *_supported calls admit runs on
the same inputs; each prints its two ratios (max bar, rms bar; both must be <= 1)."""
import pytest
import torch

from fastervit_amd import _lib, hat_runtime
from tests import fused_block_refs as R
from tests.util import tuned

pytestmark = pytest.mark.gpu

CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}
DT_IDS = ["f16", "bf16"]
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t, dtype=None):
    if t is None:
        return None
    return (t if dtype is None else t.to(dtype)).contiguous().cuda()


def _bias_table(bias, S, spad):
    """[heads][spad][spad] as hat_runtime builds it: the mask on padded key columns, 0 on padded query rows."""
    heads = bias.shape[0]
    t = torch.zeros(heads, spad, spad)
    t[:, :S, :S] = bias
    t[:, :, S:] = _lib.FVIT_MASK_BIAS
    t[:, S:, :S] = 0.0
    return t.cuda()


def _attn_weights(inp):
    dt, heads = inp["dt"], inp["heads"]
    return dict(wqf=hat_runtime.frag_pack_qkv(inp["wqkv"], heads).to(dt).contiguous().cuda(),
                bqh=inp["bqkv"].view(3, heads, 32).permute(1, 0, 2).reshape(heads, 96).contiguous().cuda(),
                wpf=hat_runtime.frag_pack_fc2(inp["wproj"]).to(dt).contiguous().cuda(),
                ln_w=_dev(inp["ln_w"]), ln_b=_dev(inp["ln_b"]), bproj=_dev(inp["bproj"]), gamma=_dev(inp.get("gamma")))


def _mlp_weights(inp):
    dt = inp["dt"]
    return dict(w1f=hat_runtime.frag_pack_fc1(inp["w1"]).to(dt).contiguous().cuda(), w2f=hat_runtime.frag_pack_fc2(inp["w2"]).to(dt).contiguous().cuda(),
                b1=_dev(inp["b1"]), b2=_dev(inp["b2"]))


class _Ref:
    """exact and plain16 of one case, computed once for all of its routes."""

    def __init__(self, cid, chain, inp):
        self.cid, self.chain, self.dt = cid, chain, inp["dt"]
        self.exact, self.xin = R.CHAIN[chain].exact(inp)
        self.plain, _ = R.CHAIN[chain].plain16(inp)

    def check(self, route, got):
        """``got``: the kernel's output rows (fp32 chains: xin + branch; ln_gemm: the 16-bit result)."""
        got = got.detach().cpu().to(torch.float64)
        assert torch.isfinite(got).all(), f"{self.cid} {route}: non-finite output"
        if self.chain != "ln_gemm":
            got = got - self.xin
        rmax, rrms = R.ratios(self.chain, got, self.exact, self.plain, self.xin, self.dt)
        print(f"{self.cid} {route}: {rmax:.3f} x max bar, {rrms:.3f} x rms bar")
        assert rmax <= 1.0, f"{self.cid} {route}: {rmax:.3f} x the max bar"
        assert rrms <= 1.0, f"{self.cid} {route}: {rrms:.3f} x the rms bar"


def _out(rows, C, dtype=torch.float32):
    return torch.full((rows + R.SPARE, C), NAN, dtype=dtype, device="cuda")


def _spare_untouched(out, rows):
    return bool(torch.isnan(out[rows:].float()).all())


# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_attn_block_branch(case, dt):
    lib = _lib.lib()
    C, S, nwin, tables = case
    heads, rows = C // 32, nwin * S
    inp = R.attn_inputs(case, dt)
    ref = _Ref(f"attn_block C={C} S={S} nwin={nwin} tables={int(tables)} {DT_IDS[CODE[dt] - 1]}", "attn_block", inp)
    spad = lib.fvit_attention_spad(S)
    assert spad == R.spad(S)
    w = _attn_weights(inp)
    srcA, srcB, add = _dev(inp["srcA"]), _dev(inp.get("srcB")), _dev(inp.get("add"))
    si, ai = _dev(inp.get("src_idx"), torch.int32), _dev(inp.get("add_idx"), torch.int32)
    bp = _bias_table(inp["bias"], S, spad)
    args = (CODE[dt], _ptr(srcA), inp["rowsA"], _ptr(srcB), inp["rowsB"], _ptr(si), _ptr(ai), _ptr(add), _ptr(w["ln_w"]), _ptr(w["ln_b"]), inp["eps"],
            inp["rows_per_image"], _ptr(w["wqf"]), _ptr(w["bqh"]), _ptr(w["wpf"]), _ptr(w["bproj"]), _ptr(w["gamma"]), _ptr(bp))
    tail = (nwin, S, heads, C, inp["scale"])

    def run(route, fn, *extra):
        out = _out(rows, C)
        _lib.check(fn(*args, out.data_ptr(), *tail, *extra, _stream()), route)
        torch.cuda.synchronize()
        assert _spare_untouched(out, rows), f"{route}: rows behind the output written"
        ref.check(route, out[:rows])
        return out[:rows]

    routes = 0
    if lib.fvit_attn_block_supported(C, heads, S):
        with tuned(ab_variant=0):
            run("attn_block_fused", lib.fvit_attn_block_fused)
        routes += 1
        if C == 256 and S > 48:        # the wave-per-(window, head) form, one and two windows per workgroup (odd nwin: the two-window form has a tail)
            for nw in (1, 2):
                with tuned(ab_variant=3, ab2_nwin=nw):
                    run(f"attn_block_fused ab_variant=3 ab2_nwin={nw}", lib.fvit_attn_block_fused)
                routes += 1
    if lib.fvit_win_block_supported(C, heads, S):
        run("win_block_fused", lib.fvit_win_block_fused)
        routes += 1
        if C == 512:                   # the heads split over two sibling workgroups that meet in L2
            slab = torch.full((nwin * 2 * 64 * C,), NAN, device="cuda")
            cnt = torch.zeros(nwin, dtype=torch.int32, device="cuda")
            run("win_block_fused_split nsplit=2", lib.fvit_win_block_fused_split, slab.data_ptr(), cnt.data_ptr(), 2)
            assert int(cnt.abs().sum().item()) == 0, "split counters not back at 0"
            routes += 1
    assert routes >= 1
    assert lib.fvit_win_block_supported(C, heads, S) == (1 if S > 48 else 0) and lib.fvit_attn_block_supported(C, heads, S) == 1


# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.CT_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_ct_block_branch(case, dt):
    lib = _lib.lib()
    batch, G, use_add, use_gamma = case
    C, heads, hid, rows = R.CT_C, R.CT_HEADS, R.CT_HIDDEN, batch * G
    assert lib.fvit_ct_block_supported(C, heads, G, hid) == 1
    inp = R.ct_inputs(case, dt)
    ref = _Ref(f"ct_block batch={batch} G={G} add={int(use_add)} gamma={int(use_gamma)} {DT_IDS[CODE[dt] - 1]}", "ct_block", inp)
    w, m = _attn_weights(inp), _mlp_weights(inp)
    X, add, si = _dev(inp["srcA"]), _dev(inp.get("add")), _dev(inp["src_idx"], torch.int32)
    ln2w, ln2b, g2 = _dev(inp["ln2_ln_w"]), _dev(inp["ln2_ln_b"]), _dev(inp.get("ln2_gamma"))
    bp = _bias_table(inp["bias"], G, 16)
    for variant in (0, 1, 2, 3):
        out = _out(rows, C)
        with tuned(ct_variant=variant):
            rc = lib.fvit_ct_block_fused(CODE[dt], X.data_ptr(), inp["rowsA"], si.data_ptr(), _ptr(add), out.data_ptr(), batch, G, heads, C, hid,
                                         _ptr(w["ln_w"]), _ptr(w["ln_b"]), _ptr(w["wqf"]), _ptr(w["bqh"]), _ptr(w["wpf"]), _ptr(w["bproj"]), _ptr(w["gamma"]),
                                         bp.data_ptr(), inp["scale"], ln2w.data_ptr(), ln2b.data_ptr(), _ptr(m["w1f"]), _ptr(m["b1"]), _ptr(m["w2f"]),
                                         _ptr(m["b2"]), _ptr(g2), inp["eps"], _stream())
        _lib.check(rc, "ct_block_fused")
        torch.cuda.synchronize()
        assert _spare_untouched(out, rows), f"ct_variant {variant}: rows behind the output written"
        ref.check(f"ct_block_fused ct_variant={variant}", out[:rows])


# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "nogamma"])
@pytest.mark.parametrize("C", R.MLP_C)
@pytest.mark.parametrize("M", R.MLP_M)
def test_mlp_branch(M, C, use_gamma, dt):
    lib = _lib.lib()
    hid = 4 * C
    inp = R.mlp_inputs(M, C, use_gamma, dt)
    ref = _Ref(f"mlp M={M} C={C} gamma={int(use_gamma)} {DT_IDS[CODE[dt] - 1]}", "mlp", inp)
    m = _mlp_weights(inp)
    x0, ln_w, ln_b, gamma = _dev(inp["srcA"]), _dev(inp["ln_w"]), _dev(inp["ln_b"]), _dev(inp.get("gamma"))

    def run(route, fn, *extra):
        x = x0.clone()
        _lib.check(fn(CODE[dt], x.data_ptr(), M, C, hid, ln_w.data_ptr(), ln_b.data_ptr(), inp["eps"], _ptr(m["w1f"]), _ptr(m["b1"]), _ptr(m["w2f"]),
                      _ptr(m["b2"]), _ptr(gamma), *extra, _stream()), route)
        torch.cuda.synchronize()
        assert torch.equal(x[M:], x0[M:]), f"{route}: rows behind the M rows written"
        ref.check(route, x[:M])
        return x[:M]

    routes = 0
    if lib.fvit_mlp_fused_supported(C, hid):
        run("mlp_fused", lib.fvit_mlp_fused)
        routes += 1
    if lib.fvit_win_mlp_supported(C, hid):
        outs = []
        for pipe in (0, 1):
            with tuned(win_mlp_pipe=pipe):
                outs.append(run(f"win_mlp_fused win_mlp_pipe={pipe}", lib.fvit_win_mlp_fused))
        assert torch.equal(outs[0], outs[1])          # the pipelined loop runs the same operations per value in the same order
        routes += 2
        if C == 512:
            slab = torch.full((lib.fvit_win_mlp_split_bytes(M, C, 2) // 4,), NAN, device="cuda")
            cnt = torch.zeros((M + 63) // 64, dtype=torch.int32, device="cuda")
            run("win_mlp_fused_split nsplit=2", lib.fvit_win_mlp_fused_split, 1, slab.data_ptr(), cnt.data_ptr(), 2)
            assert int(cnt.abs().sum().item()) == 0, "split counters not back at 0"
            routes += 1
    assert routes == (4 if C == 512 else 3)


# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.LN_GEMM_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_ln_gemm_branch(case, dt):
    lib = _lib.lib()
    M, C, N, act, gather = case
    inp = R.ln_gemm_inputs(case, dt)
    ref = _Ref(f"ln_gemm M={M} C={C} N={N} act={act} gather={int(gather)} {DT_IDS[CODE[dt] - 1]}", "ln_gemm", inp)
    ldo = (N + 63) // 64 * 64
    assert lib.fvit_ln_gemm_supported(C, N, C, ldo) == 1
    Wp = torch.zeros((N + 127) // 128 * 128, C, dtype=dt)
    Wp[:N] = inp["W"].to(dt)
    Wp = Wp.cuda()
    srcA, srcB, add = _dev(inp["srcA"]), _dev(inp.get("srcB")), _dev(inp.get("add"))
    si, ai = _dev(inp.get("src_idx"), torch.int32), _dev(inp.get("add_idx"), torch.int32)
    ln_w, ln_b, bias = _dev(inp["ln_w"]), _dev(inp["ln_b"]), _dev(inp["bias"])
    out = _out(M, ldo, dt)
    x_out = _out(M, C) if gather else None
    rc = lib.fvit_ln_gemm(CODE[dt], srcA.data_ptr(), inp["rowsA"], _ptr(srcB), inp["rowsB"], _ptr(si), _ptr(ai), _ptr(add), _ptr(x_out), ln_w.data_ptr(),
                          ln_b.data_ptr(), inp["eps"], M, inp["rows_per_image"], C, Wp.data_ptr(), C, bias.data_ptr(), out.data_ptr(), ldo, N, act, _stream())
    _lib.check(rc, "ln_gemm")
    torch.cuda.synchronize()
    assert _spare_untouched(out, M) and bool(torch.isnan(out[:M, N:].float()).all()), "ln_gemm: wrote behind its M x N result"
    ref.check("ln_gemm", out[:M, :N])
    if gather:     # the fp32 copy of the gathered rows: one fp32 add of two fp32 values, the same on any machine
        assert _spare_untouched(x_out, M)
        assert torch.equal(x_out[:M].cpu(), R.ln_gemm.plain16(inp)[1])
