"""The unit window-attention kernels through the C ABI on the cases of tests/attention_refs.py: every instance of the dense kernel
(csrc/fvit_attn.hip: SB 1..8, 10, 13 x DP 32 / 64 / 96, the 9 -> 10 and 11, 12 -> 13 remaps, the two-term instances with a tail in both
items-per-workgroup counts, the attn_drop mask; dpad 96 beyond 128 tokens must be refused by every dense entry) and the online-softmax kernel
(csrc/fvit_attnlong.hip) on selector cases whose output must EQUAL a gathered V row, and both kernels on random cases at the rounding level.

qkv rows carry 8 extra elements (NaN) and the output 8 extra columns; the output is NaN wherever the kernel must not write and the pad channels
d .. dpad-1 must come back exactly 0.  The instance that served a call is confirmed by its launch name in _lib.prof_records(), which carries SB (after
launch_attention's remaps) and DP: "attn_kernel sb10 dp64", "attn_kernel<two-term> sb4 dp32", "attn_long_kernel dp96".  tests/test_attention_refs_cpu.py holds the CPU side."""
import contextlib
import ctypes

import pytest
import torch

from fastervit_amd import _lib
from tests import attention_refs as R

pytestmark = pytest.mark.gpu
CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}
SPARE = 3
NAN = float("nan")


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


def _pack(dt, dpad, terms):
    """qkv [rows + SPARE][ldq] of NaN with the [q | k | v][head][dpad] section(s) zero-filled and the images written in; terms: list of (q, k, v), one
    per image.  Returns (buffer, ldq, q_lo_off)."""
    nwin, heads, S, d = terms[0][0].shape
    hd3, rows = 3 * heads * dpad, nwin * S
    lo_off = hd3 + 8 if len(terms) == 2 else 0
    ldq = (lo_off + hd3 if lo_off else hd3) + 8
    buf = torch.full((rows + SPARE, ldq), NAN, dtype=dt)
    for i, qkv in enumerate(terms):
        sec = torch.zeros(nwin, S, 3, heads, dpad, dtype=dt)
        for si, t in enumerate(qkv):
            sec[:, :, si, :, :d] = t.permute(0, 2, 1, 3).to(dt)
        buf[:rows, i * lo_off:i * lo_off + hd3] = sec.view(rows, hd3)
    return buf, ldq, lo_off


def _call(entry, dt, dpad, terms, scale, *, bias=None, mask=None, tab=None, w=0, ng=0, want_name):
    """Run one entry point on poisoned buffers; returns the output image(s) as [nwin][heads][S][dpad] float32 on the CPU."""
    lib = _lib.lib()
    nwin, heads, S, d = terms[0][0].shape
    rows, hd = nwin * S, heads * dpad
    qkv, ldq, q_lo = _pack(dt, dpad, terms)
    two = len(terms) == 2
    o_lo = hd + 8 if two else 0
    ldo = (o_lo + hd if two else hd) + 8
    out = torch.full((rows + SPARE, ldo), NAN, dtype=dt, device="cuda")
    qkv = qkv.cuda()
    dev = [t.cuda() if t is not None else None for t in (bias, mask, tab)]
    sc, names = ctypes.c_float(scale), []
    with _launch_names(names):
        if entry == "dense":
            rc = lib.fvit_window_attention(CODE[dt], qkv.data_ptr(), ldq, out.data_ptr(), ldo, dev[0].data_ptr(), nwin, S, heads, dpad, sc, _stream())
        elif entry == "drop":
            rc = lib.fvit_window_attention_drop(CODE[dt], qkv.data_ptr(), ldq, out.data_ptr(), ldo, dev[0].data_ptr(), nwin, S, heads, dpad, sc,
                                                _lib.ptr(dev[1]), _stream())
        elif entry == "terms":
            rc = lib.fvit_window_attention_terms(CODE[dt], qkv.data_ptr(), ldq, q_lo, out.data_ptr(), ldo, o_lo, dev[0].data_ptr(), nwin, S, heads, dpad,
                                                 sc, _stream())
        elif entry == "long":
            rc = lib.fvit_window_attention_long(CODE[dt], qkv.data_ptr(), ldq, out.data_ptr(), ldo, _lib.ptr(dev[2]), w, ng, nwin, S, heads, dpad, sc,
                                                _stream())
        else:
            rc = lib.fvit_window_attention_long_terms(CODE[dt], qkv.data_ptr(), ldq, q_lo, out.data_ptr(), ldo, o_lo, _lib.ptr(dev[2]), w, ng, nwin, S,
                                                      heads, dpad, sc, _stream())
        _lib.check(rc, entry)
        torch.cuda.synchronize()
    want_name = f"{want_name} sb{R.spad(S) // 16} dp{dpad}" if want_name.startswith("attn_kernel") else f"{want_name} dp{dpad}"
    assert names == [want_name], (names, want_name)
    out = out.cpu()
    assert _isnan(out[rows:]) and _isnan(out[:rows, (o_lo + hd if two else hd):])
    if two:
        assert _isnan(out[:rows, hd:o_lo])
    imgs = [out[:rows, i * o_lo:i * o_lo + hd].float().view(nwin, S, heads, dpad).permute(0, 2, 1, 3) for i in range(len(terms))]
    for img in imgs:
        assert torch.equal(img[..., d:], torch.zeros_like(img[..., d:])), "pad channels"
    return [img[..., :d] for img in imgs]


def _eq(got, want, what):
    assert torch.equal(got, want), (what, int((got != want).sum()), (got - want).abs().max().item())


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.DENSE_CASES, ids=R.dense_id)
def test_dense_selector(c, dt):
    assert _lib.lib().fvit_attention_spad(c.S) == R.spad(c.S) and _lib.lib().fvit_attention_dense(c.S, c.dpad) == 1
    for family in ("table", "qk"):
        inp = R.dense_selector(c, dt, family)
        q, k, perm, z = inp["q"], inp["k"], inp["perm"], torch.zeros_like(inp["q"])
        kw = dict(bias=inp["bias"])
        (got,) = _call("dense", dt, c.dpad, [(q, k, inp["v"])], inp["scale"], want_name="attn_kernel", **kw)
        _eq(got, R.gathered(inp["v"], perm), (family, "dense"))
        hi, lo = _call("terms", dt, c.dpad, [(q, k, inp["v_hi"]), (z, z, inp["v_lo"])], inp["scale"], want_name="attn_kernel<two-term>", **kw)
        _eq(hi, R.gathered(inp["v_hi"], perm), (family, "terms hi"))
        _eq(lo, R.gathered(inp["v_lo"], perm), (family, "terms lo"))
        # attn_drop: all ones = the no-mask bits; the selected key of every third row zeroed = exactly 0 there
        sp = inp["sp"]
        mask = torch.ones(R.NWIN * R.HEADS, c.S, sp, dtype=dt)
        (ones,) = _call("drop", dt, c.dpad, [(q, k, inp["v"])], inp["scale"], mask=mask, want_name="attn_kernel", **kw)
        _eq(ones, got, (family, "drop ones"))
        rows = torch.arange(0, c.S, 3)
        m4 = mask.view(R.NWIN, R.HEADS, c.S, sp)
        for h in range(R.HEADS):
            m4[:, h, rows, perm[h][rows]] = 0
        (dropped,) = _call("drop", dt, c.dpad, [(q, k, inp["v"])], inp["scale"], mask=mask, want_name="attn_kernel", **kw)
        want = got.clone()
        want[:, :, rows] = 0
        _eq(dropped, want, (family, "drop selected"))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
def test_dpad96_beyond_128_tokens_is_refused_by_every_dense_entry(dt):
    """That geometry belongs to the long kernel, which takes the compact table: a dense entry that handed it over would drop its `bias` argument without
    a word.  All three say so instead."""
    c = R.NOT_DENSE
    assert _lib.lib().fvit_attention_dense(c.S, c.dpad) == 0
    inp = R.dense_selector(c, dt, "qk")
    z = torch.zeros_like(inp["q"])
    for entry, terms in (("dense", [(inp["q"], inp["k"], inp["v"])]), ("drop", [(inp["q"], inp["k"], inp["v"])]),
                         ("terms", [(inp["q"], inp["k"], inp["v_hi"]), (z, z, inp["v_lo"])])):
        with pytest.raises(RuntimeError, match="outside the dense-bias kernel"):
            _call(entry, dt, c.dpad, terms, inp["scale"], bias=inp["bias"], want_name="none")


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("dpad,d", R.LONG_DP)
@pytest.mark.parametrize("c", R.LONG_CASES, ids=R.long_id)
def test_long_selector(c, dpad, d, dt):
    for pair in (0, 1):
        inp = R.long_selector(c, d, dt, pair)
        z = torch.zeros_like(inp["v"])
        one = inp["onehot"][None, :, :, None].expand_as(inp["v"])
        sel = inp["bias"].argmax(-1)
        kw = dict(tab=inp["tab"], w=c.w, ng=c.ng)
        (got,) = _call("long", dt, dpad, [(z, z, inp["v"])], inp["scale"], want_name="attn_long_kernel", **kw)
        _eq(got[one], R.gathered(inp["v"], sel)[one], (pair, "long"))
        hi, lo = _call("long_terms", dt, dpad, [(z, z, inp["v_hi"]), (z, z, inp["v_lo"])], inp["scale"], want_name="attn_long_kernel<two-term>", **kw)
        _eq(hi[one], R.gathered(inp["v_hi"], sel)[one], (pair, "terms hi"))
        _eq(lo[one], R.gathered(inp["v_lo"], sel)[one], (pair, "terms lo"))
        lo_min, lo_max, _ = R.equal_rows_lo_interval(inp["v_hi"] + inp["v_lo"], inp["bias"], hi, dt)       # every row; on the one-hot rows it is v_lo itself
        bad = (lo < lo_min) | (lo > lo_max) | ~torch.isfinite(lo)
        assert not bad.any(), (pair, "terms lo interval", int(bad.sum()), int((bad & ~one).sum()))
        if not one.all():        # rows with several keys at the same score: the fp64 mean of their V rows, at the rounding level
            for name, g, v in (("long", got, inp["v"]), ("terms hi", hi, inp["v_hi"] + inp["v_lo"])):
                exact, plain = R.attention(z, z, v, inp["bias"], inp["scale"]), R.attention(z, z, v, inp["bias"], inp["scale"], dt)
                rmax, rrms = R.ratios("long", g[~one], exact[~one], plain[~one], dt)
                print(f"long selector {R.long_id(c)} dp{dpad} {dt} pair {pair} {name}: equal-score rows max ratio {rmax:.3f} rms ratio {rrms:.3f}")
                assert rmax <= 1.0 and rrms <= 1.0, (name, rmax, rrms)


def _report(kind, cid, dt, got, exact, plain):
    rmax, rrms = R.ratios(kind, got, exact, plain, dt)
    rb = R.bias_ratio(got, exact, plain)
    print(f"attention random {kind} {cid} {dt}: max ratio {rmax:.3f} rms ratio {rrms:.3f} signed-bias ratio {rb:.3f}")
    assert rmax <= 1.0 and rrms <= 1.0 and rb <= 1.0, (rmax, rrms, rb)


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("c", R.RANDOM_DENSE, ids=R.dense_id)
def test_dense_random_case_at_the_rounding_level(c, dt):
    inp = R.random_dense(c, dt)
    (got,) = _call("dense", dt, c.dpad, [(inp["q"], inp["k"], inp["v"])], inp["scale"], bias=inp["bias"], want_name="attn_kernel")
    args = (inp["q"], inp["k"], inp["v"], inp["bias"][:, :c.S, :], inp["scale"])
    _report("dense", R.dense_id(c), dt, got, R.attention(*args), R.attention(*args, dt))


@pytest.mark.parametrize("dt", R.OPERAND_DTYPES, ids=str)
@pytest.mark.parametrize("case", R.RANDOM_LONG, ids=lambda v: f"{R.long_id(v[0])}-dp{v[1]}-d{v[2]}")
def test_long_random_case_at_the_rounding_level(case, dt):
    c, dpad, d = case
    inp = R.random_long(case, dt)
    (got,) = _call("long", dt, dpad, [(inp["q"], inp["k"], inp["v"])], inp["scale"], tab=inp["tab"], w=c.w, ng=c.ng, want_name="attn_long_kernel")
    args = (inp["q"], inp["k"], inp["v"], inp["bias"], inp["scale"])
    _report("long", R.long_id(c), dt, got, R.attention(*args), R.attention(*args, dt))
