"""The CPU side of tests/test_gpu_attention_exact.py (no GPU): the conditions under which the selector cases of tests/attention_refs.py return a V row
bit for bit, the F study behind the rounding-level bar of the random cases, and the mutants both kinds of case catch:

    bias_stride_S     the bias table read at stride S instead of Spad                      selector off equality (S != Spad)
    head_table        one head's table used for another                                    selector off equality
    mask_zero         the softmax normalised over the Spad keys with 0 in place of FVIT_MASK_BIAS    selector off equality (S != Spad)
    vt_slot           two V^T slots swapped inside one 32-key block                        selector off equality
    no_rescale        the long kernel's accumulator not rescaled when the maximum moves    long selector off equality
    p_trunc           P truncated instead of rounded                                       a random case past the bar: NOT the max / rms bar (0.6 .. 0.75
                      of it: one extra half-ulp of P hides inside the output's own rounding) but the signed-bias bar, attention_refs.bias_ratio"""
import math

import pytest
import torch

from tests import attention_refs as R

DTS = R.OPERAND_DTYPES


def _exact_rows(c, inp, v):
    """fp64 attention of a dense selector case over the padded keys."""
    return R.attention(inp["q"], inp["k"], v, inp["bias"][:, :c.S, :], inp["scale"])


@pytest.mark.parametrize("family", ["table", "qk"])
@pytest.mark.parametrize("c", R.DENSE_CASES + [R.NOT_DENSE], ids=R.dense_id)
def test_dense_selector_conditions(c, family):
    for dt in DTS:
        inp = R.dense_selector(c, dt, family)
        assert R.selector_gap(inp["q"], inp["k"], inp["bias"], inp["scale"], c.S) >= R.GAP
        assert all(sorted(p.tolist()) == list(range(c.S)) for p in inp["perm"])
        if c.S > 2:
            assert not torch.equal(inp["perm"][0], inp["perm"][1])
        for t in (inp["q"], inp["k"], inp["v"], inp["v_hi"], inp["v_lo"]):
            assert torch.equal(t.to(dt).float(), t)                                   # operands are values of T
        if family == "qk":
            cd = R.codes(c.S, c.d)
            assert len({tuple(r) for r in cd.tolist()}) == c.S and set(cd.unique().tolist()) <= {-1.0, 1.0}
            assert (inp["q"].abs() == 64).all()
        want = R.gathered(inp["v"], inp["perm"])
        assert (_exact_rows(c, inp, inp["v"]) - want.double()).abs().max().item() < 1e-40
        assert torch.equal(R.attention(inp["q"], inp["k"], inp["v"], inp["bias"][:, :c.S, :], inp["scale"], dt), want)
        # the two-term split: hi + lo exact in fp32, and it splits back into the same two terms
        s32 = inp["v_hi"] + inp["v_lo"]
        assert torch.equal(s32.double(), inp["v_hi"].double() + inp["v_lo"].double())
        assert torch.equal(s32.to(dt).float(), inp["v_hi"]) and torch.equal((s32 - inp["v_hi"]).to(dt).float(), inp["v_lo"])
        assert (inp["v_lo"] != 0).any()


@pytest.mark.parametrize("c", R.LONG_CASES, ids=R.long_id)
def test_long_selector_conditions(c):
    assert c.ng + c.w * c.w == c.S
    seen = [False, False]
    for pair in (0, 1):
        inp = R.long_selector(c, 32, torch.float16, pair)
        b, one = inp["bias"], inp["onehot"]
        top = b.topk(min(2, c.S), -1).values
        if c.S > 1:
            assert ((top[..., 0] - top[..., 1])[one] >= R.GAP).all()
            assert (top[..., 0] == top[..., 1])[~one].all()                            # the other rows: several keys at exactly the same score
        exact = R.attention(torch.zeros_like(inp["v"]), torch.zeros_like(inp["v"]), inp["v"], b, inp["scale"])
        sel = b.argmax(-1)                                                             # [heads][S]
        want = R.gathered(inp["v"], sel)
        m = one[None, :, :, None].expand_as(want)
        assert (exact - want.double())[m].abs().max().item() < 1e-40 if m.any() else True
        # the selected keys reach the first and the last 32-key tile, in the first and the last query tile
        for h in range(b.shape[0]):
            q = one[h].nonzero().flatten()
            if q.numel():
                seen[0] |= bool((sel[h][q] < 32).any())
                seen[1] |= bool((sel[h][q] >= (c.S - 1) // 32 * 32).any())
    if c.ng == 0:
        assert all(seen)


def _study(kernel, cases, make, S_of):
    worst, e16s = {}, []
    for case in cases:
        for dt in DTS:
            for seed in R.STUDY_SEEDS:
                inp = make(case, dt, seed)
                S = S_of(case)
                args = (inp["q"], inp["k"], inp["v"], inp["bias"][:, :S, :], inp["scale"])
                exact, plain = R.attention(*args), R.attention(*args, dt)
                e16s.append((plain.double() - exact).abs().max().item())
                for name, opt in R.VARIANTS[kernel].items():
                    var = R.attention(*args, dt, **opt)
                    w = worst.setdefault(name, [0.0, 0.0])
                    rm, rr = R.variant_ratios(exact, plain, var)
                    w[0], w[1] = max(w[0], rm), max(w[1], rr)
                    gm, gr = R.ratios(kernel, var, exact, plain, dt)     # a variant, stored to T, passes the bar
                    assert gm <= 1.0 and gr <= 1.0, (kernel, case, dt, seed, name, gm, gr)
    return worst, e16s


@pytest.mark.parametrize("kernel", ["dense", "long"])
def test_f_study(kernel, capsys):
    if kernel == "dense":
        worst, e16s = _study(kernel, R.RANDOM_DENSE, R.random_dense, lambda c: c.S)
    else:
        worst, e16s = _study(kernel, R.RANDOM_LONG, R.random_long, lambda c: c[0].S)
    wm, wr = max(w[0] for w in worst.values()), max(w[1] for w in worst.values())
    need = [math.ceil(2 * x * 1.02 * 10 - 1e-9) / 10 for x in (wm, wr)]
    with capsys.disabled():
        print(f"\nattention F study, {kernel}: e16 {min(e16s):.2e} .. {max(e16s):.2e}; " +
              "; ".join(f"{k} max {v[0]:.3f} rms {v[1]:.3f}" for k, v in worst.items()) +
              f" -> needs F_max {need[0]} F_rms {need[1]}; module has {R.F_MAX[kernel]} / {R.F_RMS[kernel]}")
    # F is the documented rounding-up of the study; the 2 % is the room for another CPU's matmul
    assert 2 * wm <= R.F_MAX[kernel] <= 4.0 and 2 * wr <= R.F_RMS[kernel] <= 4.0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ------------------------------------------------------------------------------------------------------------------------------------------------
RAGGED = [c for c in R.DENSE_CASES if c.S != R.spad(c.S) and c.S > 1]


@pytest.mark.parametrize("c", R.DENSE_CASES, ids=R.dense_id)
def test_selector_mutants(c):
    dt = torch.float16
    for family in ("table", "qk"):
        inp = R.dense_selector(c, dt, family)
        S, sp, perm = c.S, inp["sp"], inp["perm"]
        want = R.gathered(inp["v"], perm).double()

        def off(bias=None, v=None):
            b = inp["bias"] if bias is None else bias
            got = R.attention(inp["q"], inp["k"], inp["v"] if v is None else v, b[:, :S, :], inp["scale"])
            return not torch.equal(got.float().to(dt).double(), want.float().to(dt).double())

        assert not off()
        if S > 1:
            vs = inp["v"].clone()
            vs[..., [0, 1], :] = vs[..., [1, 0], :]
            assert off(v=vs), "vt_slot"
        if family == "table" and S > 2:
            assert off(bias=inp["bias"].roll(1, 0)), "head_table"
        if S != sp and family == "table":
            bz = inp["bias"].clone()
            bz[:, :, S:] = 0.0
            assert off(bias=bz), "mask_zero"
            if S > 1:
                flat = inp["bias"].reshape(inp["bias"].shape[0], -1)
                idx = torch.arange(S)[:, None] * S + torch.arange(sp)[None, :]
                bs = inp["bias"].clone()
                bs[:, :S, :] = flat[:, idx]
                assert off(bias=bs), "bias_stride_S"


@pytest.mark.parametrize("c", [c for c in R.LONG_CASES if c.S > 32 and c.ng == 0], ids=R.long_id)
def test_long_selector_catches_a_missing_rescale(c):
    dt = torch.float16
    hit = False
    for pair in (0, 1):
        inp = R.long_selector(c, 32, dt, pair)
        z = torch.zeros_like(inp["v"])
        args = (z, z, inp["v"], inp["bias"], inp["scale"])
        m = inp["onehot"][None, :, :, None].expand_as(inp["v"])
        want = R.gathered(inp["v"], inp["bias"].argmax(-1))
        good = R.attention(*args, dt, online=32)
        assert torch.equal(good[m], want[m])
        bad = R.attention(*args, dt, online=32, mut="no_rescale")
        hit |= not torch.equal(bad[m], want[m])
    assert hit


@pytest.mark.parametrize("dt", DTS, ids=str)
def test_truncated_p_fails_a_random_case(dt):
    over = []
    for c in R.RANDOM_DENSE:
        inp = R.random_dense(c, dt)
        args = (inp["q"], inp["k"], inp["v"], inp["bias"][:, :c.S, :], inp["scale"])
        exact, plain = R.attention(*args), R.attention(*args, dt)
        bad = R.attention(*args, dt, mut="p_trunc")
        over.append(R.ratios("dense", bad, exact, plain, dt) + (R.bias_ratio(bad, exact, plain),))
    for case in R.RANDOM_LONG:
        inp = R.random_long(case, dt)
        args = (inp["q"], inp["k"], inp["v"], inp["bias"], inp["scale"])
        exact, plain = R.attention(*args), R.attention(*args, dt)
        bad = R.attention(*args, dt, online=32, mut="p_trunc")
        over.append(R.ratios("long", bad, exact, plain, dt) + (R.bias_ratio(bad, exact, plain),))
        assert R.bias_ratio(R.attention(*args, dt, online=32), exact, plain) <= 0.5          # the online form itself is unbiased
    print(dt, [tuple(round(x, 3) for x in o) for o in over])
    assert all(max(o) > 1.0 for o in over), over


@pytest.mark.parametrize("dt", DTS, ids=str)
@pytest.mark.parametrize("c", [c for c in R.LONG_CASES if c.S > 1], ids=R.long_id)
def test_equal_rows_lo_interval_holds_the_split_and_has_teeth(c, dt):
    """The two-term split of the float32 mean lies inside equal_rows_lo_interval on every row; a lo image that is zero, or that belongs to the
    neighbouring query, falls outside somewhere on the rows with several equal scores."""
    for pair in (0, 1):
        inp = R.long_selector(c, 32, dt, pair)
        v = inp["v_hi"] + inp["v_lo"]
        z = torch.zeros_like(v)
        y32 = R.attention(z, z, v, inp["bias"], inp["scale"], torch.float32)
        y32 = R.attention(z, z, v, inp["bias"], inp["scale"], torch.float32, online=32) if pair else y32
        hi = y32.to(dt).float()
        lo = (y32 - hi).to(dt).float()
        lo_min, lo_max, exact = R.equal_rows_lo_interval(v, inp["bias"], hi, dt)
        assert ((lo >= lo_min) & (lo <= lo_max)).all()
        many = ~inp["onehot"][None, :, :, None].expand_as(v)
        if many.any():
            for bad in (torch.zeros_like(lo), lo.roll(1, 2)):
                assert (((bad < lo_min) | (bad > lo_max)) & many).any()
