"""The references of tests/fused_block_refs.py checked against themselves, without a GPU, on every case that tests/test_gpu_fused_blocks_branch.py
runs on the kernels:

  * fair reference: ``exact`` agrees with an independent float64 statement of the chain (rows gathered one by one, F.layer_norm,
    F.scaled_dot_product_attention, F.gelu, F.linear);
  * fair bar: every other legitimate way to do plain16's arithmetic (R.VARIANTS), on 4 seeds, lies within HALF the bar -- which is how F_max and F_rms
    are defined -- and F_max <= 4;
  * teeth: every mutant of plain16 (one masking, indexing, bias or gamma error each) is at least 2 x over the max bar wherever it applies.

tanh-GELU in place of the erf form is below this suite's resolution and is only measured (test_tanh_gelu_is_below_resolution prints it): over the mlp
and ct_block cases it moves the branch by 7e-4 .. 1.5e-3 where e16 is 5e-4 .. 2.2e-3 in fp16, and by 1.5e-3 .. 4.8e-3 where e16 is 5e-3 .. 2.5e-2 in
bf16: 0.30 .. 0.53 x the max bar, 0.39 .. 0.53 x the rms bar, next to 0.33 .. 0.49 for the unchanged plain16.  No case is bent to catch it."""
import pytest
import torch
import torch.nn.functional as F

from tests import fused_block_refs as R

F64 = torch.float64
EXACT_RTOL = 1e-11      # two float64 evaluations of the same chain, relative to the tensor's largest entry
CASES = R.all_cases()


def _inp(cid, make):
    return make(0)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the independent statement
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _gather_loop(inp):
    C, rpi = inp["C"], inp["rows_per_image"]
    si, ai, add = inp.get("src_idx"), inp.get("add_idx"), inp.get("add")
    rows = []
    for b in range(inp["nimg"]):
        for pr in range(rpi):
            s = pr if si is None else int(si[pr])
            if si is None:
                v = inp["srcA"][b * rpi + pr]
            else:
                v = inp["srcA"][b * inp["rowsA"] + s] if s >= 0 else inp["srcB"][b * inp["rowsB"] + (-s - 1)]
            v = v.to(F64)
            if add is not None:
                a = pr if ai is None else int(ai[pr])
                if a >= 0:
                    v = v + add[a].to(F64)
            rows.append(v)
    return torch.stack(rows).view(-1, C)


def _d(t):
    return None if t is None else t.to(F64)


def _attn_sub(inp, x):
    C, S, heads = inp["C"], inp["S"], inp["heads"]
    xn = F.layer_norm(x.view(-1, S, C), (C,), _d(inp["ln_w"]), _d(inp["ln_b"]), inp["eps"])
    q, k, v = F.linear(xn, _d(inp["wqkv"]), _d(inp["bqkv"])).view(-1, S, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=_d(inp["bias"]), scale=inp["scale"])
    y = F.linear(o.transpose(1, 2).reshape(-1, C), _d(inp["wproj"]), _d(inp["bproj"]))
    return y * _d(inp["gamma"]) if inp.get("gamma") is not None else y


def _mlp_sub(inp, x, pre=""):
    xn = F.layer_norm(x, (inp["C"],), _d(inp[pre + "ln_w"]), _d(inp[pre + "ln_b"]), inp["eps"])
    y = F.linear(F.gelu(F.linear(xn, _d(inp["w1"]), _d(inp["b1"]))), _d(inp["w2"]), _d(inp["b2"]))
    return y * _d(inp[pre + "gamma"]) if inp.get(pre + "gamma") is not None else y


def _independent(chain, inp):
    xin = _gather_loop(inp)
    if chain == "attn_block":
        return _attn_sub(inp, xin), xin
    if chain == "ct_block":
        ct1 = xin + _attn_sub(inp, xin)
        return ct1 + _mlp_sub(inp, ct1, "ln2_") - xin, xin
    if chain == "mlp":
        return _mlp_sub(inp, xin), xin
    y = F.linear(F.layer_norm(xin, (inp["C"],), _d(inp["ln_w"]), _d(inp["ln_b"]), inp["eps"]), _d(inp["W"]), _d(inp["bias"]))
    return (F.gelu(y) if inp["act"] else y), xin


@pytest.mark.parametrize("cid,chain,make", CASES, ids=[c[0] for c in CASES])
def test_exact_matches_independent_statement(cid, chain, make):
    inp = _inp(cid, make)
    got, xin = R.CHAIN[chain].exact(inp)
    want, xin_want = _independent(chain, inp)
    assert got.dtype == F64 and torch.equal(xin, xin_want)
    err, peak = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= EXACT_RTOL * peak, f"{cid}: exact vs the independent statement {err:.3e} (largest entry {peak:.3e})"
    # the inputs are the ones the issue of the masked keys needs: a hot row, a bias table far below zero, garbage behind every buffer
    hot = xin.mean(1).abs().max().item()
    assert abs(hot - R.HOT_MEAN) < 2.0 and xin.abs().max().item() < R.HOT_MEAN + 10.0, f"{cid}: gathered rows reach {xin.abs().max().item():.1f}"
    assert inp["srcA"][-R.SPARE:].abs().mean().item() > 100.0
    if "bias" in inp and chain != "ln_gemm":
        assert -9.0 < inp["bias"].mean().item() < -7.0


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the bar is one the arithmetic meets with room: F = 2 x the worst variant
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _as_got(chain, t, dt):
    return R.rounded(t, dt) if chain == "ln_gemm" else t


@pytest.mark.parametrize("chain", R.CHAINS)
def test_variants_meet_half_the_bar(chain):
    assert 2.0 <= R.F_MAX[chain] <= 4.0 and 2.0 <= R.F_RMS[chain] <= 4.0
    worst = {}
    for cid, ch, make in CASES:
        if ch != chain:
            continue
        for seed in R.STUDY_SEEDS:
            inp = make(seed)
            exact, xin = R.CHAIN[chain].exact(inp)
            plain, _ = R.CHAIN[chain].plain16(inp)
            for name, opt in [("base", {})] + list(R.VARIANTS.items()):
                if name == "p_after_norm" and chain not in ("attn_block", "ct_block"):
                    continue
                var = plain if name == "base" else R.CHAIN[chain].plain16(inp, **opt)[0]
                rmax, rrms = R.ratios(chain, _as_got(chain, var, inp["dt"]), exact, plain, xin, inp["dt"])
                if chain == "ln_gemm":     # a correct rounding of the output may use all of the bar's u_T * |exact| + sub_T: half the bar is asked before it
                    assert rmax <= 1.0, f"{cid} seed {seed} {name}: rounded to T {rmax:.3f} x the max bar"
                    rmax = R.ratios(chain, var, exact, plain, xin, inp["dt"])[0]
                smax, srms = R.variant_ratios(exact, plain, var)
                w = worst.setdefault(name, [0.0, 0.0, 0.0, 0.0])
                w[:] = [max(a, b) for a, b in zip(w, (rmax, rrms, smax, srms))]
                assert rmax <= 0.5 and rrms <= 0.5, f"{cid} seed {seed} {name}: {rmax:.3f} x the max bar, {rrms:.3f} x the rms bar"
    for name, w in worst.items():
        print(f"{chain} {name}: worst {w[0]:.3f} x max bar, {w[1]:.3f} x rms bar (error / base plain16 error: max {w[2]:.3f}, rms {w[3]:.3f}); "
              f"F_max {R.F_MAX[chain]} F_rms {R.F_RMS[chain]}")


# ------------------------------------------------------------------------------------------------------------------------------------------------
# teeth
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _mutants(chain, inp):
    """The mutants that apply to this case."""
    tables, gamma = inp.get("src_idx") is not None and (inp["src_idx"] < 0).any().item(), inp.get("gamma") is not None
    rows = inp["nimg"] * inp.get("rows_per_image", 1)
    out = []
    if chain in ("attn_block", "ct_block"):
        S = inp["S"]
        out += ["proj_bias_tile"]
        out += ["leak_key"] if S < R.spad(S) else []
        out += ["drop_last_key", "head_bias_shift", "bias_transposed"] if S > 1 else []      # one key: the softmax is 1 whatever the bias
    if chain == "ct_block":
        out += ["ln2_pre_residual"] + (["gamma2_one"] if gamma else [])
    if chain != "attn_block":
        out += ["fc1_bias_tile"]
    if chain in ("ct_block", "mlp"):
        out += ["fc2_bias_channel"]
    if chain != "ln_gemm" and gamma:
        out += ["gamma_one"]
    if inp.get("add") is not None:
        out += ["add_ignored_one_row"]
    if tables:
        out += ["neg_src_neighbour"]
    if rows > 1:
        out += ["last_row_from_prev"]
    return out


@pytest.mark.parametrize("cid,chain,make", CASES, ids=[c[0] for c in CASES])
def test_mutants_exceed_the_bar(cid, chain, make):
    inp = _inp(cid, make)
    exact, xin = R.CHAIN[chain].exact(inp)
    plain, _ = R.CHAIN[chain].plain16(inp)
    names = _mutants(chain, inp)
    assert names
    line = []
    for name in names:
        mut, _ = R.CHAIN[chain].plain16(inp, mut=name)
        rmax, rrms = R.ratios(chain, _as_got(chain, mut, inp["dt"]), exact, plain, xin, inp["dt"])
        line.append(f"{name} {rmax:.1f}")
        assert rmax >= 2.0, f"{cid}: mutant {name} is only {rmax:.2f} x the max bar ({rrms:.2f} x the rms bar)"
    print(f"{cid}: " + "  ".join(line))


def test_every_mutant_of_the_list_runs_somewhere():
    seen = set()
    for cid, chain, make in CASES:
        seen.update((chain, m) for m in _mutants(chain, _inp(cid, make)))
    want = {("attn_block", m) for m in ("leak_key", "drop_last_key", "head_bias_shift", "bias_transposed", "add_ignored_one_row", "neg_src_neighbour",
                                        "gamma_one", "proj_bias_tile", "last_row_from_prev")}
    want |= {("ct_block", m) for m in ("leak_key", "drop_last_key", "head_bias_shift", "bias_transposed", "add_ignored_one_row", "gamma_one", "gamma2_one",
                                      "proj_bias_tile", "fc1_bias_tile", "fc2_bias_channel", "ln2_pre_residual", "last_row_from_prev")}
    want |= {("mlp", m) for m in ("gamma_one", "fc1_bias_tile", "fc2_bias_channel", "last_row_from_prev")}
    want |= {("ln_gemm", m) for m in ("add_ignored_one_row", "neg_src_neighbour", "fc1_bias_tile", "last_row_from_prev")}
    assert seen == want


def test_tanh_gelu_is_below_resolution():
    """Measured, not asserted: the tanh form against the erf form, in units of the max bar."""
    for cid, chain, make in CASES:
        if chain not in ("mlp", "ct_block") or "-300-" in cid:
            continue
        inp = _inp(cid, make)
        exact, xin = R.CHAIN[chain].exact(inp)
        plain, _ = R.CHAIN[chain].plain16(inp)
        mut, _ = R.CHAIN[chain].plain16(inp, gelu="tanh")
        rmax, rrms = R.ratios(chain, mut, exact, plain, xin, inp["dt"])
        print(f"{cid}: tanh-GELU moves the branch by {(mut - plain).abs().max().item():.2e}, e16 {(plain.double() - exact).abs().max().item():.2e}: "
              f"{rmax:.2f} x the max bar, {rrms:.2f} x the rms bar")
        assert torch.isfinite(mut).all()
