"""Backward of the attention core for windows and carrier grids of MORE than 64 tokens (csrc/fvit_attnbwd.hip, fvit_bwd_window_attention_long) and the
training path built on it (hat_backward with ``long_sequences``, FasterViT.enable_hat_backward(True, long_sequences=True)).

Kernel level: through the C ABI against fp32 torch.autograd of the same core on the device, from the SAME 16-bit operands (so the figures are the
kernel's own error: P and dS narrowed to 16 bits for the MFMAs, 16-bit dq / dk / dv), each gradient as max-abs error over the reference's largest entry.
Bars: for S <= 64 the project's sub-block bars (fp16 5e-3, bf16 4e-2; tests/test_gpu_backward.py); for S > 64 about twice the worst case MEASURED on
the MI355X over all cases of the table below (recorded next to the bars)."""
import ctypes

import pytest
import torch

from fastervit_amd import _lib, hat_backward
from tests.backward_long_util import gather_compact

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 1, torch.bfloat16: 2}
SHORT_BAR = {torch.float16: 5e-3, torch.bfloat16: 4e-2}     # S <= 64: tests/test_gpu_backward.py:86
# S > 64, measured on the MI355X over every case of LONG_CASES (worst case of dq / dk / dv, and of the bias gradient); bars = 2 x measured:
#   fp16  dq / dk / dv 7.7e-4 (dv, S = 130, no bias; 5.6e-4 at S = 240, 5.3e-4 at S = 2304)     bias gradient 1.2e-6 (compact, S = 2304)
#   bf16  dq / dk / dv 5.3e-3 (dk, S = 130; 5.0e-3 at S = 576)                                   bias gradient 8.1e-7 (compact, S = 2304)
# The same kernel at S = 49 / 64 measures 5.6e-4 / 4.4e-3 (the scalar fp32 kernel beside it 4.3e-4 / 3.2e-3): no growth with the length.  The bias
# gradient is summed from the fp32 dS before anything is narrowed, hence its fp32-sized error in both operand types.
LONG_BAR = {torch.float16: 1.6e-3, torch.bfloat16: 1.1e-2}
LONG_BIAS_BAR = {torch.float16: 2.5e-6, torch.bfloat16: 2.5e-6}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dpad(d):
    return 32 if d <= 32 else (64 if d <= 64 else 96)


def _inputs(dt, nwin, S, heads, d, seed):
    """q, k, v, dO as 16-bit-representable fp32 (nwin, heads, S, d) + the kernel's padded operand buffers."""
    D = _dpad(d)
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v, do = ((torch.randn(nwin, heads, S, d, generator=g) * sc).to(dt).float().cuda() for sc in (1.0, 1.0, 1.0, 1.0))
    qkv = torch.zeros(nwin * S, 3, heads, D, dtype=dt, device="cuda")
    for i, t in enumerate((q, k, v)):
        qkv[:, i, :, :d] = t.permute(0, 2, 1, 3).reshape(nwin * S, heads, d).to(dt)
    dO = torch.zeros(nwin * S, heads, D, dtype=dt, device="cuda")
    dO[:, :, :d] = do.permute(0, 2, 1, 3).reshape(nwin * S, heads, d).to(dt)
    return q, k, v, do, qkv.view(nwin * S, 3 * heads * D), dO.view(nwin * S, heads * D), D


def _reference(q, k, v, do, scale, bias=None, rel=None, w=0, ng=0):
    """fp32 autograd of the core on the device; returns dq, dk, dv, d(bias leaf)."""
    S = q.shape[2]
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    bl = None
    att = (leaves[0] @ leaves[1].transpose(-1, -2)) * scale
    if bias is not None:
        bl = bias.clone().requires_grad_(True)
        att = att + bl
    elif rel is not None:
        bl = rel.clone().requires_grad_(True)
        att = att + gather_compact(bl, w, ng, S)
    (att.softmax(-1) @ leaves[2]).backward(do)
    return leaves[0].grad, leaves[1].grad, leaves[2].grad, (bl.grad if bl is not None else None)


def _run_long(dt, qkv, dO, nwin, S, heads, D, scale, bias=None, rel=None, w=0, ng=0, dbias=None):
    lib = _lib.lib()
    spad = 0
    btab = None
    if bias is not None:
        spad = lib.fvit_attention_spad(S)
        btab = torch.zeros(heads, spad, spad, device="cuda")
        btab[:, :S, :S] = bias
        btab[:, :, S:] = _lib.FVIT_MASK_BIAS
    nbytes = lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, D, w if (rel is not None and dbias is not None) else 0)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    dqkv = torch.full_like(qkv, float("nan"))
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = lib.fvit_bwd_window_attention_long(CODE[dt], qkv.data_ptr(), qkv.shape[1], dO.data_ptr(), dO.shape[1], p(btab), spad, p(rel), w, ng,
                                            ctypes.c_float(scale), dqkv.data_ptr(), p(dbias), ws.data_ptr(), nbytes, nwin, S, heads, D, _stream())
    _lib.check(rc, "fvit_bwd_window_attention_long")
    torch.cuda.synchronize()
    return dqkv


def _split(dqkv, nwin, S, heads, D, d):
    t = dqkv.float().view(nwin, S, 3, heads, D)
    assert torch.isfinite(t).all()
    assert (t[..., d:] == 0).all()          # zero pad channels receive zero gradients
    return [t[:, :, i, :, :d].permute(0, 2, 1, 3) for i in range(3)]


def _err(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def _bias_of(kind, heads, S, w, ng, seed, lead0=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 99)
    if kind == "dense":
        b = torch.randn(heads, S, S, generator=g).cuda()
        if lead0:
            b[:, :lead0] = 0
            b[:, :, :lead0] = 0
        return dict(bias=b)
    if kind == "compact":
        return dict(rel=(torch.randn(heads, (2 * w - 1) ** 2, generator=g) * 2).cuda(), w=w, ng=ng)
    return {}


# (nwin, S, heads, real head_dim, bias form, w, ng, leading zero-bias tokens of the dense table)
LONG_CASES = [
    (3, 65, 8, 32, "dense", 0, 0, 0),        # first size over the old limit, ragged last tile
    (2, 144, 4, 32, "dense", 0, 0, 0),       # 12^2 window (21k-384 stage 3)
    (2, 100, 4, 49, "dense", 0, 0, 4),       # padded head_dim, carrier rows in front
    (2, 576, 2, 32, "compact", 24, 0, 0),    # 21k-384 stage 2
    (1, 576, 16, 49, "compact", 24, 0, 0),   # FasterViT-4's real width, bias partial memory
    (2, 400, 4, 32, "compact", 20, 0, 0),    # ragged last tile
    (2, 240, 4, 32, "compact", 15, 15, 0),   # rel_ng > 0: rows / columns without bias get none and give none
    (1, 2304, 1, 80, "compact", 48, 0, 0),   # longest registry window, D = 96
    (4, 130, 4, 32, "none", 0, 0, 0),        # no bias
]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nwin,S,heads,d,kind,w,ng,lead0", LONG_CASES)
def test_long_attention_backward_kernel_vs_autograd(dt, nwin, S, heads, d, kind, w, ng, lead0):
    q, k, v, do, qkv, dO, D = _inputs(dt, nwin, S, heads, d, seed=S * 7 + heads)
    scale = d ** -0.5
    bk = _bias_of(kind, heads, S, w, ng, S, lead0)
    rq, rk, rv, rb = _reference(q, k, v, do, scale, **bk)
    dbias = None
    if kind == "dense":
        dbias = torch.zeros(heads, S, S, device="cuda")
    elif kind == "compact":
        dbias = torch.zeros(heads, (2 * w - 1) ** 2, device="cuda")
    dqkv = _run_long(dt, qkv, dO, nwin, S, heads, D, scale, dbias=dbias, **bk)
    gq, gk, gv = _split(dqkv, nwin, S, heads, D, d)
    errs = dict(dq=_err(gq, rq), dk=_err(gk, rk), dv=_err(gv, rv))
    if dbias is not None:
        assert torch.isfinite(dbias).all()
        errs["dbias"] = _err(dbias, rb)
        if kind == "compact" and ng:   # tokens in front of the bias window give no gradient: the table gradient equals the window block's alone
            assert rb.abs().max().item() > 0
    print(f"long attention backward {dt} nwin={nwin} S={S} heads={heads} d={d} {kind}: " + " ".join(f"{n}={e:.3e}" for n, e in errs.items()))
    for n, e in errs.items():
        bar = LONG_BIAS_BAR[dt] if n == "dbias" else LONG_BAR[dt]
        assert e < bar, f"{n}: {e:.3e} of the reference's largest entry (bar {bar:.1e})"
    # bit-reproducible, and the bias gradient ACCUMULATES: a second call into the same buffer doubles it exactly
    first = dbias.clone() if dbias is not None else None
    dqkv2 = _run_long(dt, qkv, dO, nwin, S, heads, D, scale, dbias=dbias, **bk)
    assert torch.equal(dqkv, dqkv2)
    if dbias is not None:
        assert torch.equal(dbias, 2 * first)
        fresh = torch.zeros_like(first)
        _run_long(dt, qkv, dO, nwin, S, heads, D, scale, dbias=fresh, **bk)
        assert torch.equal(fresh, first)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("S", [49, 64])
def test_long_kernel_overlaps_the_short_one(dt, S):
    """S <= 64: both kernels against the same reference at the project's existing bars, and the new one against the old one's output."""
    nwin, heads, d = 5, 8, 32
    lib = _lib.lib()
    q, k, v, do, qkv, dO, D = _inputs(dt, nwin, S, heads, d, seed=S)
    scale = d ** -0.5
    bias = _bias_of("dense", heads, S, 0, 0, S)["bias"]
    rq, rk, rv, rb = _reference(q, k, v, do, scale, bias=bias)
    dbias = torch.zeros(heads, S, S, device="cuda")
    new = _run_long(dt, qkv, dO, nwin, S, heads, D, scale, bias=bias, dbias=dbias)
    spad = lib.fvit_attention_spad(S)
    btab = torch.zeros(heads, spad, spad, device="cuda")
    btab[:, :S, :S] = bias
    old = torch.zeros_like(qkv)
    part = torch.empty(nwin, heads, S, S, device="cuda")
    _lib.check(lib.fvit_bwd_window_attention(CODE[dt], qkv.data_ptr(), qkv.shape[1], dO.data_ptr(), dO.shape[1], btab.data_ptr(), spad, ctypes.c_float(scale),
                                             old.data_ptr(), part.data_ptr(), nwin, S, heads, D, _stream()), "fvit_bwd_window_attention")
    torch.cuda.synchronize()
    tol = SHORT_BAR[dt]
    refs = (rq, rk, rv)
    for name, buf, db in (("new", new, dbias), ("old", old, part.sum(0))):
        for n, a, b in zip(("dq", "dk", "dv"), _split(buf, nwin, S, heads, D, d), refs):
            e = _err(a, b)
            print(f"S={S} {dt} {name} kernel {n}: {e:.3e}")
            assert e < tol, f"{name} {n}: {e:.3e}"
        e = _err(db, rb)
        print(f"S={S} {dt} {name} kernel dbias: {e:.3e}")
        assert e < tol, f"{name} dbias: {e:.3e}"
    for n, a, b in zip(("dq", "dk", "dv"), _split(new, nwin, S, heads, D, d), _split(old, nwin, S, heads, D, d)):
        assert _err(a, b) < tol, f"new vs old {n}: {_err(a, b):.3e}"
    assert _err(dbias, part.sum(0)) < tol


def test_long_attention_backward_rejects_bad_arguments():
    lib = _lib.lib()
    nwin, S, heads, D = 1, 100, 2, 32
    qkv = torch.zeros(nwin * S, 3 * heads * D, dtype=torch.float16, device="cuda")
    dO = torch.zeros(nwin * S, heads * D, dtype=torch.float16, device="cuda")
    dqkv = torch.zeros_like(qkv)
    bias = torch.zeros(heads, 112, 112, device="cuda")
    rel = torch.zeros(heads, 19 * 19, device="cuda")
    nbytes = lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, D, 10)
    assert nbytes == (2 * nwin * heads * 128 + heads * S * S) * 4
    assert lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, D, 0) == 2 * nwin * heads * 128 * 4
    ws = torch.zeros(nbytes // 4, device="cuda")

    def call(qkv_=qkv, dO_=dO, bias_=None, spad=0, rel_=None, w=0, ng=0, dqkv_=dqkv, dbias=None, ws_=ws, nb=nbytes, S_=S, D_=D, code=1):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return lib.fvit_bwd_window_attention_long(code, p(qkv_), 3 * heads * D, p(dO_), heads * D, p(bias_), spad, p(rel_), w, ng, ctypes.c_float(1.0),
                                                  p(dqkv_), p(dbias), p(ws_), nb, nwin, S_, heads, D_, _stream())

    assert call(bias_=bias, spad=112) == 0
    assert call(rel_=rel, w=10, ng=0) == 0
    assert call(bias_=bias, spad=112, rel_=rel, w=10, ng=0) == -1 and b"not both" in lib.fvit_last_error()
    assert call(rel_=rel, w=10, ng=1) == -1 and b"n_g + w^2 == S" in lib.fvit_last_error()
    assert call(rel_=rel, w=9, ng=0) == -1
    assert call(bias_=bias, spad=96) == -1
    assert call(D_=48) == -1 and b"32 / 64 / 96" in lib.fvit_last_error()
    assert call(code=0) == -1
    assert call(nb=1024) == -2 and b"workspace" in lib.fvit_last_error()
    assert call(rel_=rel, w=10, ng=0, dbias=rel, nb=2 * nwin * heads * 128 * 4) == -2   # the compact bias gradient needs the window-sum scratch
    assert call(qkv_=None) == -1 and call(dO_=None) == -1 and call(dqkv_=None) == -1 and call(ws_=None) == -1
    assert call(S_=0) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------------------------
# stage level: hat_backward with ``long_sequences`` against torch.autograd through the CPU oracle
# ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = dict(depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)
ANYRES = dict(TINY, window_size=[7, 7, 7, 7], ct_size=2)
# (entry, kwargs, input size, levels, batch).  Measured on the MI355X (fp16 operands, 'stress' weights), max-abs error over the reference gradient's largest
# entry, dx / worst parameter gradient:  21k-384 level 2 (S = 576) 5.3e-4 / 1.1e-3, level 3 (S = 144) 5.7e-4 / 8.1e-4;  any-res 448 x 672 (G = 96)
# 9.6e-4 / 2.2e-3 (a cpb_mlp weight of hat_attn);  any-res 672 x 1120 (G = 240) 1.2e-3 / 1.5e-3.
STAGES = [
    ("faster_vit_4_21k_384", TINY, (384, 384), (2, 3), 2),                          # 576-token window (compact table), 144-token window (dense table)
    ("faster_vit_4_any_res", dict(ANYRES, resolution=[448, 672]), (448, 672), (2,), 2),    # carrier grid 4 x 6 windows, G = 96 (dense), last-block propagation
    ("faster_vit_4_any_res", dict(ANYRES, resolution=[672, 1120]), (672, 1120), (2,), 2),  # 6 x 10 windows, G = 240 (compact, non-square: zero-padded grid part)
]
STAGE_DX_BAR, STAGE_PARAM_BAR = 2.5e-3, 4.5e-3   # ~2 x the measured worst cases above (the stage bars for S <= 64 are 2e-2 / 3e-2)


@pytest.mark.parametrize("entry,kwargs,hw,levels,batch", STAGES)
def test_long_stage_backward_vs_oracle_autograd(entry, kwargs, hw, levels, batch):
    """local_stage_backward / hier_stage_backward with windows / carrier grids above 64 tokens: dx and the gradient of every parameter of ``layer.blocks`` and
    ``layer.global_tokenizer`` (the cpb_mlp of both position-bias modules included) against torch.autograd through oracle.hat_reference.hat_stage on the
    same synthetic 'stress' weights; the train-mode forward chain reproduces the oracle's forward."""
    import fastervit_amd
    from oracle import hat_reference as hr
    from tests.synth import synth_state_dict
    torch.manual_seed(0)
    model = fastervit_amd.create_model(entry, **kwargs).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=77, family="stress"))
    model.enable_hat_backward(True, long_sequences=True)
    g = torch.Generator(device="cpu").manual_seed(9)
    for li in levels:
        layer = model.levels[li]
        b0 = layer.blocks[0]
        C = b0.attn.qkv.in_features
        H, W = hw[0] // (4 * 2 ** li), hw[1] // (4 * 2 ** li)
        ncw = b0.cr_window ** 2 if b0.do_sr_hat else 0
        S = b0.window_size ** 2 + ncw
        G = ncw * b0.sr_ratio[0] * b0.sr_ratio[1] if b0.do_sr_hat else 0
        assert max(S, G) > 64
        if b0.do_sr_hat:
            assert layer.blocks[-1].do_propagation      # FasterViT-3 and up: the last block's carrier propagation with G > 64
        x = torch.randn(batch, C, H, W, generator=g)
        dy = torch.randn(batch, C, H, W, generator=g)
        sd = {k: v.detach().clone().float().requires_grad_(v.dtype.is_floating_point) for k, v in layer.state_dict().items()}
        xr = x.clone().requires_grad_(True)
        out = hr.hat_stage(xr, sd, "", depth=len(layer.blocks), heads=b0.attn.num_heads, ws=layer.window_size, cw=b0.cr_window, input_resolution=[H, W],
                           only_local=not b0.do_sr_hat, do_propagation=bool(b0.do_propagation), any_res=layer.any_res)
        out.backward(dy)
        ref = {k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None and (k.startswith("blocks.") or k.startswith("global_tokenizer."))}
        layer = layer.cuda()
        for p in layer.parameters():
            p.grad = None
        fn = hat_backward.hier_stage_backward if b0.do_sr_hat else hat_backward.local_stage_backward
        dx = fn(layer, x.cuda(), dy.cuda())
        torch.cuda.synchronize()
        y = hat_backward.stage_forward_train(layer, x.cuda()).cpu()
        assert (y - out.detach()).abs().max().item() < 1e-2 * out.abs().max().item(), f"{entry} level {li}: forward chain"
        err, scale = (dx.cpu() - xr.grad).abs().max().item(), xr.grad.abs().max().item()
        got = dict(layer.named_parameters())
        checked, worst, worst_k, cpb = 0, 0.0, "", 0
        for k, r in ref.items():
            if k not in got:
                continue
            assert got[k].grad is not None, f"{entry} level {li}: no gradient for {k}"
            a = got[k].grad.float().cpu()
            assert torch.isfinite(a).all(), k
            e = (a - r).abs().max().item() / (r.abs().max().item() + 1e-30)
            if e > worst:
                worst, worst_k = e, k
            cpb += "pos_emb_funct.cpb_mlp" in k
            checked += 1
        print(f"long stage {entry} {hw} level {li} (S = {S}, G = {G}): {checked} parameter gradients, worst {worst:.3e} ({worst_k}); dx {err / scale:.3e}")
        assert err < STAGE_DX_BAR * scale, f"{entry} level {li} dx: {err:.3e} vs {scale:.3e}"
        assert worst < STAGE_PARAM_BAR, f"{entry} level {li} {worst_k}: {worst:.3e}"
        assert checked >= 14 * len(layer.blocks) and cpb >= (2 if b0.do_sr_hat else 1) * 3 * len(layer.blocks)
        # a carrier-free stage is kernels and row permutations only: bit-reproducible as a whole.  (A hierarchical stage also runs PyTorch's index_add_
        # for the propagation and MIOpen's convolution backward for the tokenizer, which are not run-to-run deterministic; the kernel tests above cover it.)
        if not b0.do_sr_hat:
            for p in layer.parameters():
                p.grad = None
            dx2 = fn(layer, x.cuda(), dy.cuda())
            assert torch.equal(dx, dx2)
        model.levels[li] = layer.cpu()


# ------------------------------------------------------------------------------------------------------------------------------------------------
# model level: the reduced faster_vit_4_21k_384 (one window of 576 / 144 tokens in stages 2 / 3)
# ------------------------------------------------------------------------------------------------------------------------------------------------
MODEL_L2_BAR = 1.6e-4   # relative L2 over all 115 parameter gradients: measured 7.9e-5 on the MI355X (worst tensor 7.0e-4 of its largest entry); FasterViT-0: 3.6e-4


def test_whole_model_gradients_of_a_576_token_model_vs_oracle_autograd():
    import fastervit_amd
    from oracle import model_reference as mr
    from tests.cases import _arch
    from tests.synth import synth_state_dict
    torch.manual_seed(0)
    model = fastervit_amd.create_model("faster_vit_4_21k_384", **TINY).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1234, family="init"))
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(2, 3, 384, 384, generator=g)
    r = torch.randn(2, 1000, generator=g)
    sd = {k: (v.detach().clone().float().requires_grad_(True) if v.dtype.is_floating_point and "running_" not in k and "num_batches" not in k
              else v.detach().clone()) for k, v in model.state_dict().items()}
    arch = _arch(TINY["depths"], TINY["num_heads"], [7, 7, 24, 12], 16, 384, hat=[False] * 4, prop=True)
    (mr.model_forward(sd, x, arch) * r).sum().backward()
    model = model.cuda()
    with pytest.raises(RuntimeError, match="no kernel-sequence backward"):
        model.enable_hat_backward(True)                      # the default stays what it was
    model.enable_hat_backward(True, long_sequences=True)
    logits = model(x.cuda())
    assert logits.grad_fn is not None
    (logits * r.cuda()).sum().backward()
    torch.cuda.synchronize()
    num = den = worst = 0.0
    n = 0
    for k, p in model.named_parameters():
        ref = sd[k].grad if k in sd and isinstance(sd[k], torch.Tensor) and sd[k].requires_grad else None
        if ref is None:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        diff = p.grad.float().cpu() - ref
        worst = max(worst, diff.abs().max().item() / (ref.abs().max().item() + 1e-30))
        num += diff.double().pow(2).sum().item()
        den += ref.double().pow(2).sum().item()
        n += 1
    l2 = (num / den) ** 0.5
    print(f"576-token model: {n} tensors, worst per-tensor max-abs / max {worst:.3e}, relative L2 over all {l2:.3e}")
    assert n > 100 and l2 < MODEL_L2_BAR, f"relative L2 error of all parameter gradients {l2:.3e}"


def test_training_a_576_token_model():
    """model.train() with stochastic depth: a step runs, every parameter gets a finite gradient, a few AdamW steps on a fixed batch reduce the loss; train
    mode with attn_drop_rate > 0 is refused at FORWARD time, by name."""
    import torch.nn.functional as F
    import fastervit_amd
    torch.manual_seed(0)
    model = fastervit_amd.create_model("faster_vit_4_21k_384", drop_path_rate=0.1, num_classes=10, **TINY).cuda()
    model.enable_hat_backward(True, long_sequences=True).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(8, 3, 384, 384, generator=g).cuda()
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    losses = []
    for step in range(8):
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        if step == 0:
            missing = [k for k, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
            assert not missing, missing[:5]
        opt.step()
        losses.append(loss.item())
    print("576-token model training losses:", [round(v, 4) for v in losses])
    assert losses[-1] < 0.7 * losses[0], losses
    bad = fastervit_amd.create_model("faster_vit_4_21k_384", attn_drop_rate=0.1, **TINY).cuda().eval().enable_hat_backward(True, long_sequences=True).train()
    with pytest.raises(RuntimeError, match="attn_drop = 0.1 in train mode on windows of 576 tokens"):
        bad(x[:2])
    plain = fastervit_amd.create_model("faster_vit_4_21k_384", **TINY).cuda().train()     # without the flag: today's refusal
    with pytest.raises(RuntimeError, match="holds at most 64"):
        plain(x[:2])
