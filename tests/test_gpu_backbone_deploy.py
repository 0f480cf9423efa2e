"""Deploy plan and graph runner of the detection backbone on the GPU: the two glue kernels (fvit_map_pad_cl, fvit_layernorm2d_crop_cl) bit for bit
against torch / the dense LayerNorm2d kernel, the 16-bit plan against the reference goldens, the runner against eager deploy, the pinning of the
per-geometry stage state against the LRU of hat_runtime, weight updates, and the untouched grad / train / module paths.

Measured on MI355X, per-level max|d| / max|ref| of eager deploy against the goldens, worst level of each case (module mode 'f16': 8.7e-4):
fp16  bb_fvit0_160x192 9.5e-4, bb_tiny_21k_384 8.5e-4, bb_tiny_exact 1.06e-3, bb_tiny_g8 1.09e-3, bb_tiny_odd 1.24e-3, bb_tiny_wide 9.6e-4;
bf16  bb_tiny_odd 9.6e-3.  ``BOUND`` = 2 x the worst value of each dtype."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fastervit_amd
from fastervit_amd import _lib, hat_runtime
from tests.backbone_cases import BACKBONE_CASES, BATCH, SEED, make_mask
from tests.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
# per-level max|d| / max|ref| of eager deploy against the goldens: 2 x the worst measured value of each dtype (fp16 1.24e-3, bf16 9.57e-3: DESIGN section 11)
BOUND = {torch.float16: 2.5e-3, torch.bfloat16: 1.9e-2}
CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}
DTYPES = [torch.float16, torch.bfloat16]
_TINY = dict(depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)
# (C, H, W, Hp, Wp): bottom pad only; both pads; one pixel into a whole window; no pad (a copy)
GEOMETRIES = [(64, 13, 21, 14, 21), (128, 5, 9, 7, 14), (8, 1, 1, 7, 7), (64, 14, 14, 14, 14)]


class _Nested:
    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _model(name, kwargs, family, sd=None):
    m = fastervit_amd.build_fastervit(name, **kwargs)
    if sd is None:
        sd = synth_state_dict(m.state_dict(), SEED, family)
    m.load_state_dict(sd, strict=True)
    return m.eval().to(DEV).requires_grad_(False), sd


def _case_model(name):
    case = BACKBONE_CASES[name]
    return _model(case["name"], case["kwargs"], case["family"])[0], synth_input(BATCH, *case["hw"], SEED).to(DEV)


def _rel(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item() / b.double().abs().max().item()


# ---- the two kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,H,W,Hp,Wp", GEOMETRIES)
def test_map_pad_equals_f_pad(C, H, W, Hp, Wp, dt):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(C + 31 * H + W)
    x = torch.randn(BATCH, H, W, C, generator=g).to(dt).to(DEV)            # [B][H][W][C]
    want = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
    outs = []
    for _ in range(2):
        out = torch.full((BATCH, Hp, Wp, C), float("nan"), dtype=dt, device=DEV)   # every pixel must be written
        _lib.check(lib.fvit_map_pad_cl(CODE[dt], x.data_ptr(), out.data_ptr(), BATCH, H, W, Hp, Wp, C, _stream()), "fvit_map_pad_cl")
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want) and torch.equal(outs[1], outs[0])


def test_map_pad_error_returns():
    lib = _lib.lib()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV)
    out = torch.full((1, 8, 8, 64), 3.0, dtype=torch.float16, device=DEV)
    for H, W, Hp, Wp, C in [(8, 8, 7, 8, 64), (8, 8, 8, 7, 64), (8, 8, 8, 8, 12)]:
        assert lib.fvit_map_pad_cl(_lib.FVIT_F16, x.data_ptr(), out.data_ptr(), 1, H, W, Hp, Wp, C, _stream()) != 0
        assert b"map_pad" in lib.fvit_last_error()
    torch.cuda.synchronize()
    assert (out == 3.0).all()   # nothing was launched


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,Cv,H,W,Hp,Wp", [(64, 64, 13, 21, 14, 21), (128, 128, 5, 9, 7, 14), (64, 64, 14, 14, 14, 14),
                                             (64, 32, 13, 21, 14, 21), (256, 196, 5, 9, 7, 14)])
def test_layernorm2d_crop_equals_dense_kernel_on_the_crop(C, Cv, H, W, Hp, Wp, dt):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(C + Cv + 31 * H + W)
    xp = torch.zeros(BATCH, Hp, Wp, C)
    xp[..., :Cv] = torch.randn(BATCH, Hp, Wp, Cv, generator=g) * 2 + 0.3       # the pad PIXELS hold values (a conv level's), the pad CHANNELS zeros
    xp = xp.to(dt).to(DEV)
    w, b = torch.zeros(C), torch.zeros(C)
    w[:Cv] = torch.rand(Cv, generator=g) + 0.5
    b[:Cv] = torch.randn(Cv, generator=g)
    w, b = w.to(DEV), b.to(DEV)
    eps = ctypes.c_float(1e-6)
    crop = xp[:, :H, :W].contiguous()
    dense = torch.full_like(crop, float("nan"))
    _lib.check(lib.fvit_layernorm2d_cl(CODE[dt], crop.data_ptr(), dense.data_ptr(), w.data_ptr(), b.data_ptr(), eps, BATCH * H * W, C, Cv, _stream()),
               "fvit_layernorm2d_cl")
    outs = []
    for _ in range(2):
        out = torch.full_like(crop, float("nan"))
        _lib.check(lib.fvit_layernorm2d_crop_cl(CODE[dt], xp.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), eps, BATCH, H, W, Hp, Wp, C, Cv,
                                                _stream()), "fvit_layernorm2d_crop_cl")
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], dense) and torch.equal(outs[1], outs[0])
    assert outs[0][..., Cv:].abs().max().item() == 0.0 if Cv < C else True
    # within the dense kernel's own error of fp32 F.layer_norm, which is one rounding of the result to 16 bits (fp32 statistics): 1 ulp allowed
    ref = F.layer_norm(crop[..., :Cv].float(), (Cv,), w[:Cv], b[:Cv], 1e-6)
    e_crop, e_dense = ((o[..., :Cv].float() - ref).abs().max().item() for o in (outs[0], dense))
    ulp = 2.0 ** (-10 if dt == torch.float16 else -7)
    print(f"ln2d crop C={C} Cv={Cv} {dt}: err {e_crop:.3e} dense {e_dense:.3e} |ref| {ref.abs().max().item():.2f}")
    assert e_crop <= e_dense <= ulp * max(ref.abs().max().item(), 1.0)


def test_layernorm2d_crop_error_returns():
    lib = _lib.lib()
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV)
    w = torch.ones(64, device=DEV)
    for H, W, Hp, Wp, C in [(8, 8, 7, 8, 64), (8, 8, 8, 7, 64), (8, 8, 8, 8, 12)]:
        assert lib.fvit_layernorm2d_crop_cl(_lib.FVIT_F16, x.data_ptr(), x.data_ptr(), w.data_ptr(), w.data_ptr(), ctypes.c_float(1e-6), 1, H, W, Hp, Wp,
                                            C, C, _stream()) != 0
        assert b"layernorm2d_crop" in lib.fvit_last_error()


# ---- eager deploy against the goldens ----------------------------------------------------------------------------------------------------
_DEPLOYED = {}   # (case, dtype) -> (model with the plan installed, input, features): computed once, read-only, shared by the tests below


def _deployed(name, dt=torch.float16):
    if (name, dt) not in _DEPLOYED:
        model, x = _case_model(name)
        model.switch_to_deploy(dt)
        with torch.no_grad():
            feats = model.forward_features(x)
        _DEPLOYED[(name, dt)] = (model, x, tuple(f.clone() for f in feats))
    return _DEPLOYED[(name, dt)]


@pytest.mark.parametrize("name,dt", [(n, torch.float16) for n in sorted(BACKBONE_CASES)] + [("bb_tiny_odd", torch.bfloat16)])
def test_eager_deploy_matches_reference(name, dt):
    case = BACKBONE_CASES[name]
    _, _, feats = _deployed(name, dt)
    gold = np.load(os.path.join(GOLDEN, f"backbone_{name}.npz"))
    assert len(feats) == len(case["kwargs"]["out_indices"])
    errs = []
    for k, f in enumerate(feats):
        ref = torch.from_numpy(gold[f"out{k}"])
        assert f.dtype == torch.float32 and f.is_contiguous() and f.shape == ref.shape
        errs.append(_rel(f, ref))
    print(f"deploy {name} {dt}: per-level max|d|/max|ref| " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < BOUND[dt], errs


@pytest.mark.parametrize("name", ["bb_tiny_odd", "bb_tiny_exact"])
def test_forward_nested_in_deploy(name):
    case = BACKBONE_CASES[name]
    model, x, feats = _deployed(name)
    mask = make_mask(case["mask"], BATCH, *case["hw"]).to(DEV)
    gold = np.load(os.path.join(GOLDEN, f"backbone_{name}.npz"))
    with torch.no_grad():
        out = model(_Nested(x, mask))
    assert sorted(out) == list(range(len(case["kwargs"]["out_indices"])))
    for k, nt in out.items():
        assert isinstance(nt, _Nested) and torch.equal(nt.tensors, feats[k])
        assert torch.equal(nt.mask.cpu(), torch.from_numpy(gold[f"mask{k}"]))     # the masks module mode returns (test_gpu_backbone.py)


# ---- the runner --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bb_tiny_odd", "bb_tiny_exact"])
def test_runner_equals_eager_deploy(name):
    case = BACKBONE_CASES[name]
    model, x, feats = _deployed(name)
    runner = model.compile_inference(x)
    assert runner.graph is not None and runner.max_batch == BATCH
    first = tuple(o.clone() for o in runner(x))
    for a, b in zip(first, feats):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    for a, b in zip(runner(x), first):                     # a second replay
        assert torch.equal(a, b)
    one = runner(x[:1])                                    # a shorter batch is zero-padded; kernels may tile differently per batch: the plan's bar
    for a, b in zip(one, first):
        assert a.shape == (1,) + tuple(b.shape[1:])
        assert (a - b[:1]).abs().max().item() <= BOUND[torch.float16] * b.abs().max().item()
    mask = make_mask(case["mask"], BATCH, *case["hw"]).to(DEV)
    with torch.no_grad():
        want = model(_Nested(x, mask))
    got = runner.forward(_Nested(x, mask))
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k].tensors, want[k].tensors) and torch.equal(got[k].mask, want[k].mask)
    if name == "bb_tiny_odd":
        with pytest.raises(RuntimeError, match=r"\(2, 3, 224, 224\).*\(2, 3, 200, 328\)"):
            runner(torch.zeros(2, 3, 224, 224, device=DEV))


def test_runner_survives_eviction_of_its_geometry():
    """Eager calls at other sizes push the runner's geometry out of hat_runtime's LRU (DYN_CACHE_SIZE = 8): first the nine sizes {112, 224, 336}^2 --
    nine other stage workspaces, so the runner's (a 13 x 21 stage-2 map) is dropped; one of them shares its padded 14 x 21 window grid -- then five more
    grids, which drop the packed weights and tables of 14 x 21 too.  After each round the captured graph must still address live memory (the runner
    pins what it captured) and return the same bits."""
    model, x = _case_model("bb_tiny_odd")
    model.switch_to_deploy()
    runner = model.compile_inference(x)
    want = tuple(o.clone() for o in runner(x))
    st = hat_runtime._state(model.levels[2], torch.device(DEV))
    mine = (BATCH, 14, 21, 13, 21)
    assert (14, 21) in st.packs and (14, 21) in st.tables and any(k[:5] == mine for k in st.workspaces) and hat_runtime.DYN_CACHE_SIZE == 8

    def sweep(sizes):
        with torch.no_grad():
            for H, W in sizes:
                model.forward_features(synth_input(BATCH, H, W, SEED + H + W).to(DEV))
        filler = [torch.full((1 << 20,), float("nan"), device=DEV) for _ in range(8)]    # whatever was freed is likely reused by now
        got = runner(x)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        del filler

    sweep([(H, W) for H in (112, 224, 336) for W in (112, 224, 336)])
    assert not any(k[:5] == mine for k in st.workspaces)                              # the runner's workspace left the cache ...
    sweep([(448, 112), (448, 224), (448, 336), (448, 448), (112, 448)])
    assert (14, 21) not in st.packs and (14, 21) not in st.tables                     # ... and now its packed weights and tables
    with torch.no_grad():                                   # an eager call at the runner's geometry builds its own state; the runner keeps its
        eager = model.forward_features(x)
    for a, b, c in zip(eager, want, runner(x)):
        assert torch.equal(a, b) and torch.equal(c, b)


def test_weight_update_is_picked_up_eagerly_and_by_recompile():
    case = BACKBONE_CASES["bb_tiny_odd"]
    model, sd = _model(case["name"], case["kwargs"], case["family"])
    x = synth_input(BATCH, *case["hw"], SEED).to(DEV)
    model.switch_to_deploy()
    runner = model.compile_inference(x)
    before = tuple(o.clone() for o in runner(x))
    with torch.no_grad():
        model.levels[0].blocks[0].conv1.weight.mul_(1.5)
        model.norm1.running_mean.add_(0.25)
    sd2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fresh, _ = _model(case["name"], case["kwargs"], case["family"], sd=sd2)
    fresh.switch_to_deploy()
    with torch.no_grad():
        want = fresh.forward_features(x)
        got = model.forward_features(x)
    for a, b, c in zip(got, want, before):
        assert torch.equal(a, b) and not torch.equal(a, c)
    for a, c in zip(runner(x), before):                     # the graph still holds the old packed copies
        assert torch.equal(a, c)
    runner.recompile()
    for a, b in zip(runner(x), want):
        assert torch.equal(a, b)


# ---- nothing else changes ------------------------------------------------------------------------------------------------------------------
def test_grad_train_and_module_paths_unchanged_by_the_plan():
    case = BACKBONE_CASES["bb_tiny_odd"]
    x = synth_input(BATCH, *case["hw"], SEED).to(DEV)
    res = {}
    for deploy in (False, True):
        m, _ = _model(case["name"], case["kwargs"], case["family"])
        m.requires_grad_(True).enable_hat_backward()
        if deploy:
            m.switch_to_deploy()
        outs = m.forward_features(x)                        # eval, grad enabled: the autograd path
        sum(o.square().mean() for o in outs).backward()
        g_eval = m.levels[0].blocks[0].conv1.weight.grad.clone()
        m.zero_grad()
        m.train()
        torch.manual_seed(11)
        outs_t = m.forward_features(x)
        sum(o.square().mean() for o in outs_t).backward()
        g_train = m.levels[2].blocks[0].mlp.fc1.weight.grad.clone()
        m.eval()
        if deploy:
            with torch.no_grad():
                assert not torch.equal(m.forward_features(x)[0], outs[0].detach())    # under no_grad the plan IS used (16-bit conv side)
            m.switch_to_deploy(None)
        with torch.no_grad():
            plain = m.forward_features(x)
        res[deploy] = ([o.detach() for o in outs], [o.detach() for o in outs_t], g_eval, g_train, plain)
    a, b = res[False], res[True]
    for i in (0, 1, 4):
        for u, v in zip(a[i], b[i]):
            assert torch.equal(u, v), i
    for r in (a, b):                                        # the gradients exist
        assert torch.isfinite(r[2]).all() and torch.isfinite(r[3]).all() and r[2].abs().max().item() > 0 and r[3].abs().max().item() > 0
