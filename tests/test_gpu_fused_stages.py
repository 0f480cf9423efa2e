"""The fused HAT stage kernels (ctblk8 / attnblk / winblk / winmlp / mlp_fused) against the float64 oracle on every geometry users reach
with FasterViT-0 builds: non-square carrier grids (no hat_pos_embed, the ct_window scramble), padded windows, carrier grids beyond the
fused carrier kernel (G = 24, 216), layer scale + propagation, a hierarchical C = 512 stage, a qk_scale override, and the 16-bit and
two-term operand modes.

One stage at a time (``hat_runtime.stage_forward`` on ``model.levels[li]``), 'stress' weights (tests/synth.py), batch 2 with different
images, each run under three dispatch settings -- default, fused forced at small batch (row thresholds 0; "alt" also forces the opt-in
C = 256 forms winblk<256> and mlp_fused<256>), fused disabled -- with the launched kernel names recorded by the library's launch
profiler, so the dispatch each comparison covers is asserted, not assumed.  Bars are relative to max|oracle| (test_gpu_parity's
stage-map bar is 1e-3) at about twice the worst error measured on an MI355X; the measured numbers are next to BARS and in each docstring.
"""
import math

import pytest
import torch

from fastervit_amd import _lib, hat_runtime
from oracle import hat_reference as hr
from tests.cases import SEED
from tests.synth import synth_state_dict
from tests.util import build_product_model, load_golden, rel_err, tuned

pytestmark = pytest.mark.gpu

F, T = False, True

# dispatch settings (knob names are checked against the HIP sources by tests/test_tune_knobs.py)
FORCED = dict(attn_fused_min_rows=0, mlp_fused_min_rows=0)
FORCED_ALT = dict(attn_fused_min_rows=0, mlp_fused_min_rows=0, win_fused256=1, win_mlp256=0)
DISABLED = dict(attn_fused=0, mlp_fused=0, win_mlp256=0, win_fused=0, win_mlp=0, ct_fused=0)
SETTINGS = {"default": {}, "forced": FORCED, "alt": FORCED_ALT, "disabled": DISABLED}
FUSED_PREFIXES = ("ctblk", "attnblk", "winblk", "winmlp", "mlp_fused")

# geometry id -> (entry, kwargs, image size, levels, golden case, qk_scale for the oracle)
GEOMETRIES = {
    "anyres_112x224": ("faster_vit_0_any_res", dict(resolution=[112, 224]), (112, 224), (2, 3), "fvit0_anyres_112x224", None),
    "anyres_336x112": ("faster_vit_0_any_res", dict(resolution=[336, 112]), (336, 112), (2, 3), None, None),
    "anyres_160x160_ls_prop": ("faster_vit_0_any_res", dict(resolution=[160, 160], layer_scale=1e-5, do_propagation=True), (160, 160), (2, 3),
                               "fvit0_anyres_160x160", None),
    "anyres_200x312": ("faster_vit_0_any_res", dict(resolution=[200, 312]), (200, 312), (2, 3), None, None),
    "anyres_576x960": ("faster_vit_0_any_res", dict(), (576, 960), (2, 3), None, None),
    "fvit0_224_ls_prop": ("faster_vit_0_224", dict(layer_scale=1e-5, do_propagation=True), (224, 224), (2, 3), None, None),
    "fvit0_448_hat3": ("faster_vit_0_224", dict(hat=[F, F, T, T], resolution=448), (448, 448), (3,), None, None),
    "fvit0_224_qk": ("faster_vit_0_224", dict(qk_scale=0.31), (224, 224), (2, 3), None, 0.31),
}
ALL_MODES = ("f16", "bf16", "f16x2", "bf16x2", "f16x3")
MODES = {g: ("f16",) for g in GEOMETRIES}
MODES.update({g: ALL_MODES for g in ("anyres_112x224", "anyres_160x160_ls_prop", "fvit0_224_ls_prop")})

# per operand mode: (bar vs the fp64 oracle, bar for forced-fused vs disabled), both relative to max(|oracle|, 1).  Worst measured on an
# MI355X over every geometry / stage / setting / image (oracle; forced vs disabled):
#   f16 7.1e-4; 4.6e-4   f16x2 4.0e-4; 3.8e-4   bf16 5.9e-3; 3.0e-3   bf16x2 3.3e-3; 3.0e-3   f16x3 1.4e-6; -
# f16 stays at test_gpu_parity's 1e-3 stage-map bar (1.4x margin).  The bf16 modes round every ACTIVATION to 8 mantissa bits (2^-9 = 2e-3 per
# rounding; the second weight term of bf16x2 removes only the weight rounding), so their stage maps cannot meet 1e-3: their bars are 2x measured.
# Forced vs disabled: with 'stress' weights the fused and unfused chains round their 16-bit intermediates at different points, and each is
# ~5e-4 from the oracle, so they differ by up to 4.6e-4 (test_gpu_determinism's 2e-4 is for init weights, whose sub-block outputs are small).
BARS = {"f16": (1e-3, 9e-4), "f16x2": (8e-4, 8e-4), "bf16": (1.2e-2, 6e-3), "bf16x2": (7e-3, 6e-3), "f16x3": (3e-6, None)}


def _stage_hw(hw, li):
    """Spatial size of level ``li``'s input: the stem halves twice, every Downsample once (3x3 stride-2 convs, padding 1: ceil)."""
    h, w = hw
    for _ in range(2 + li):
        h, w = -(-h // 2), -(-w // 2)
    return h, w


def _kind(layer):
    """Which fused kernels the dispatch can reach on this stage."""
    b0 = layer.blocks[0]
    C = b0.attn.qkv.in_features
    if C == 512:
        return "512"
    assert C == 256 and b0.attn.num_heads == 8
    if not b0.do_sr_hat:
        return "256-local"
    G = b0.sr_ratio[0] * b0.sr_ratio[1] * b0.cr_window ** 2
    return "256-ct" if G <= 16 else "256-bigG"


def expected_fused(kind, setting, terms):
    """The fused kernel names fvit_api.hip's stage dispatch launches at batch 2 (rows far below attn_fused_min_rows / mlp_fused_min_rows)."""
    if terms == 3 or setting == "disabled":
        return set()
    if kind == "512":                                              # winblk / winmlp: no row threshold at C = 512
        return {"winblk_kernel<512,S64>", "winmlp_kernel<512>"}
    out = {"ctblk8_kernel<256,G16>"} if kind == "256-ct" else set()   # the whole carrier branch for G <= 16, no row threshold
    if setting == "forced":
        out |= {"attnblk_kernel<256,S64>" if terms == 1 else "attnblk_kernel<256,S64,2 terms>", "winmlp_kernel<256>"}
    elif setting == "alt":
        out |= {"winblk_kernel<256,S64>", "mlp_fused_kernel<256>"}
    return out


def settings_for(terms):
    if terms == 3:
        return ("default", "forced")
    if terms == 2:
        return ("default", "forced", "disabled")   # (winblk<256> / mlp_fused take one weight term only)
    return ("default", "forced", "alt", "disabled")


def _build(entry, kwargs, golden):
    import fastervit_amd
    if golden is not None:
        model, sd = build_product_model(golden)
    else:
        model = fastervit_amd.create_model(entry, **kwargs).eval()
        sd = synth_state_dict(model.state_dict(), SEED, "stress")
        model.load_state_dict(sd, strict=True)
    return model


def _oracle(layer, x, qk_scale):
    b0 = layer.blocks[0]
    sd = {k: v.detach().double().cpu() for k, v in layer.state_dict().items()}
    return hr.hat_stage(x.double(), sd, "", depth=len(layer.blocks), heads=b0.attn.num_heads, ws=layer.window_size, cw=b0.cr_window,
                        input_resolution=list(x.shape[2:]), only_local=not b0.do_sr_hat, do_propagation=bool(b0.do_propagation),
                        any_res=layer.any_res, qk_scale=qk_scale)


def run_stage(layer, x, knobs):
    """stage_forward under ``knobs``; returns (float output on the CPU, set of fused kernel names launched)."""
    with tuned(**knobs), torch.no_grad():
        _lib.prof_enable(True)
        try:
            y = hat_runtime.stage_forward(layer, x).float().cpu()
            names = {r["name"] for r in _lib.prof_records()}
        finally:
            _lib.prof_enable(False)
    return y, {n for n in names if n.startswith(FUSED_PREFIXES)}


def _stage_inputs(layer, hw, li, golden, seed):
    C = layer.blocks[0].attn.qkv.in_features
    H, W = _stage_hw(hw, li)
    x = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(seed))
    if golden is not None:
        g = load_golden(golden)
        x0 = torch.from_numpy(g[f"level{li}_in"])
        assert tuple(x0.shape[1:]) == (C, H, W)
        x[0] = x0[0]                                                # image 0: the reference's own stage input
        x[1] *= x0.std()
        return x, torch.from_numpy(g[f"level{li}_out"])
    return x, None


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_fused_stage_kernels_vs_fp64_oracle(geom):
    """Every geometry x operand mode x dispatch setting against hr.hat_stage in float64 on both images (and, for the golden geometries,
    image 0 against the reference's own stage output); the fused kernel set launched is the one the dispatch rules predict; forced-fused and
    disabled agree with each other.  Measured bars: BARS (f16 worst 7.1e-4 of max|oracle|, f16x3 1.4e-6)."""
    entry, kwargs, hw, levels, golden, qk_scale = GEOMETRIES[geom]
    model = _build(entry, kwargs, golden).cuda()
    failures, rows = [], []
    for li in levels:
        layer = model.levels[li]
        kind = _kind(layer)
        x, gold = _stage_inputs(layer, hw, li, golden, seed=100 + li)
        ref = _oracle(layer, x, qk_scale).float()
        scale = max(ref.abs().max().item(), 1.0)
        if gold is not None:
            assert rel_err(ref[:1], gold) < 1e-4, "fp64 oracle vs reference golden"   # pins the oracle on this grid (test_oracle_golden)
        for mode in MODES[geom]:
            model.set_hat_operand_dtype(mode)
            terms = hat_runtime._OP[mode][2]
            bar, bar_fd = BARS[mode]
            outs = {}
            for setting in settings_for(terms):
                y, fused = run_stage(layer, x.cuda(), SETTINGS[setting])
                outs[setting] = y
                want = expected_fused(kind, setting, terms)
                errs = [rel_err(y[i], ref[i]) for i in range(2)]
                eg = rel_err(y[:1], gold) if gold is not None else float("nan")
                rows.append(f"{geom} L{li} {mode:6s} {setting:8s} err {max(errs):.2e} (img0 {errs[0]:.2e} img1 {errs[1]:.2e}, golden {eg:.2e}) "
                            f"kernels {sorted(fused)}")
                if fused != want:
                    failures.append(f"{geom} L{li} {mode} {setting}: launched {sorted(fused)}, expected {sorted(want)}")
                if not all(math.isfinite(e) and e < bar for e in errs) or (gold is not None and not eg < bar):
                    failures.append(f"{geom} L{li} {mode} {setting}: oracle err {errs} golden {eg:.2e} > {bar:.1e}")
            if bar_fd is not None:
                d = (outs["forced"] - outs["disabled"]).abs().max().item() / scale
                rows.append(f"{geom} L{li} {mode:6s} forced vs disabled {d:.2e}")
                if not d < bar_fd:
                    failures.append(f"{geom} L{li} {mode}: forced vs disabled {d:.2e} > {bar_fd:.1e}")
        model.set_hat_operand_dtype("f16")
    print("\n".join(rows))
    assert not failures, "\n".join(failures)


def test_natural_row_threshold_flips_dispatch_at_batch_6():
    """Default faster_vit_0_any_res (576 x 960, stage 2: 36 x 60 padded to 42 x 63, 54 windows of 53 rows, G = 216 carrier tokens on the
    long-window attention kernel), no knobs: batch 5 = 14 310 window rows stays below attn_fused_min_rows / mlp_fused_min_rows (16 384),
    batch 6 = 17 172 rows takes attnblk<256> + winmlp<256>.  Both against the fp64 oracle on two images (the same two images in both):
    measured 5.0e-4 / 5.1e-4 of max|oracle|, asserted at the f16 bar (1e-3)."""
    model = _build("faster_vit_0_any_res", {}, None).cuda()
    layer = model.levels[2]
    x6 = torch.randn(6, 256, 36, 60, generator=torch.Generator().manual_seed(56))
    idx = [0, 4]
    ref = _oracle(layer, x6[idx], None).float()
    for B, want in ((5, set()), (6, {"attnblk_kernel<256,S64>", "winmlp_kernel<256>"})):
        y, fused = run_stage(layer, x6[:B].cuda(), {})
        errs = [rel_err(y[i], ref[k]) for k, i in enumerate(idx)]
        print(f"anyres_576x960 L2 batch {B}: kernels {sorted(fused)}, err {errs}")
        assert fused == want, f"batch {B}: {sorted(fused)}"
        assert all(e < BARS["f16"][0] for e in errs), f"batch {B}: {errs}"


@pytest.mark.parametrize("geom", ["anyres_160x160_ls_prop", "anyres_112x224"])
def test_block_api_last_block_vs_fp64_oracle(geom):
    """The block-level entry (HAT.forward -> fvit_hat_block_forward) on the last stage-2 block, where the propagation (x += gamma1 * upsampled
    carrier rows, AR:703-706) follows the fused carrier / window kernels: x and ct against hr.hat_block in float64, per dispatch setting.
    On the non-square grid the carrier rows themselves are compared, so a wrong ct_src / ln1_src row shows at full size (the stage output
    sees a swapped pair of carriers only through attention: 4.5e-4).  Measured: x 3.8e-4, ct 4.9e-4 of max|oracle| (f16 bar 1e-3)."""
    entry, kwargs, hw, _, golden, qk_scale = GEOMETRIES[geom]
    model = _build(entry, kwargs, golden).cuda()
    layer = model.levels[2]
    blk = layer.blocks[-1]
    assert blk.last and blk.do_sr_hat
    sr, ws, cw, C = tuple(blk.sr_ratio), blk.window_size, blk.cr_window, blk.attn.qkv.in_features
    g = torch.Generator().manual_seed(21)
    xw = torch.randn(2 * sr[0] * sr[1], ws * ws, C, generator=g)
    ct = torch.randn(2, sr[0] * sr[1] * cw * cw, C, generator=g)
    sd = {k[len(f"blocks.{len(layer.blocks) - 1}."):]: v.detach().double().cpu() for k, v in layer.state_dict().items()
          if k.startswith(f"blocks.{len(layer.blocks) - 1}.")}
    rx, rct = hr.hat_block(xw.double(), ct.double(), sd, "", heads=blk.attn.num_heads, ws=ws, cw=cw, sr=sr, last=True,
                           do_propagation=bool(blk.do_propagation), qk_scale=qk_scale)
    for setting in ("default", "forced", "disabled"):
        with tuned(**SETTINGS[setting]), torch.no_grad():
            yx, yct = blk(xw.cuda(), ct.cuda())
        ex, ect = rel_err(yx.float().cpu(), rx), rel_err(yct.float().cpu(), rct)
        print(f"{geom} block API, last block, {setting}: x {ex:.2e} ct {ect:.2e}")
        assert ex < BARS["f16"][0] and ect < BARS["f16"][0], f"{setting}: x {ex:.2e} ct {ect:.2e}"
