"""Multi-scale detection backbone (fastervit_amd.build_fastervit) without a GPU: the fp64 restatement against the reference goldens, the
state_dict layout and load report, the per-call geometry helpers, frozen_stages and the duck-typed forward contract."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fastervit_amd
from fastervit_amd import hat_runtime
from fastervit_amd.models.backbone import _BACKBONE_CFGS, BACKBONE_NAMES, FasterViTBackbone
from oracle import hat_reference as hr
from tests import backbone_reference as br
from tests.backbone_cases import BACKBONE_CASES, BATCH, SEED, make_mask
from tests.synth import synth_input, synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "backbone_keys.json")) as _f:
    KEYS = json.load(_f)


def _digest(sd):
    lines = sorted(f"{k}:{tuple(v.shape)}:{str(v.dtype).replace('torch.', '')}" for k, v in sd.items())
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines)


def case_cfg(case):
    cfg = dict(_BACKBONE_CFGS[case["name"]])
    cfg.update(case["kwargs"])
    return cfg


@pytest.mark.parametrize("name", sorted(BACKBONE_CASES))
def test_restatement_matches_reference_golden(name):
    case = BACKBONE_CASES[name]
    model = fastervit_amd.build_fastervit(case["name"], **case["kwargs"])
    sd = synth_state_dict(model.state_dict(), SEED, case["family"])
    H, W = case["hw"]
    x = synth_input(BATCH, H, W, SEED)
    cfg = case_cfg(case)
    got = br.backbone_forward(sd, x, cfg, cfg["out_indices"])
    gold = np.load(os.path.join(GOLDEN, f"backbone_{name}.npz"))
    assert len(got) == len(cfg["out_indices"])
    for k, g in enumerate(got):
        ref = torch.from_numpy(gold[f"out{k}"]).double()
        assert g.shape == ref.shape
        err = (g - ref).abs().max().item() / ref.abs().max().item()
        assert err < 1e-5, f"level {cfg['out_indices'][k]}: {err:.2e}"
        m = make_mask(case["mask"], BATCH, H, W)
        want = F.interpolate(m[None].float(), size=ref.shape[-2:]).to(torch.bool)[0]
        assert torch.equal(want, torch.from_numpy(gold[f"mask{k}"]))


@pytest.mark.parametrize("name", BACKBONE_NAMES)
def test_state_dict_layout_and_classifier_load_report(name):
    rec = KEYS[name]
    with torch.device("meta"):
        bb = fastervit_amd.build_fastervit(name, use_checkpoint=True)
        cls = fastervit_amd.create_model(name)
    assert bb.num_features == rec["num_features"]
    assert _digest(bb.state_dict()) == (rec["sha256"], rec["n"])
    res = bb.load_state_dict(cls.state_dict(), strict=False)
    assert sorted(res.missing_keys) == rec["missing"]
    assert sorted(res.unexpected_keys) == rec["unexpected"]


def test_builder_names_and_errors():
    assert set(BACKBONE_NAMES) == set(KEYS)
    with pytest.raises(ValueError):
        fastervit_amd.build_fastervit("faster_vit_5_224")
    with pytest.raises(NotImplementedError):
        fastervit_amd.build_fastervit("faster_vit_0_224", norm_layer=torch.nn.LayerNorm)
    m = fastervit_amd.build_fastervit("faster_vit_0_224", out_indices=(1, 2, 3))
    assert isinstance(m, FasterViTBackbone) and m.out_indices == (1, 2, 3)
    assert not hasattr(m, "norm0") and hasattr(m, "norm3")


@pytest.mark.parametrize("Hp,Wp,want", [
    (14, 14, (5, 5, 3, 3, 4, 4, 4, 4)),        # the build-time 2x2 grid
    (7, 14, (4, 5, 3, 3, 2, 4, 2, 4)),         # 1x2 windows: G = 8
    (56, 84, (11, 15, 3, 3, 16, 24, 16, 24)),  # 800 x 1333 input: 8x12 windows, G = 384
    (70, 70, (13, 13, 3, 3, 20, 20, 20, 20)),  # 1024 x 1024
])
def test_token_geometry(Hp, Wp, want):
    got = hat_runtime.token_geometry(Hp, Wp, 7, 2)
    assert got == want
    kh, kw, sh, sw, Ho, Wo, Hq, Wq = got
    y = F.avg_pool2d(torch.zeros(1, 1, Hp, Wp), (kh, kw), (sh, sw))
    assert y.shape[-2:] == (Ho, Wo)
    assert (kh, kw), (sh, sw) == br.pool_geometry(Hp, Wp, 7, 2)


def test_token_geometry_pads_to_ct_multiple():
    # window multiples pool to multiples of ct_size; 21 x 30 with ws 4, ct 3 pools to 15 x 22 -> padded 15 x 24
    assert hat_runtime.token_geometry(21, 30, 4, 3)[4:] == (15, 22, 15, 24)
    for Hp, Wp, ws, cw in [(10, 15, 5, 3), (8, 12, 4, 3), (21, 30, 4, 3)]:
        kh, kw, sh, sw, Ho, Wo, Hq, Wq = hat_runtime.token_geometry(Hp, Wp, ws, cw)
        assert Hq % cw == 0 and Wq % cw == 0 and 0 <= Hq - Ho < cw and 0 <= Wq - Wo < cw


@pytest.mark.parametrize("sr0,sr1", [(1, 1), (1, 2), (2, 3), (8, 12), (5, 2)])
def test_dynamic_grid_tables_follow_ct_dewindow(sr0, sr1):
    """The raster order of the carrier grid (hg, wg) = (2 sr0, 2 sr1): ct_src of the gather tables is DET's ct_dewindow(ct, hg, wg, 2)."""
    cw, ws = 2, 7
    tb = hat_runtime.build_tables(sr0, sr1, ws, cw, True)
    S, ncw, G = tb["S"], tb["ncw"], tb["G"]
    assert G == cw * cw * sr0 * sr1
    src = tb["ct_src"].long()
    p = (src // S) * ncw + src % S                             # windowed row feeding raster r
    ct = torch.arange(G, dtype=torch.float64).view(1, G, 1)
    want = hr.ct_dewindow(ct, cw * sr0, cw * sr1, cw).reshape(G).long()
    assert torch.equal(p, want)


def test_dynamic_geometry_only_for_backbone_layers():
    bb = fastervit_amd.build_fastervit("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4])
    assert hat_runtime._geometry(bb.levels[2], 56, 84)[2:] == (8, 12)
    cls = fastervit_amd.create_model("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4])
    assert hat_runtime._geometry(cls.levels[2], 14, 14)[2:] == (2, 2)
    with pytest.raises(ValueError, match="built for 2x2"):
        hat_runtime._geometry(cls.levels[2], 56, 84)


@pytest.mark.parametrize("h,w", [(7, 7), (2, 4), (4, 2), (16, 24)])
def test_grid_position_table(h, w):
    bb = fastervit_amd.build_fastervit("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4])
    sd = synth_state_dict(bb.state_dict(), SEED, "stress")
    bb.load_state_dict(sd)
    blk = bb.levels[2].blocks[0]
    got = hat_runtime.grid_pos_table(blk.hat_pos_embed, h, w).double()
    want = br.pos_grid(sd, "levels.2.blocks.0.hat_pos_embed.", h, w, torch.float64)[0]
    assert (got - want).abs().max().item() < 1e-5
    if h * w > 1:   # not the classifier's table (normalised by sqrt(tokens) // 2)
        assert (blk.pos_embed.table(49).double() - br.pos_grid(sd, "levels.2.blocks.0.pos_embed.", 7, 7, torch.float64)[0]).abs().max() > 1e-3


@pytest.mark.parametrize("G", [4, 8, 16, 24, 384])
def test_carrier_bias_padded_or_cropped(G):
    bb = fastervit_amd.build_fastervit("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4])
    sd = synth_state_dict(bb.state_dict(), SEED, "stress")
    bb.load_state_dict(sd)
    got = bb.levels[2].blocks[0].hat_attn.pos_emb_funct.table(G).double()
    want = hr.attn_bias(sd, "levels.2.blocks.0.hat_attn.pos_emb_funct.", 4, 2, G, torch.float64)
    assert got.shape == want.shape == (2, G, G)
    assert (got - want).abs().max().item() < 1e-5


def test_frozen_stages():
    for fs in (-1, 0, 1):
        m = fastervit_amd.build_fastervit("faster_vit_0_224", frozen_stages=fs, dim=16, in_dim=16, depths=[1, 1, 1, 1],
                                          num_heads=[1, 1, 2, 4])
        m.train()
        frozen = fs >= 0
        assert all(p.requires_grad != frozen for p in m.patch_embed.parameters())
        assert m.patch_embed.training != frozen
        assert all(p.requires_grad for p in m.levels.parameters())
        assert m.levels.training
    for fs in (2, 3):
        with pytest.raises(ValueError):
            fastervit_amd.build_fastervit("faster_vit_0_224", frozen_stages=fs)


class _Nested:
    """Stand-in for DINO's NestedTensor (util.misc is not imported by the product)."""

    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask


def test_forward_contract_through_stub(monkeypatch):
    m = fastervit_amd.build_fastervit("faster_vit_0_224", out_indices=(1, 2, 3)).eval()
    feats = (torch.randn(2, 128, 25, 42), torch.randn(2, 256, 13, 21), torch.randn(2, 512, 7, 11))
    seen = []
    monkeypatch.setattr(m, "forward_features", lambda x: (seen.append(x), feats)[1])
    x = torch.zeros(2, 3, 200, 333)
    mask = make_mask("pad", 2, 200, 333)
    out = m(_Nested(x, mask))
    assert seen[0] is x
    assert sorted(out) == [0, 1, 2]
    for k, f in enumerate(feats):
        assert type(out[k]) is _Nested
        assert out[k].tensors is f
        want = F.interpolate(mask[None].float(), size=f.shape[-2:]).to(torch.bool)[0]
        assert out[k].mask.dtype == torch.bool and torch.equal(out[k].mask, want)
    with pytest.raises(ValueError):
        m(_Nested(x, None))


def test_inference_only_guards():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 1, 1], num_heads=[1, 1, 2, 4])
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train().forward_features(x)
    m.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_features(x)                      # parameters require grad, grad mode on
    m.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_features(x.requires_grad_())
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        m.forward_features(torch.zeros(1, 3, 64, 64))   # no CPU fallback for the transformer stages


def test_operand_modes():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", dim=16, in_dim=16, depths=[1, 1, 1, 1], num_heads=[1, 1, 2, 4])
    for mode in hat_runtime.OPERAND_MODES:
        assert m.set_hat_operand_dtype(mode) is m
        assert all(blk.hat_operand_dtype == mode for blk in m.levels[2].blocks)
    with pytest.raises(ValueError):
        m.set_hat_operand_dtype("fp8")
