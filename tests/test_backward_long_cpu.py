"""The long-sequence training path (fvit_bwd_window_attention_long, ``enable_hat_backward(True, long_sequences=True)``): what can be checked without a GPU."""
import os
import re

import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, hat_backward
from tests.backward_long_util import gather_compact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(depths=[1, 1, 1, 1], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)


def test_default_flag_answers_exactly_as_before():
    big = fastervit_amd.create_model("faster_vit_4_21k_384", **TINY).eval()      # one window of 576 / 144 tokens
    assert hat_backward.backward_unsupported_reason(big.levels[2]) == "windows of 576 tokens (the attention-core backward holds at most 64 in LDS)"
    assert hat_backward.backward_unsupported_reason(big.levels[3]) == "windows of 144 tokens (the attention-core backward holds at most 64 in LDS)"
    with pytest.raises(RuntimeError, match=r"enable_hat_backward: level 2 of this model has no kernel-sequence backward: windows of 576 tokens"):
        big.enable_hat_backward(True)
    assert not any(lvl.__dict__.get("hat_backward", False) or lvl.__dict__.get("hat_backward_long", False) for lvl in big.levels)
    wide = fastervit_amd.create_model("faster_vit_0_any_res", resolution=[448, 672]).eval()     # 28 x 42 map: 4 x 6 windows, 96 carrier tokens
    assert hat_backward.backward_unsupported_reason(wide.levels[2]) == "96 carrier tokens per image (at most 64)"


def test_long_sequences_flag_accepts_long_windows_and_still_refuses_the_rest():
    big = fastervit_amd.create_model("faster_vit_4_21k_384", **TINY).eval()
    assert big.enable_hat_backward(True, long_sequences=True) is big
    assert [bool(lvl.__dict__.get("hat_backward_long", False)) for lvl in big.levels] == [False, False, True, True]
    assert [bool(lvl.__dict__.get("hat_backward", False)) for lvl in big.levels] == [False, False, True, True]
    assert hat_backward.backward_unsupported_reason(big.levels[2]) is None and hat_backward.backward_unsupported_reason(big.levels[3], 12, 12) is None
    big.enable_hat_backward(False)
    assert not any(lvl.__dict__.get("hat_backward_long", False) for lvl in big.levels)
    assert hat_backward.backward_unsupported_reason(big.levels[2]) is not None
    wide = fastervit_amd.create_model("faster_vit_0_any_res", resolution=[448, 672]).eval().enable_hat_backward(True, long_sequences=True)
    assert hat_backward.backward_unsupported_reason(wide.levels[2], 28, 42) is None
    assert "does not pad into" in hat_backward.backward_unsupported_reason(wide.levels[2], 28, 28)
    # head_dim 128 > 96: refused with or without the option
    fat = fastervit_amd.create_model("faster_vit_4_21k_384", depths=[1, 1, 1, 1], num_heads=[1, 1, 1, 1], dim=32, in_dim=16).eval()
    with pytest.raises(RuntimeError, match="head_dim 128"):
        fat.enable_hat_backward(True, long_sequences=True)
    assert not any(lvl.__dict__.get("hat_backward_long", False) for lvl in fat.levels)
    # attn_drop above 64 tokens: refused in train mode only
    drop = fastervit_amd.create_model("faster_vit_4_21k_384", attn_drop_rate=0.1, **TINY).eval().enable_hat_backward(True, long_sequences=True)
    assert hat_backward.backward_unsupported_reason(drop.levels[2]) is None
    drop.train()
    assert "attn_drop = 0.1 in train mode on windows of 576 tokens" in hat_backward.backward_unsupported_reason(drop.levels[2])


def test_enable_twice_without_the_option_is_refused_again():
    big = fastervit_amd.create_model("faster_vit_4_21k_384", **TINY).eval().enable_hat_backward(True, long_sequences=True)
    with pytest.raises(RuntimeError, match="windows of 576 tokens"):
        big.enable_hat_backward(True)


def test_header_and_binding_declare_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    assert re.search(r"#define FVIT_ABI_VERSION 10\b", hdr) and _lib.FVIT_ABI_VERSION == 10
    for name in ("fvit_bwd_window_attention_long", "fvit_bwd_window_attention_long_workspace"):
        m = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S | re.M)   # the declaration, not the comment above it
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.EXPORTED_SYMBOLS
        if not os.path.isfile(_lib.LIB_PATH):
            _lib.build()
        fn = getattr(_lib.lib(), name)
        assert len(fn.argtypes) == nargs, (name, nargs, len(fn.argtypes))
    assert _lib.lib().fvit_abi_version() == 10
    # the short kernel keeps its contract: S > 64 is still its caller's error (no GPU needed: argument validation comes first)
    assert _lib.lib().fvit_bwd_window_attention(1, None, 0, None, 0, None, 0, 1.0, None, None, 1, 65, 8, 32, None) != 0
    assert _lib.lib().fvit_bwd_window_attention_long(1, None, 0, None, 0, None, 0, None, 0, 0, 1.0, None, None, None, 0, 1, 65, 8, 32, None) == -1
    assert _lib.lib().fvit_bwd_window_attention_long_workspace(3, 65, 8, 32, 0) == 2 * 3 * 8 * 128 * 4
    assert _lib.lib().fvit_bwd_window_attention_long_workspace(3, 576, 8, 32, 24) == (2 * 3 * 8 * 576 + 8 * 576 * 576) * 4


@pytest.mark.parametrize("entry,kwargs,level,which", [
    ("faster_vit_4_21k_384", TINY, 2, "attn"),                                                                                        # w = 24, ng = 0
    ("faster_vit_4_any_res", dict(TINY, window_size=[7, 7, 7, 7], ct_size=2, resolution=[672, 1120]), 2, "hat_attn"),                  # non-square carrier grid
    ("faster_vit_4_any_res", dict(TINY, window_size=[7, 7, 16, 8], ct_size=2, resolution=[256, 512]), 2, "attn"),                      # ng = 4 carrier tokens in front
])
def test_compact_table_restatement_equals_the_folded_table(entry, kwargs, level, which):
    """tests/backward_long_util.gather_compact (what the GPU test differentiates) of ``PosEmbMLPSwinv2D.rel_table()`` == ``PosEmbMLPSwinv2D.table(S)``."""
    torch.manual_seed(3)
    model = fastervit_amd.create_model(entry, **kwargs).eval()
    blk = model.levels[level].blocks[0]
    at = getattr(blk, which)
    ncw = blk.cr_window ** 2 if blk.do_sr_hat else 0
    S = blk.window_size ** 2 + ncw if which == "attn" else ncw * blk.sr_ratio[0] * blk.sr_ratio[1]
    rel, w = at.pos_emb_funct.rel_table()
    ng = S - w * w
    assert ng >= 0 and tuple(rel.shape) == (at.num_heads, (2 * w - 1) ** 2)
    dense = at.pos_emb_funct.table(S)
    assert torch.equal(gather_compact(rel, w, ng, S), dense)
    if ng:
        assert (dense[:, :ng] == 0).all() and (dense[:, :, :ng] == 0).all()
    # the host side differentiates the compact table: the autograd output hat_backward builds is that table, attached to cpb_mlp
    t, arg = hat_backward._bias_with_grad(at, S) if os.path.isfile(_lib.LIB_PATH) else (None, None)
    if t is not None and isinstance(arg, hat_backward.CompactBias):
        assert t.requires_grad and torch.equal(t.detach(), rel) and (arg.w, arg.ng) == (w, ng)
