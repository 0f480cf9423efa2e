"""Training the detection backbone (``FasterViTBackbone.enable_hat_backward``, fvit_token_init_dyn_backward, fvit_feature_tap_backward): what can be
checked without a GPU -- the C ABI of the two new entry points, the opt-in flag and its refusals, and that nothing falls back to the CPU."""
import ctypes
import os
import re

import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, hat_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(dim=16, in_dim=16, depths=[1, 1, 1, 1], num_heads=[1, 1, 2, 4])
NEW_SYMBOLS = ("fvit_token_init_dyn_backward", "fvit_feature_tap_backward")


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    assert re.search(r"#define FVIT_ABI_VERSION 10\b", hdr) and _lib.FVIT_ABI_VERSION == 10
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    assert lib.fvit_abi_version() == 10
    for name in NEW_SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S | re.M)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == nargs, (name, nargs)
        for so in ("libfvit_hip.so", "libfvit_hip_diag.so"):
            assert hasattr(ctypes.CDLL(os.path.join(_lib.CSRC_DIR, so)), name), (so, name)
    # argument validation comes before any launch: no GPU needed
    assert lib.fvit_token_init_dyn_backward(None, None, None, None, None, None, None, 1, 1, 7, 7, 1, 1, 1, 1, 2, None) != 0
    assert b"token_init_dyn_backward" in lib.fvit_last_error()
    assert lib.fvit_feature_tap_backward(None, None, None, 1, 1, 1, 1, 1, 1, None, None, 0, None, None) != 0
    assert b"feature_tap_backward" in lib.fvit_last_error()


def test_enable_returns_the_model_and_sets_the_level_flags():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", **TINY).eval()
    assert not any(lvl.__dict__.get("hat_backward", False) or lvl.__dict__.get("hat_backward_long", False) for lvl in m.levels)
    assert m.enable_hat_backward() is m
    assert m.__dict__["hat_backward"] is True
    assert [bool(lvl.__dict__.get("hat_backward", False)) for lvl in m.levels] == [False, False, True, True]
    assert [bool(lvl.__dict__.get("hat_backward_long", False)) for lvl in m.levels] == [False, False, True, True]   # no short-only mode: grids change per call
    assert m.enable_hat_backward(False) is m
    assert not any(lvl.__dict__.get("hat_backward", False) or lvl.__dict__.get("hat_backward_long", False) for lvl in m.levels)


def test_head_dim_above_96_is_refused_at_enable_time_by_name():
    fat = fastervit_amd.build_fastervit("faster_vit_0_224", dim=32, in_dim=16, depths=[1, 1, 1, 1], num_heads=[1, 1, 1, 1]).eval()   # stage 2: C = 128, one head
    with pytest.raises(RuntimeError, match=r"enable_hat_backward: level 2 .*head_dim 128"):
        fat.enable_hat_backward()
    assert not fat.__dict__.get("hat_backward", False)
    assert not any(lvl.__dict__.get("hat_backward", False) or lvl.__dict__.get("hat_backward_long", False) for lvl in fat.levels)


def test_dynamic_grid_reasons_depend_on_the_call_not_on_the_build_time_grid():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", attn_drop_rate=0.1, **TINY).eval().enable_hat_backward()
    lvl = m.levels[2]
    assert hat_backward.backward_unsupported_reason(lvl) is None
    assert hat_backward.backward_unsupported_reason(lvl, 13, 21) is None          # 2 x 3 windows: not the build-time 2 x 2 grid
    assert "16384 pixels" in hat_backward.backward_unsupported_reason(lvl, 130, 130)   # pads to 133 x 133 = 17 689 pixels
    lvl.train()
    assert hat_backward.backward_unsupported_reason(lvl, 14, 14) is None          # 53-token windows, 16 carrier tokens: the short kernels mask attn_drop
    assert "attn_drop = 0.1 in train mode on 96 carrier tokens" in hat_backward.backward_unsupported_reason(lvl, 28, 42)


def test_disabling_restores_the_inference_only_raises():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", **TINY).enable_hat_backward().enable_hat_backward(False)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train().forward_features(x)
    m.eval()
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_features(x)
    m.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_features(x.clone().requires_grad_())


def test_enabled_model_has_no_cpu_fallback():
    m = fastervit_amd.build_fastervit("faster_vit_0_224", **TINY).eval().enable_hat_backward()
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_features(torch.zeros(1, 3, 64, 64))                       # eval, parameters require grad
    with pytest.raises(RuntimeError, match="HIP device"):
        m.train().forward_features(torch.zeros(2, 3, 64, 64))
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        m.forward_features(torch.zeros(1, 3, 64, 64))
    x = torch.zeros(2, 4, 5, 6)
    with pytest.raises(RuntimeError, match="HIP device"):
        hat_backward.feature_tap_with_grad(x, torch.nn.BatchNorm2d(4).eval())
    with pytest.raises(RuntimeError, match="HIP device"):
        hat_backward.feature_tap_backward(x, x, torch.ones(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        hat_backward.token_init_dyn_backward(m.levels[2].global_tokenizer, torch.zeros(1, 64, 14, 14), torch.zeros(1, 16, 64), 7)
