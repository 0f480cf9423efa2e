"""Deploy plan and graph runner of the detection backbone, the part that needs no GPU: the two new C symbols in the header, the binding and both
library builds; the public entry points and what they refuse by name."""
import ctypes
import os
import re

import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fvit_map_pad_cl", "fvit_layernorm2d_crop_cl")
_TINY = dict(depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)


@pytest.fixture(scope="module")
def built():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()


def _model(**kw):
    return fastervit_amd.build_fastervit("faster_vit_0_224", **dict(_TINY, **kw)).eval().requires_grad_(False)


def test_new_symbols_in_header_binding_and_both_builds(built):
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    assert re.search(r"#define FVIT_ABI_VERSION 10\b", hdr) and _lib.FVIT_ABI_VERSION == 10
    diag_at = hdr.index("#ifdef FVIT_DIAG")
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr[:diag_at]), s     # declared in the product section
        assert s in _lib.EXPORTED_SYMBOLS and s not in _lib.DIAG_SYMBOLS
    for so in ("libfvit_hip.so", "libfvit_hip_diag.so"):
        lib = ctypes.CDLL(os.path.join(_lib.CSRC_DIR, so))
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), (so, s)
        lib.fvit_abi_version.restype = ctypes.c_int
        assert lib.fvit_abi_version() == 10
    bound = _lib.lib()
    assert len(bound.fvit_map_pad_cl.argtypes) == 10 and len(bound.fvit_layernorm2d_crop_cl.argtypes) == 14


def test_new_kernels_refuse_bad_geometry_before_any_launch(built):
    """The argument checks run on the host in front of the launch: Hp < H, Wp < W and C % 8 return an error with a message (no GPU needed)."""
    lib = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    for H, W, Hp, Wp, C in [(8, 8, 7, 8, 64), (8, 8, 8, 7, 64), (8, 8, 8, 8, 12)]:
        assert lib.fvit_map_pad_cl(_lib.FVIT_F16, p, p, 1, H, W, Hp, Wp, C, None) != 0
        assert b"map_pad" in lib.fvit_last_error()
        assert lib.fvit_layernorm2d_crop_cl(_lib.FVIT_F16, p, p, p, p, 1e-6, 1, H, W, Hp, Wp, C, C, None) != 0
        assert b"layernorm2d_crop" in lib.fvit_last_error()
    assert lib.fvit_map_pad_cl(_lib.FVIT_F32, p, p, 1, 8, 8, 8, 8, 64, None) != 0 and b"dtype" in lib.fvit_last_error()


def test_public_interface_and_refusals():
    m = _model()
    assert callable(m.switch_to_deploy) and callable(m.compile_inference)
    assert m.switch_to_deploy() is m
    from fastervit_amd.conv_runtime import BackboneDeployPlan, DeployPlan
    plan = m.__dict__["_deploy_plan"]
    assert isinstance(plan, BackboneDeployPlan) and isinstance(plan, DeployPlan) and plan.dtype == torch.float16
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad(), pytest.raises(RuntimeError, match="deploy plan: the input must be on a HIP device"):
        m.forward_features(x)
    assert m.switch_to_deploy(torch.bfloat16).__dict__["_deploy_plan"].dtype == torch.bfloat16
    assert m.switch_to_deploy(None) is m and "_deploy_plan" not in m.__dict__
    with torch.no_grad(), pytest.raises(RuntimeError, match="runs only on a HIP device"):   # module mode again: the stage's own message
        m.forward_features(x)
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        m.switch_to_deploy(torch.float32)
    assert "_deploy_plan" not in m.__dict__


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_compile_inference_refuses_by_name(dtype):
    m = _model()
    x = torch.randn(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="precise=True is not implemented for the backbone"):
        m.compile_inference(x, dtype=dtype, precise=True)
    with pytest.raises(NotImplementedError, match="streams > 1"):
        m.compile_inference(x, dtype=dtype, streams=2)
    with pytest.raises(ValueError, match="float16 or torch.bfloat16"):
        m.compile_inference(x, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.compile_inference(x, dtype=dtype)


def test_plan_refuses_options_and_norm_without_statistics(monkeypatch):
    from fastervit_amd.conv_runtime import BackboneDeployPlan
    m = _model()
    plan = BackboneDeployPlan(m)
    for attr, val, msg in [("precise", True, "precise=True"), ("conv_weight_terms", 2, "two-term conv weights"),
                           ("down_weight_terms", 2, "two-term conv weights"), ("streams", 2, "streams > 1")]:
        old = getattr(plan, attr)
        setattr(plan, attr, val)
        with pytest.raises(NotImplementedError, match=msg):
            plan.forward(torch.randn(1, 3, 64, 64))
        setattr(plan, attr, old)
    monkeypatch.setenv("FVIT_PRECISE_DEPLOY", "1")
    with pytest.raises(NotImplementedError, match="precise=True"):
        m.switch_to_deploy()
    monkeypatch.delenv("FVIT_PRECISE_DEPLOY")
    m2 = _model(out_indices=(1, 3))
    m2.norm3 = torch.nn.BatchNorm2d(128, track_running_stats=False).eval()
    with pytest.raises(NotImplementedError, match="no running statistics"):
        m2.switch_to_deploy()
    assert "_deploy_plan" not in m2.__dict__


def test_signature_covers_the_output_norms():
    """The plan's weight signature changes with norm{i} (a buffer and a parameter) and with a conv weight, not with a HAT block's parameter."""
    from fastervit_amd.conv_runtime import BackboneDeployPlan
    m = _model(out_indices=(1, 2))
    plan = BackboneDeployPlan(m)
    s0 = plan._signature()
    with torch.no_grad():
        m.norm1.running_mean.add_(1.0)
    s1 = plan._signature()
    with torch.no_grad():
        m.norm2.weight.mul_(2.0)
    s2 = plan._signature()
    with torch.no_grad():
        m.levels[0].blocks[0].conv1.weight.mul_(2.0)
    s3 = plan._signature()
    with torch.no_grad():
        m.levels[2].blocks[0].mlp.fc1.weight.mul_(2.0)
    assert len({s0, s1, s2, s3}) == 4 and plan._signature() == s3
