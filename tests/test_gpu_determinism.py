"""Bitwise repeatability of the HIP path on an MI355X (VERDICT r01 "what's weak" #1d): the same HAT stage run twice on identical
input must give identical bits -- for the fused C = 256 / 512 kernels of FasterViT-0 AND for the unfused path of the other widths
(C = 320 / 640 with head_dim 40 -> dpad 64, C = 384 / 768, FasterViT-4's head_dim 49 with layer scale and propagation).  Only then is a
run-to-run difference of the whole model MIOpen's (module-mode fp32 convolutions), not ours.

Also: the order-staggered variants of the GEMM / fused kernels (fvit_tune knobs) are results-equivalent to the default order
within fp32 summation-order noise, and themselves repeatable.
"""
import pytest
import torch

from fastervit_amd import hat_runtime
from tests.util import tuned

pytestmark = pytest.mark.gpu


def _model(entry, **kw):
    import fastervit_amd
    torch.manual_seed(0)
    m = fastervit_amd.create_model(entry, **kw).eval().cuda()
    # 'stress'-like perturbation so that gamma / biases are not the trivial init values
    g = torch.Generator(device="cpu").manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(".bias") or "gamma" in n:
                p.add_(torch.randn(p.shape, generator=g).to(p.device) * 0.02)
    return m


@pytest.mark.parametrize("entry,batch", [("faster_vit_0_224", 5), ("faster_vit_1_224", 3), ("faster_vit_2_224", 3), ("faster_vit_4_224", 2)])
def test_hat_stages_are_bitwise_repeatable(entry, batch):
    model = _model(entry)
    g = torch.Generator(device="cpu").manual_seed(11)
    for li in (2, 3):
        lvl = model.levels[li]
        C = lvl.blocks[0].attn.qkv.in_features
        R = 14 if li == 2 else 7
        for dtype, fmt in ((torch.float32, torch.contiguous_format), (torch.float16, torch.channels_last)):
            x = torch.randn(batch, C, R, R, generator=g).cuda().to(dtype).contiguous(memory_format=fmt)
            outs = []
            for _ in range(3):
                outs.append(hat_runtime.stage_forward(lvl, x.clone()).clone())
            torch.cuda.synchronize()
            assert torch.isfinite(outs[0].float()).all()
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), f"{entry} level {li} {dtype}: repeat call differs"


def test_deploy_forward_is_bitwise_repeatable_across_graph_replays():
    """The whole deploy-mode forward (our conv kernels, no MIOpen) is bit-repeatable, eager and replayed from a hipGraph."""
    model = _model("faster_vit_0_224")
    x = torch.randn(12, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda()
    model.switch_to_deploy(torch.float16, streams=3)
    with torch.no_grad():
        a = model(x).clone()
        b = model(x).clone()
    assert torch.equal(a, b)
    runner = model.compile_inference(x)
    y1 = runner(x).clone()
    y2 = runner(x).clone()
    assert torch.equal(y1, y2)
    assert (y1.float() - a.float()).abs().max().item() < 2e-4


@pytest.mark.parametrize("streams,join_from", [(2, 3), (3, None)], ids=["timed-2shards-join3", "3shards-nojoin"])
def test_bench_configuration_is_bitwise_repeatable_across_calls(streams, join_from):
    """Batch 256 as concurrent stream shards -- the configuration bench.py times (2 shards joined in front of level 3) and the r03 form (3 shards,
    no join): every call / replay gives the same bits, eager and from the hipGraph, including the side-stream shards and the cross-stream join +
    torch.cat + whole-batch level 3.  r02 (profiles/r02_repeatability_hunt.log): single waves of the fused MLP kernel returned a wrong LayerNorm row
    mean (a ds_bpermute lane exchange issued while LDS-DMA was landing) when kernels of other shards shared the CU; whether it showed depended on
    the plan's streams (4 of 6 plans), so several plans are tried.  The lane reductions are VALU swaps since."""
    model = _model("faster_vit_0_224").to(memory_format=torch.channels_last)
    x = torch.randn(256, 3, 224, 224, generator=torch.Generator().manual_seed(1000)).cuda().contiguous(memory_format=torch.channels_last)
    first = None
    for graph in (False, True, False, True):
        runner = model.compile_inference(x, dtype=torch.float16, streams=streams, graph=graph, join_from=join_from)
        assert runner.plan.join_from == join_from
        outs = [runner(x).clone() for _ in range(6)]
        torch.cuda.synchronize()
        first = outs[0] if first is None else first
        for k, o in enumerate(outs):
            assert torch.equal(o, first), f"graph={graph}: call {k} differs from the first call (max {(o.float() - first.float()).abs().max().item():.3e})"
        del runner


def test_results_do_not_depend_on_leftover_registers_or_lds():
    """A poison kernel in front of every launch fills all 512 vector registers of every SIMD and all LDS with a pattern
    (fvit_debug_poison_launches): a kernel that reads a register or an LDS byte it never wrote would change its result with the
    pattern (on one stream such a read is repeatable and passes every other test).  The hook exists only in the DIAGNOSIS build of the
    library (libfvit_hip_diag.so: the same sources with -DFVIT_DIAG), so the check runs in a subprocess with FVIT_DIAG=1."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import torch
import fastervit_amd
from fastervit_amd import _lib
from fastervit_amd.conv_runtime import DeployPlan
assert _lib.DIAG and _lib.LIB_PATH.endswith("libfvit_hip_diag.so")
lib = _lib.lib()
sink = torch.zeros(16, dtype=torch.int32, device="cuda")
for entry, bs, precise in (("faster_vit_0_224", 86, False), ("faster_vit_1_224", 4, False), ("faster_vit_0_224", 8, True)):
    torch.manual_seed(0)
    model = fastervit_amd.create_model(entry).eval().cuda().to(memory_format=torch.channels_last)
    if precise:
        model.set_hat_operand_dtype("f16x3")
    x = torch.randn(bs, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda().contiguous(memory_format=torch.channels_last)
    plan = DeployPlan(model, torch.float16)
    plan.streams = 1
    plan.precise = precise
    with torch.no_grad():
        base = plan.forward(x).clone()
        try:
            for pattern in (0x7fc07fc0, 0x40004000, 0):
                lib.fvit_debug_poison_launches(sink.data_ptr(), pattern)
                y = plan.forward(x).clone()
                torch.cuda.synchronize()
                assert torch.isfinite(y).all() and torch.equal(y, base), f"{entry} precise={precise}: result depends on the register / LDS poison {pattern:#x}"
        finally:
            lib.fvit_debug_poison_launches(None, 0)
print("POISON-OK")
"""
    env = dict(os.environ, FVIT_DIAG="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert res.returncode == 0 and "POISON-OK" in res.stdout, res.stdout[-3000:]


# every knob set the sweep below runs (tests/test_tune_knobs.py checks each key against the tune_get calls of the HIP sources)
KNOB_SETS = [dict(gemm_stagger=1), dict(ab_stagger=1, mlp_stagger=1), dict(mlp_stagger=2), dict(ab_variant=2),
             dict(ab_variant=1),
             dict(attn_fused_min_rows=0, mlp_fused_min_rows=0), dict(ln_gemm=1), dict(ct_fused=0), dict(ct_variant=0), dict(ct_variant=1), dict(ct_variant=2), dict(ct_variant=0, ct_touch=1), dict(win_fused=0), dict(win_mlp=0), dict(win_mlp=0, win_fused=0, ln_gemm=1), dict(win_fused256=1), dict(win_mlp_pipe=0), dict(ct8_depth=2)]


@pytest.mark.parametrize("knobs", KNOB_SETS)
def test_order_stagger_knobs_keep_the_result(knobs):
    """Kernel-selection knobs (K / chunk / head order stagger, LDS ring depths, workgroup shapes, fused vs unfused carrier branch) only
    permute fp32 sums or change who computes what: same stage output within summation-order noise, still bit-repeatable."""
    model = _model("faster_vit_0_224")
    g = torch.Generator(device="cpu").manual_seed(5)
    for li, R, C in ((2, 14, 256), (3, 7, 512)):
        lvl = model.levels[li]
        x = torch.randn(96, C, R, R, generator=g).cuda()
        ref = hat_runtime.stage_forward(lvl, x).clone()
        with tuned(**knobs):
            a = hat_runtime.stage_forward(lvl, x).clone()
            b = hat_runtime.stage_forward(lvl, x).clone()
        assert torch.equal(a, b)
        err = (a - ref).abs().max().item()
        assert err < 2e-4 * max(ref.abs().max().item(), 1.0), f"level {li}: {err}"   # fp16 operands re-rounded after a different fp32 sum order
