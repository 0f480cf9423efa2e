"""The stage-boundary fusions of the HAT stage driver on an MI355X (fvit_tune "stage_entry_fused" / "stage_exit_fused", both default 1).

Entry: block 0's window attention kernel (attnblk<256> / winblk<512>) reads the level's 16-bit map itself, and the fused carrier kernel reads ct_init,
instead of the window_partition pass + carrier copy.  Each value is widened with (float), which is what the partition stored: the stage output is BITWISE
that of the same call with the knob at 0.

Exit: the last winmlp<256> of a level writes LayerNorm2d of the map the window_reverse would have written.  It normalises the same rounded values as
map_rows_ln_cl_kernel but adds them in another order, so the bar is that of tests/test_gpu_level_glue_fusion.py (imported from there, not restated):
every element within one unit in the last place of the map type + 1e-5 of the fp64 LayerNorm of the 16-bit map the plain reverse route writes; the
two-kernel results (reverse + LayerNorm2d in one pass, and map then fvit_layernorm2d_cl) are held to the same bound in the same test.

The fused routes are forced at these small row counts (attn_fused_min_rows = mlp_fused_min_rows = 0).  Level 2 at batch 3 has 3 x 4 x 53 = 636 rows = 9 full
64-row groups + 60 rows: groups straddle windows and images and the last group is partial."""
import pytest
import torch

import fastervit_amd
from fastervit_amd import _lib, hat_runtime
from tests.cases import SEED
from tests.synth import synth_state_dict
from tests.test_gpu_fused_stages import FUSED_PREFIXES, expected_fused
from tests.test_gpu_level_glue_fusion import _exact_ln, _ln_params, _two_kernel_ln, _within_one_unit
from tests.util import build_product_model, case_input, load_golden, max_abs, tuned

pytestmark = pytest.mark.gpu

FORCED = dict(attn_fused_min_rows=0, mlp_fused_min_rows=0)
OFF = dict(stage_entry_fused=0, stage_exit_fused=0)
DTYPES = [(torch.float16, "f16", 2.0 ** -10), (torch.bfloat16, "bf16", 2.0 ** -7)]
EPS = 1e-6


def _stress_model(entry, **kwargs):
    model = fastervit_amd.create_model(entry, **kwargs).eval()
    model.load_state_dict(synth_state_dict(model.state_dict(), SEED, "stress"), strict=True)
    return model.cuda()


@pytest.fixture(scope="module")
def fvit0():
    """faster_vit_0_224 with 'stress' weights: level 2 is 14 x 14 x 256 (8 heads, 7 x 7 windows, 2 x 2 carriers per window: S = 53, G = 16), level 3 is
    7 x 7 x 512 (16 heads, one window, no carriers); no layer scale, no propagation."""
    return _stress_model("faster_vit_0_224")


def _map(B, C, H, W, dt, seed):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
    return x.to(dt).cuda().contiguous(memory_format=torch.channels_last)


def _run(layer, x, knobs, out=None, ln2d=None):
    """stage_forward under ``knobs``: (output, launch records)."""
    with tuned(**knobs), torch.no_grad():
        _lib.prof_enable(True)
        try:
            y = hat_runtime.stage_forward(layer, x, out=out, ln2d=ln2d)
            torch.cuda.synchronize()
            recs = _lib.prof_records()
        finally:
            _lib.prof_enable(False)
    return y, recs


def _kinds(recs):
    return {r["kind"] for r in recs}


def _names(recs):
    return {r["name"] for r in recs}


def _fused(recs):
    return {n for n in _names(recs) if n.startswith(FUSED_PREFIXES)}


@pytest.fixture
def operand_mode(fvit0):
    def set_mode(mode):
        fvit0.set_hat_operand_dtype(mode)
    yield set_mode
    fvit0.set_hat_operand_dtype("f16")


@pytest.mark.parametrize("dt,mode,ulp", DTYPES)
def test_level2_entry_is_bitwise(fvit0, operand_mode, dt, mode, ulp):
    operand_mode(mode)
    layer = fvit0.levels[2]
    x = _map(3, 256, 14, 14, dt, 21)
    on, r_on = _run(layer, x, FORCED)
    off, r_off = _run(layer, x, dict(FORCED, stage_entry_fused=0))
    assert "window_partition" not in _kinds(r_on) and "ct_rows_kernel" not in _names(r_on)
    assert "window_partition" in _kinds(r_off) and "ct_rows_kernel" in _names(r_off)
    assert _fused(r_on) == _fused(r_off) == expected_fused("256-ct", "forced", 1)
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
    # the same behind the fused exit: identical rows in, identical map out
    lw, lb = _ln_params(256, torch.Generator().manual_seed(3))
    on2, _ = _run(layer, x, FORCED, out=torch.empty_like(x), ln2d=(lw, lb, EPS))
    off2, _ = _run(layer, x, dict(FORCED, stage_entry_fused=0), out=torch.empty_like(x), ln2d=(lw, lb, EPS))
    assert torch.equal(on2, off2)


@pytest.mark.parametrize("dt,mode,ulp", DTYPES)
@pytest.mark.parametrize("strided", [False, True])
def test_level2_exit_within_one_unit(fvit0, operand_mode, dt, mode, ulp, strided):
    operand_mode(mode)
    layer = fvit0.levels[2]
    C = 256
    x = _map(3, C, 14, 14, dt, 22)
    lw, lb = _ln_params(C, torch.Generator().manual_seed(4))

    def dest():
        if not strided:
            return torch.empty_like(x), None
        wide = torch.full((3, C + 64, 14, 14), 3.0, dtype=dt, device="cuda").contiguous(memory_format=torch.channels_last)
        return wide[:, :C], wide   # the first 256 channels of a 320-channel map

    plain, r_plain = _run(layer, x, FORCED)                                     # the existing route: plain reverse into a 16-bit map
    assert "window_reverse" in _kinds(r_plain)
    out, wide = dest()
    assert hat_runtime.ln2d_tail_supported(x, out)
    fused, r_fused = _run(layer, x, FORCED, out=out, ln2d=(lw, lb, EPS))
    assert "map_rows_ln_cl_kernel" not in _names(r_fused) and "window_reverse" not in _kinds(r_fused)
    assert _fused(r_fused) == expected_fused("256-ct", "forced", 1)
    out2, _ = dest()
    rev_ln, r_rev = _run(layer, x, dict(FORCED, stage_exit_fused=0), out=out2, ln2d=(lw, lb, EPS))   # reverse + LayerNorm2d in one pass
    assert "map_rows_ln_cl_kernel" in _names(r_rev)
    two = _two_kernel_ln(hat_runtime._DT[dt], plain.permute(0, 2, 3, 1).contiguous(), lw, lb, EPS)     # map, then fvit_layernorm2d_cl
    torch.cuda.synchronize()
    exact = _exact_ln(plain.permute(0, 2, 3, 1), lw, lb, EPS)
    _within_one_unit(fused.permute(0, 2, 3, 1), exact, ulp, f"winmlp + LayerNorm2d into the map ({mode}, strided={strided})")
    _within_one_unit(rev_ln.permute(0, 2, 3, 1), exact, ulp, "reverse + LayerNorm2d")
    _within_one_unit(two, exact, ulp, "reverse, then LayerNorm2d")
    if strided:
        assert (wide[:, C:] == 3.0).all()   # the pad channels are not touched
    out3, _ = dest()
    again, _ = _run(layer, x, FORCED, out=out3, ln2d=(lw, lb, EPS))
    assert torch.equal(again, fused)


@pytest.mark.parametrize("dt,mode,ulp", DTYPES)
def test_level3_entry_is_bitwise(fvit0, operand_mode, dt, mode, ulp):
    operand_mode(mode)
    layer = fvit0.levels[3]
    x = _map(3, 512, 7, 7, dt, 23)   # 147 rows, one window per image: the fused entry is only a change of the load type
    on, r_on = _run(layer, x, FORCED)
    off, r_off = _run(layer, x, dict(FORCED, stage_entry_fused=0))
    assert "window_partition" not in _kinds(r_on) and "window_partition" in _kinds(r_off)
    assert _fused(r_on) == _fused(r_off) == expected_fused("512", "forced", 1)
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
    again, _ = _run(layer, x, FORCED)
    assert torch.equal(again, on)


def _unaligned_view(B, C, H, W, dt, seed):
    """C channels at channel offset 1 of a (C + 2)-channel map: pixels start at odd multiples of 2 bytes."""
    wide = torch.zeros(B, C + 2, H, W, dtype=dt, device="cuda").contiguous(memory_format=torch.channels_last)
    wide[:, 1:C + 1] = _map(B, C, H, W, dt, seed)
    return wide[:, 1:C + 1]


FALLBACKS = ["ls_prop", "padded_anyres", "unaligned_map", "default_thresholds_batch2"]


@pytest.mark.parametrize("case", FALLBACKS)
def test_fallbacks_keep_the_passes_and_the_bits(fvit0, case):
    """Where a boundary is not eligible the window_partition and window_reverse passes run as before, and the output equals, bitwise, that of the same
    call with both knobs at 0."""
    dt = torch.float16
    ln = False
    knobs = FORCED
    if case == "ls_prop":          # layer scale + propagation (the fvit0_224_ls_prop geometry)
        layer = _stress_model("faster_vit_0_224", layer_scale=1e-5, do_propagation=True).levels[2]
        x, ln = _map(2, 256, 14, 14, dt, 31), True
    elif case == "padded_anyres":  # 112 x 224: level 3 is 4 x 7, padded to one 7 x 7 window
        layer = _stress_model("faster_vit_0_any_res", resolution=[112, 224]).levels[3]
        x = _map(2, 512, 4, 7, dt, 32)
    elif case == "unaligned_map":  # pixels that are not 8-byte aligned: the partition's scalar path reads them
        layer = fvit0.levels[2]
        x = _unaligned_view(2, 256, 14, 14, dt, 33)
        assert x.data_ptr() % 8 != 0
    else:                          # batch 2 without forcing: level 2 stays on the unfused chain
        layer = fvit0.levels[2]
        x, ln, knobs = _map(2, 256, 14, 14, dt, 34), True, {}
    lw, lb = _ln_params(x.shape[1], torch.Generator().manual_seed(5))

    def call(k):
        if ln:
            return _run(layer, x, k, out=torch.empty(x.shape, dtype=dt, device="cuda").contiguous(memory_format=torch.channels_last), ln2d=(lw, lb, EPS))
        return _run(layer, x, k)

    got, recs = call(knobs)
    ref, _ = call(dict(knobs, **OFF))
    assert {"window_partition", "window_reverse"} <= _kinds(recs), sorted(_kinds(recs))
    assert torch.isfinite(got.float()).all() and torch.equal(got, ref)


def test_routes_taken_with_both_parts_on(fvit0):
    lw, lb = _ln_params(256, torch.Generator().manual_seed(6))
    x2 = _map(3, 256, 14, 14, torch.float16, 41)
    _, recs = _run(fvit0.levels[2], x2, FORCED, out=torch.empty_like(x2), ln2d=(lw, lb, EPS))
    names = _names(recs)
    assert "window_partition" not in _kinds(recs) and "window_reverse" not in _kinds(recs)
    assert "ct_rows_kernel" not in names and "map_rows_ln_cl_kernel" not in names
    assert _fused(recs) == expected_fused("256-ct", "forced", 1)
    x3 = _map(3, 512, 7, 7, torch.float16, 42)
    _, recs = _run(fvit0.levels[3], x3, FORCED)
    assert "window_partition" not in _kinds(recs)
    assert _fused(recs) == expected_fused("512", "forced", 1)


def test_model_logits_with_and_without_the_boundary_fusions():
    """faster_vit_0_224, deploy fp16, batch 4, thresholds forced to 0: logits against the golden under 1e-3 with both knobs on and with both off; two runs
    with the knobs on bitwise equal; graph replay (compile_inference) equal to the eager result.  Without forcing, level 2 at batch 4 is below the row
    thresholds and map_rows_ln_cl_kernel still runs."""
    gold = torch.from_numpy(load_golden("fvit0_224")["logits"][:4])
    model, _ = build_product_model("fvit0_224", "cuda")
    x = case_input("fvit0_224")[:4].cuda()
    model.switch_to_deploy(torch.float16)
    with torch.no_grad():
        with tuned(**FORCED):
            model(x)   # packs the weights, sizes the workspaces
            _lib.prof_enable(True)
            try:
                on = model(x).float().cpu()
                recs = _lib.prof_records()
            finally:
                _lib.prof_enable(False)
            on2 = model(x).float().cpu()
            runner = model.compile_inference(x, dtype=torch.float16, streams=1)   # whole-batch launches, as the eager call above
            replay = runner(x).float().cpu()
            replay2 = runner(x).float().cpu()
        with tuned(**FORCED, **OFF):
            off = model(x).float().cpu()
        _lib.prof_enable(True)
        try:
            model(x)
            names_default = _names(_lib.prof_records())
        finally:
            _lib.prof_enable(False)
    names = _names(recs)
    assert "window_partition" not in _kinds(recs) and "ct_rows_kernel" not in names and "map_rows_ln_cl_kernel" not in names, sorted(names)
    assert {"attnblk_kernel<256,S64>", "winblk_kernel<512,S64>", "winmlp_kernel<256>", "ctblk8_kernel<256,G16>"} <= names
    e_on, e_off = max_abs(on, gold), max_abs(off, gold)
    print(f"logits max-abs vs reference: boundaries fused {e_on:.3e}, not fused {e_off:.3e}; fused vs not {max_abs(on, off):.3e}")
    assert e_on < 1e-3 and e_off < 1e-3
    assert torch.equal(on, on2)
    assert torch.equal(replay, on) and torch.equal(replay2, on)
    assert "map_rows_ln_cl_kernel" in names_default
