"""The yardsticks of tests/test_gpu_detection.py, checked without a GPU (tests/detection_refs.py):

* the float64 restatements equal what the reference's own PostProcess, box_ops and HungarianMatcher computed (tests/golden/detection_cases.npz) to float64
  rounding, and their fp32 boxes bit for bit;
* ordinary fp32 evaluations stay well inside the bar the kernels are held to;
* the conditions that make the reference's answer unique hold on every case (distinct top sigmoids; no IoU within 1e-5 of the NMS threshold);
* every wrong variant -- >= instead of >, +1-pixel areas, the 1e-6 dropped or added in the wrong op, ties to the higher index, suppression by
  already-suppressed boxes, class ids ignored, (h, w) swapped, gamma = 1 -- fails at least one case;
* the ABI declarations and the Python module exist, and every refusal that needs no device is raised.
"""
import ctypes
import os
import re

import pytest
import torch

from fastervit_amd import _lib
from tests import detection_refs as R

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fvit_det_select", "fvit_box_nms", "fvit_box_nms_workspace", "fvit_box_pairwise", "fvit_det_matcher_cost")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _close64(a, b, what):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, what
    tol = 1e-12 * max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= tol, f"{what}: {(a - b).abs().max().item():.3e} > {tol:.1e}"


def _checksum(golden, key, *tensors):
    want = golden[key]
    got = torch.tensor([t.double().sum().item() for t in tensors], dtype=F64)
    assert torch.allclose(got[:len(want)], want, rtol=1e-12, atol=1e-12), f"{key}: the random generator no longer produces the inputs the golden file was recorded on"


@pytest.mark.parametrize("case,raw,test", R.SELECT_RUNS, ids=[R.run_name(*r) for r in R.SELECT_RUNS])
def test_select_restatement_equals_the_reference_postprocess(golden, case, raw, test):
    logits, boxes, sizes, K = R.select_inputs(case)
    name = R.run_name(case, raw, test)
    _checksum(golden, f"{name}_checksum", logits, boxes)
    assert R.select_condition(logits, K), "the fp32 sigmoids of the top K + 1 candidates are not pairwise distinct"
    s64, l64, q64, b64 = R.select(logits, boxes, sizes, K, F64, raw, test)
    _close64(s64, golden[f"{name}_scores"], "scores")
    assert torch.equal(l64, golden[f"{name}_labels"])
    _close64(b64, golden[f"{name}_boxes"], "boxes")
    s32, l32, q32, b32 = R.select(logits, boxes, sizes, K, F32, raw, test)
    assert torch.equal(l32, l64) and torch.equal(q32, q64)
    assert b32.dtype == F32 and torch.equal(b32, golden[f"{name}_boxes32"]), "fp32 boxes differ from the reference's fp32 boxes"
    assert R.worst_ratio(s32, s64, s32, F32) <= 0.5
    # wrong answers
    if not raw:
        b_sw = R.select(logits, boxes, sizes, K, F32, raw, test, swap_hw=True)[3]
        assert not torch.equal(b_sw, golden[f"{name}_boxes32"]), "(h, w) swapped went unnoticed"


@pytest.mark.parametrize("name", R.SELECT_EXACT)
def test_select_tie_and_special_value_cases(name):
    logits, boxes, sizes, K = R.select_exact_inputs(name)
    B, Q, C = logits.shape
    s, l, q, b = R.select(logits, boxes, sizes, K, F64)
    idx = q * C + l
    flat = logits.reshape(B, -1)
    for i in range(B):      # descending, and among equal values ascending flat index; NaN in front
        v = flat[i][idx[i]]
        nan = torch.isnan(v)
        assert not nan[int(nan.sum()):].any()
        vv, ii = v[~nan], idx[i][~nan]
        assert ((vv[:-1] > vv[1:]) | ((vv[:-1] == vv[1:]) & (ii[:-1] < ii[1:]))).all()
        assert (idx[i][nan][:-1] < idx[i][nan][1:]).all()
        rest = torch.ones(Q * C, dtype=torch.bool)
        rest[idx[i]] = False
        if rest.any() and not nan.all():
            assert (flat[i][rest] <= vv.min()).all()
    if name.startswith("all_equal"):
        assert torch.equal(idx, torch.arange(K).expand(B, K))
    if name in ("four_values", "all_equal_small", "all_equal_large"):
        hi = R.select(logits, boxes, sizes, K, F64, ties_high=True)
        assert not torch.equal(hi[2] * C + hi[1], idx), "ties to the higher index went unnoticed"


def test_nms_value_cases_meet_their_condition_and_fp32_agrees():
    for N in R.NMS_N:
        for G in R.NMS_G:
            for with_idxs, with_order in ((False, False), (True, True)):
                boxes, order, idxs, _ = R.nms_inputs(N, G, with_idxs, with_order)
                assert R.nms_condition(boxes, R.NMS_THR)
                k64, c64 = R.nms_groups(boxes, order, R.NMS_THR, F64, idxs)
                k32, c32 = R.nms_groups(boxes, order, R.NMS_THR, F32, idxs)
                assert torch.equal(k64, k32) and torch.equal(c64, c32), (N, G)


def test_nms_wrong_variants_fail():
    boxes, order, idxs, _ = R.nms_inputs(300, 1, True, True)
    right = R.nms_groups(boxes, order, R.NMS_THR, F64, idxs)[0]
    assert 1 < (right[0] >= 0).sum() < 300
    for kw in (dict(plus1=True), dict(chain=True), dict(ignore_idxs=True)):
        assert not torch.equal(R.nms_groups(boxes, order, R.NMS_THR, F64, idxs, **kw)[0], right), kw
    b, want, thr = R.nms_exact_inputs("iou_exactly_thr")
    ident = torch.arange(b.shape[0])
    assert R.nms_rule(b, ident, thr, F64).tolist() == want
    assert R.nms_rule(b, ident, thr, F64, ge=True).tolist() != want
    assert R.nms_rule(b, ident, thr, F64, plus1=True).tolist() != want
    b, want, thr = R.nms_exact_inputs("chain")
    assert R.nms_rule(b, torch.arange(b.shape[0]), thr, F64, chain=True).tolist() != want


@pytest.mark.parametrize("name", R.NMS_EXACT)
def test_nms_exact_cases(name):
    b, want, thr = R.nms_exact_inputs(name)
    for dt in (F64, F32):
        assert R.nms_rule(b, torch.arange(b.shape[0]), thr, dt).tolist() == want


def test_postprocess_with_nms_equals_the_reference(golden):
    logits, boxes, sizes, K = R.select_inputs(R.PP_NMS_CASE)
    s, l, q, b = R.select(logits, boxes, sizes, K, F64)
    assert R.nms_condition(b.to(F32), R.PP_NMS_THR) and R.nms_condition(b, R.PP_NMS_THR)
    keep, count = R.nms_groups(b, None, R.PP_NMS_THR, F64)
    assert torch.equal(count.long(), golden["ppnms_counts"]) and 0 < count.min() and count.max() < K
    rows = [k[:n] for k, n in zip(keep, count.tolist())]
    _close64(torch.cat([s[i][r] for i, r in enumerate(rows)]), golden["ppnms_scores"], "scores")
    assert torch.equal(torch.cat([l[i][r] for i, r in enumerate(rows)]), golden["ppnms_labels"])
    _close64(torch.cat([b[i][r] for i, r in enumerate(rows)]), golden["ppnms_boxes"], "boxes")


@pytest.mark.parametrize("case", range(len(R.PAIR_CASES)))
def test_pairwise_restatement_equals_box_ops(golden, case):
    b1, b2 = R.pair_inputs(case)
    _checksum(golden, f"pair{case}_checksum", b1, b2)
    iou, union = R.pair_iou(b1, b2, F64)
    giou = R.pair_giou(b1, b2, F64)
    _close64(iou, golden[f"pair{case}_iou"], "iou")
    _close64(union, golden[f"pair{case}_union"], "union")
    _close64(giou, golden[f"pair{case}_giou"], "giou")
    iou32, union32 = R.pair_iou(b1, b2, F32)
    giou32 = R.pair_giou(b1, b2, F32)
    for got, ex in ((iou32, iou), (union32, union), (giou32, giou)):
        assert R.worst_ratio(got, ex, got, F32) <= 0.5
    if case != len(R.PAIR_CASES) - 1:
        return
    # the 1e-6 dropped, or added in the wrong op (on the case with thousands of pairs)
    assert R.worst_ratio(R.pair_iou(b1, b2, F32, eps_iou=0.0)[0], iou, iou32, F32) > 1.0
    assert R.worst_ratio(R.pair_iou(b1, b2, F32, eps_union=1e-6)[1], union, union32, F32) > 1.0
    assert R.worst_ratio(R.pair_giou(b1, b2, F32, eps_area=0.0), giou, giou32, F32) > 1.0
    assert R.worst_ratio(R.pair_giou(b1, b2, F32, eps_iou=0.0), giou, giou32, F32) > 1.0


@pytest.mark.parametrize("case", range(len(R.COST_CASES)))
def test_cost_restatement_equals_the_reference_matcher(golden, case):
    logits, pred, ids, tgt = R.cost_inputs(case)
    _checksum(golden, f"cost{case}_checksum", logits, torch.cat([pred.flatten(), tgt.flatten()]))
    c64 = R.matcher_cost(logits, pred, ids, tgt, F64, **R.COST_WEIGHTS)
    _close64(c64, golden[f"cost{case}_C"], "C")
    c32 = R.matcher_cost(logits, pred, ids, tgt, F32, **R.COST_WEIGHTS)
    assert R.worst_ratio(c32, c64, c32, F32) <= 0.5
    assert R.worst_ratio(R.matcher_cost(logits, pred, ids, tgt, F32, gamma=1.0, **R.COST_WEIGHTS), c64, c32, F32) > 1.0, "gamma = 1 went unnoticed"


def test_abi_declarations_and_python_module_exist():
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), f"{s} is not declared in include/fvit_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS
    assert "#define FVIT_BOX_IOU" in hdr and "#define FVIT_BOX_GIOU" in hdr and "#define FVIT_ABI_VERSION 10" in hdr
    assert "fvit_boxes.hip" in open(os.path.join(ROOT, "fastervit_amd", "csrc", "Makefile")).read()
    import fastervit_amd
    from fastervit_amd import detection_ops
    for name in ("box_cxcywh_to_xyxy", "box_xyxy_to_cxcywh", "box_iou", "generalized_box_iou", "nms", "batched_nms", "PostProcess", "postprocess_launch",
                 "HungarianMatcher"):
        assert getattr(fastervit_amd, name) is getattr(detection_ops, name)
    src = open(detection_ops.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|torchvision)", src, re.M), "the module imports oracle or torchvision"
    assert not re.search(r"^(from|import)\s+scipy", src, re.M), "scipy is imported at module level, not lazily"


def test_box_converters_are_the_reference_formulas():
    from fastervit_amd import detection_ops as D
    x = torch.rand(7, 4, dtype=F64)
    assert torch.equal(D.box_cxcywh_to_xyxy(x), R.cxcywh_to_xyxy(x))
    x0, y0, x1, y1 = x.unbind(-1)
    assert torch.equal(D.box_xyxy_to_cxcywh(x), torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1))


def test_python_refusals_that_need_no_device():
    from fastervit_amd import detection_ops as D
    b, s = torch.rand(4, 4), torch.rand(4)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.box_iou(b, b)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.generalized_box_iou(b, b)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.nms(b, s, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.batched_nms(b, s, torch.zeros(4, dtype=torch.int64), 0.5)
    out = {"pred_logits": torch.zeros(1, 3, 2), "pred_boxes": torch.zeros(1, 3, 4)}
    with pytest.raises(RuntimeError, match="HIP device"):
        D.PostProcess(num_select=2)(out, torch.ones(1, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        D.postprocess_launch(out["pred_logits"], out["pred_boxes"], torch.ones(1, 2), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        D.HungarianMatcher()(out, [{"labels": torch.zeros(1, dtype=torch.int64), "boxes": torch.rand(1, 4)}])
    with pytest.raises(AssertionError):
        D.HungarianMatcher(0, 0, 0)


def test_c_abi_refusals_are_raised_before_any_launch():
    """Every size limit is checked on the host before a pointer is used or a kernel launched: with made-up pointers and no device the calls return
    FVIT_EINVAL and name the limit."""
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.lib()
    p = 4096      # never dereferenced
    def select(B, Q, C, K, raw=0, test=0):
        return lib.fvit_det_select(p, p, p, p, p, p, p, B, Q, C, K, raw, test, None)
    for args, word in (((0, 4, 4, 1), b"B=0"), ((1, 4, 4, 0), b"K=0"), ((1, 4, 4, 17), b"K=17"), ((1, 600, 4, 1025), b"K=1025"),
                       ((1, 4096, 4096, 10), b"2^24"), ((1, 4, 4, 2, 1, 1), b"not_to_xyxy")):
        assert select(*args) == -1 and word in lib.fvit_last_error(), (args, lib.fvit_last_error())
    assert lib.fvit_box_nms(p, None, None, 0.5, p, p, p, 1 << 40, 1, 8193, None) == -1 and b"N=8193" in lib.fvit_last_error()
    assert lib.fvit_box_nms(p, None, None, 0.5, p, p, p, 1 << 40, 0, 5, None) == -1 and b"G=0" in lib.fvit_last_error()
    assert lib.fvit_box_nms(p, None, None, 0.5, p, p, p, 8, 1, 65, None) == -2 and b"workspace" in lib.fvit_last_error()
    assert lib.fvit_box_nms(p, None, None, 0.5, None, p, p, 1 << 40, 1, 5, None) == -1 and b"null" in lib.fvit_last_error()
    assert lib.fvit_box_nms(p, None, None, 0.5, p, p, p, 0, 1, 0, None) == 0      # N = 0: nothing to do, no launch
    assert lib.fvit_box_nms_workspace(1, 8193) == 0 and lib.fvit_box_nms_workspace(0, 5) == 0
    assert lib.fvit_box_nms_workspace(3, 65) == 3 * 65 * 2 * 8 and lib.fvit_box_nms_workspace(1, 64) == 64 * 8
    assert lib.fvit_box_pairwise(2, p, p, p, None, 3, 3, None) == -1 and b"mode 2" in lib.fvit_last_error()
    assert lib.fvit_box_pairwise(0, p, p, p, None, -1, 3, None) == -1 and b"N=-1" in lib.fvit_last_error()
    assert lib.fvit_box_pairwise(0, p + 4, p, p, None, 3, 3, None) == -1 and b"aligned" in lib.fvit_last_error()
    assert lib.fvit_box_pairwise(1, p, p, p, None, 0, 3, None) == 0
    assert lib.fvit_det_matcher_cost(p, p, p, p, p, 3, 0, 2, 1.0, 1.0, 1.0, 0.25, None) == -1 and b"C=0" in lib.fvit_last_error()
    assert lib.fvit_det_matcher_cost(p, p, None, p, p, 3, 2, 2, 1.0, 1.0, 1.0, 0.25, None) == -1 and b"null" in lib.fvit_last_error()
    assert lib.fvit_det_matcher_cost(p, p, p, p, p, 3, 2, 0, 1.0, 1.0, 1.0, 0.25, None) == 0
    shipped = ctypes.CDLL(os.path.join(_lib.CSRC_DIR, "libfvit_hip.so"))
    assert all(hasattr(shipped, s) for s in SYMBOLS)
