"""tests/criterion_refs.py against the reference's own SetCriterion (tests/golden/criterion_cases.npz), without a GPU: the float64 restatement equals the
golden, an ordinary fp32 evaluation sits at most at 1/8 of every bar, each wrong variant fails at least one case, the conditions that make the
reference's answer unique hold, and the C ABI declarations, the module and the refusals that need no device are there."""
import ctypes
import os
import re

import pytest
import torch

from fastervit_amd import _lib
from tests import criterion_refs as R

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fvit_det_label_loss_workspace", "fvit_det_label_loss", "fvit_det_label_loss_backward", "fvit_det_box_loss", "fvit_det_box_loss_backward")
CASES = range(len(R.FORWARD_CASES))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


_cache = {}


def _evaluated(case):
    """(outputs, targets, indices, exact terms, exact scalars, exact grads, plain32 terms, plain32 scalars, plain32 grads) of a forward case, once."""
    if case not in _cache:
        c = R.FORWARD_CASES[case]
        outputs, targets, indices = R.forward_inputs(case)
        weights = R.weight_dict(c["aux"], c["interm"])
        res = []
        for dt in (F64, F32):
            o = R.convert(outputs, lambda v: v.to(dt).requires_grad_(True))
            terms, scalars = R.criterion(o, targets, indices, dt)
            tot = R.total(terms, weights)
            leaves = [s[k] for _, s in R.pred_sets(o) for k in ("pred_logits", "pred_boxes")]
            grads = torch.autograd.grad(tot, leaves, allow_unused=True)
            grads = [g if g is not None else torch.zeros_like(l) for g, l in zip(grads, leaves)]
            res += [terms, scalars, grads]
        _cache[case] = (outputs, targets, indices, *res)
    return _cache[case]


def _golden_grads(golden, name, outputs):
    return [golden[f"{name}_grad_{s}_{k}"] for s, _ in R.pred_sets(outputs) for k in ("logits", "boxes")]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in R.FORWARD_CASES])
def test_exact_restatement_equals_the_reference(golden, case):
    name = R.FORWARD_CASES[case]["name"]
    outputs, targets, indices, terms, scalars, grads = _evaluated(case)[:6]
    assert torch.equal(torch.from_numpy(R.checksum(outputs, targets)), golden[f"{name}_checksum"]), "the generated inputs drifted"
    values = {k: v.sum() for k, v in terms.items()}
    values.update(scalars)
    assert sorted(values) == golden[f"{name}_keys"]
    for k, v in values.items():
        want = golden[f"{name}_loss_{k}"].item()
        tol = 1e-6 * abs(want) if k.startswith(("class_error", "cardinality_error")) else 1e-12 * max(abs(want), 1e-3)   # the reference's counts are fp32
        assert abs(v.item() - want) <= tol, (k, v.item(), want)
    for g, want in zip(grads, _golden_grads(golden, name, outputs)):
        assert (g - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1e-3)
    for s, ind in enumerate(indices):
        for b, (i, j) in enumerate(ind):
            assert torch.equal(i, golden[f"{name}_idx{s}_{b}_src"]) and torch.equal(j, golden[f"{name}_idx{s}_{b}_tgt"])


def test_focal_restatement_equals_the_reference_on_dense_targets(golden):
    for case in range(len(R.LABEL_CASES)):
        logits, classes, nb = R.label_inputs(case)
        B, Q, C = logits.shape
        want = golden[f"focal{case}"].item()
        got = R.label_ref(logits, classes, nb, F64)["terms"].sum().item() / Q      # the reference's function itself does not multiply by Q
        assert abs(got - want) <= 1e-12 * abs(want), (case, got, want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in R.FORWARD_CASES])
def test_plain32_is_within_an_eighth_of_every_bar(case):
    outputs, _, _, terms, scalars, grads, terms32, scalars32, grads32 = _evaluated(case)
    for k in terms:
        r = R.scalar_ratio(terms32[k].sum().item(), terms[k], terms32[k])
        assert r <= 0.125, (k, r)
    for k in scalars:
        assert abs(scalars32[k].item() - scalars[k].item()) <= 0.125 * R.COUNT_RTOL * abs(scalars[k].item()), k
    for g, g32 in zip(grads, grads32):
        assert R.worst_ratio(g32, g, g32, F32) <= 0.125
    for M in [m for m in R.BOX_M if m] + ["small"]:
        src, tgt = R.box_inputs(R.BOX_SMALL_M, small=True) if M == "small" else R.box_inputs(M)
        ex, p32 = R.box_ref(src, tgt, 3.0, F64), R.box_ref(src, tgt, 3.0, F32)
        for k in ex:
            assert R.scalar_ratio(p32[k].sum().item(), ex[k], p32[k]) <= 0.125, (M, k)


def test_the_focal_bar_is_what_the_design_counts_on():
    """About 3.5e-6 of the sum at (2, 900, 91); lane-strided and tree fp32 summation orders of the fp32 terms sit far below it."""
    logits, classes, nb = R.label_inputs(5)
    ex, p32 = R.label_ref(logits, classes, nb, F64)["terms"], R.label_ref(logits, classes, nb, F32)["terms"]
    bar = R.scalar_bar(ex, p32)
    assert 2.9e-6 <= bar / ex.sum().item() <= 1e-5
    flat = p32.reshape(-1)
    pad = torch.cat([flat, flat.new_zeros(-flat.numel() % 64)]).view(-1, 64)
    lanes = torch.zeros(64, dtype=F32)
    for row in pad:                      # 64 lanes, each adding its strided elements in sequence
        lanes = lanes + row
    while lanes.numel() > 1:             # then a tree
        lanes = lanes[0::2] + lanes[1::2]
    assert R.scalar_ratio(lanes.item(), ex, p32) <= 0.25


VARIANTS = [dict(swap_alpha=True), dict(gamma=1.0), dict(eps_iou=0.0), dict(eps_area=0.0), dict(swap_halves=True), dict(no_q=True), dict(no_num_boxes=True),
            dict(dn_plain_num_boxes=True), dict(card_class0=True), dict(noobj_last=True)]


def _worst_over_all_cases(golden, sw):
    worst = 0.0
    for case in CASES:
        name = R.FORWARD_CASES[case]["name"]
        outputs, targets, indices, terms, scalars, _, terms32 = _evaluated(case)[:7]
        wt, ws = R.criterion(R.convert(outputs, lambda v: v.double()), targets, indices, F64, **sw)
        for k in terms:
            worst = max(worst, R.scalar_ratio(wt[k].sum().item(), terms[k], terms32[k]))
        for k in scalars:
            want = golden[f"{name}_loss_{k}"].item()
            err = abs(ws[k].item() - want)
            worst = max(worst, 0.0 if err == 0 else err / (R.COUNT_RTOL * abs(want)) if want else float("inf"))
    src, tgt = R.box_inputs(R.BOX_SMALL_M, small=True)
    ex, p32 = R.box_ref(src, tgt, 3.0, F64), R.box_ref(src, tgt, 3.0, F32)
    wrong = R.box_ref(src, tgt, 3.0, F64, **{k: v for k, v in sw.items() if k in ("eps_iou", "eps_area", "swap_halves", "no_num_boxes")})
    for k in ex:
        worst = max(worst, R.scalar_ratio(wrong[k].sum().item(), ex[k], p32[k]))
    return worst


def test_the_right_answer_passes_its_own_bars(golden):
    assert _worst_over_all_cases(golden, {}) <= 1e-3


@pytest.mark.parametrize("sw", VARIANTS, ids=[next(iter(v)) for v in VARIANTS])
def test_each_wrong_variant_fails_at_least_one_case(golden, sw):
    assert _worst_over_all_cases(golden, sw) > 1.0


def test_wrong_focal_constants_are_far_above_the_bar():
    logits, classes, nb = R.label_inputs(5)
    ex, p32 = R.label_ref(logits, classes, nb, F64)["terms"], R.label_ref(logits, classes, nb, F32)["terms"]
    for sw in (dict(alpha=0.5), dict(swap_alpha=True), dict(gamma=1.0)):
        assert R.scalar_ratio(R.label_ref(logits, classes, nb, F64, **sw)["terms"].sum().item(), ex, p32) > 1e4, sw


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in R.FORWARD_CASES])
def test_the_reference_answer_is_unique(case):
    outputs, targets, indices = _evaluated(case)[:3]
    assert R.forward_condition(outputs, targets, indices)
    for o, ind in zip(R.matched_sets(outputs), indices):
        ex, p32 = R.cost_matrices(o, targets, F64), R.cost_matrices(o, targets, F32)
        for variant in (p32, [e + R.bound(e, p, F32) for e, p in zip(ex, p32)], [e - R.bound(e, p, F32) for e, p in zip(ex, p32)]):
            for (i, j), (i2, j2) in zip(ind, R.assign([v.double() for v in variant])):
                assert torch.equal(i, i2) and torch.equal(j, j2), "the assignment depends on fp32 rounding of the cost matrix"
    for c in range(len(R.LABEL_CASES)):
        assert R.unique_row_max(R.label_inputs(c)[0])
    for M in R.BOX_M:
        assert R.no_ties(*R.box_inputs(M))


def test_abi_declares_the_loss_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert "#define FVIT_DET_MAX_SETS 16" in hdr and _lib.FVIT_DET_MAX_SETS == 16 and "#define FVIT_ABI_VERSION 10" in hdr
    assert ctypes.sizeof(_lib.FvitDetLabelSet) == 4 * 8 + 4 * 4 and ctypes.sizeof(_lib.FvitDetBoxSet) == 3 * 8 + 2 * 4
    assert "fvit_loss.hip" in open(os.path.join(ROOT, "fastervit_amd", "csrc", "Makefile")).read()
    import fastervit_amd
    from fastervit_amd import criterion
    assert fastervit_amd.SetCriterion is criterion.SetCriterion and fastervit_amd.sigmoid_focal_loss is criterion.sigmoid_focal_loss


def test_abi_refusals_that_need_no_device(lib):
    """Every refusal comes before a launch: the pointers below are not device memory."""
    p = 0x7f0000001000
    L, Bx = _lib.FvitDetLabelSet, _lib.FvitDetBoxSet
    one = lambda **k: (L * 1)(L(**{**dict(logits=p, classes=p, targets=None, grad_logits=p, R=14, Q=7, B=2, scale=1.0), **k}))
    many = lambda n: (L * n)(*[L(logits=p, classes=p, targets=None, grad_logits=p, R=14, Q=7, B=2, scale=1.0) for _ in range(n)])
    fwd = lambda sets, n, C=5, stride=2, ws=p, nbytes=1 << 20, loss=p: lib.fvit_det_label_loss(sets, n, C, 0.25, 2.0, loss, p, stride, p, ws, nbytes, None)
    bwd = lambda sets, n, C=5, g=p: lib.fvit_det_label_loss_backward(sets, n, C, 0.25, 2.0, g, None)
    err = lambda: lib.fvit_last_error()
    assert fwd(many(1), 0) == -1 and b"n_sets=0" in err()
    assert fwd(many(17), 17) == -1 and b"n_sets=17" in err()
    assert bwd(many(17), 17) == -1 and b"n_sets=17" in err()
    assert lib.fvit_det_label_loss_workspace(many(17), 17, 5) == 0 and b"n_sets=17" in err()
    assert fwd(many(1), 1, C=0) == -1 and b"C=0" in err()
    assert fwd(one(R=1 << 27, Q=1 << 26), 1, C=16) == -1 and b"2^31" in err()
    assert bwd(one(R=1 << 27, Q=1 << 26), 1, C=16) == -1 and b"2^31" in err()
    assert fwd(one(R=15), 1) == -1 and b"R == B * Q" in err()
    assert fwd(one(logits=p + 2), 1) == -1 and b"misaligned" in err()
    assert fwd(one(classes=p + 1), 1) == -1 and b"misaligned" in err()
    assert fwd(one(classes=None), 1) == -1 and b"null" in err()
    assert bwd(one(grad_logits=None), 1) == -1 and b"null" in err()
    assert bwd(many(1), 1, g=None) == -1 and b"grad_loss" in err()
    assert fwd(many(1), 1, stride=1) == -1 and b"card_stride" in err()
    assert fwd(many(1), 1, ws=p + 8) == -1 and b"misaligned" in err()
    assert fwd(many(1), 1, loss=None) == -1 and b"null" in err()
    assert fwd(many(1), 1, nbytes=8) == -2 and b"workspace" in err()
    assert lib.fvit_det_label_loss_workspace(many(3), 3, 5) == 3 * 2 * 16      # one 16-byte partial per workgroup: 2 images x 1 chunk
    box = lambda n, **k: (Bx * n)(*[Bx(**{**dict(src=p, tgt=p, grad_src=p, M=3, scale=1.0), **k}) for _ in range(n)])
    assert lib.fvit_det_box_loss(box(1), 0, p, None) == -1 and b"n_sets=0" in err()
    assert lib.fvit_det_box_loss(box(17), 17, p, None) == -1 and b"n_sets=17" in err()
    assert lib.fvit_det_box_loss_backward(box(17), 17, p, None) == -1 and b"n_sets=17" in err()
    assert lib.fvit_det_box_loss(box(1, M=-1), 1, p, None) == -1 and b"M=-1" in err()
    assert lib.fvit_det_box_loss(box(1, src=p + 4), 1, p, None) == -1 and b"16-byte" in err()
    assert lib.fvit_det_box_loss(box(1, tgt=None), 1, p, None) == -1 and b"null" in err()
    assert lib.fvit_det_box_loss_backward(box(1, grad_src=None), 1, p, None) == -1 and b"null" in err()
    assert lib.fvit_det_box_loss(box(1), 1, None, None) == -1 and b"out" in err()
    assert lib.fvit_det_box_loss(box(2, M=0, src=None, tgt=None), 2, p, None) == 0      # no pair anywhere: no launch, nothing written


def test_python_refusals_that_need_no_device():
    from fastervit_amd import HungarianMatcher, SetCriterion, sigmoid_focal_loss
    x = torch.zeros(2, 7, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        sigmoid_focal_loss(x, x, 1.0)
    with pytest.raises(RuntimeError, match="float64"):
        sigmoid_focal_loss(x.double(), x.double(), 1.0)
    targets = [{"labels": torch.zeros(1, dtype=torch.int64), "boxes": torch.full((1, 4), 0.5)}] * 2
    outputs = {"pred_logits": x, "pred_boxes": torch.full((2, 7, 4), 0.5), "dn_meta": None}
    ind = [(torch.tensor([0]), torch.tensor([0]))] * 2
    crit = SetCriterion(5, HungarianMatcher(), {}, 0.25, ["labels", "boxes", "cardinality"])
    with pytest.raises(RuntimeError, match="HIP device"):
        crit(outputs, targets)
    for fn in (crit.loss_labels, crit.loss_boxes, crit.loss_cardinality):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(outputs, targets, ind, 2.0)
        with pytest.raises(RuntimeError, match="float64"):
            fn({k: v.double() if v is not None else v for k, v in outputs.items()}, targets, ind, 2.0)
    with pytest.raises(NotImplementedError, match="masks"):
        SetCriterion(5, HungarianMatcher(), {}, 0.25, ["labels", "masks"])(outputs, targets)
    with pytest.raises(NotImplementedError, match="masks"):
        crit.get_loss("masks", outputs, targets, ind, 2.0)
    with pytest.raises(AssertionError, match="do you really want"):
        crit.get_loss("dice", outputs, targets, ind, 2.0)
