"""tests/assignment_refs.py against scipy (tests/golden/assignment_cases.npz), without a GPU: the fp64 restatement of the device solver gives scipy's
indices on every case with one optimum and scipy's total on the tie cases, every unique-optimum case is separated from its runner-up by at least 1e-6, each
wrong variant fails at least one case, and the C ABI declarations, the refusals that need no device and the untouched scipy path are there."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fastervit_amd import _lib
from tests import assignment_refs as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIQUE = [n for n in A.case_names() if n not in A.TIE_CASES]


@pytest.fixture(scope="module")
def golden():
    return A.load_golden()


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _images(name):
    cost, sizes = A.draw(name)
    return list(enumerate(A.blocks(cost, sizes)))


def _fails(golden, name, **sw):
    """Does ``exact`` with these switches miss the golden of this case?"""
    for b, block in _images(name):
        src, tgt = A.exact(block, **sw)
        if not (np.array_equal(src, golden[f"{name}_{b}_src"]) and np.array_equal(tgt, golden[f"{name}_{b}_tgt"])):
            return True
    return False


@pytest.mark.parametrize("name", A.case_names())
def test_the_cost_matrices_are_the_ones_the_golden_was_made_from(golden, name):
    assert A.checksum(A.draw(name)[0]) == golden[f"{name}_sum"].item()


@pytest.mark.parametrize("name", UNIQUE)
def test_exact_equals_scipy_on_the_unique_optimum_cases(golden, name):
    assert not _fails(golden, name)
    for b, block in _images(name):
        src, tgt = A.exact(block)
        assert A.is_assignment(src, tgt, *block.shape) and A.total(block, src, tgt) == golden[f"{name}_{b}_total"].item()


@pytest.mark.parametrize("name", list(A.TIE_CASES))
def test_exact_equals_scipys_total_on_the_tie_cases(golden, name):
    for b, block in _images(name):
        src, tgt = A.exact(block)
        assert A.is_assignment(src, tgt, *block.shape)
        assert A.is_assignment(golden[f"{name}_{b}_src"], golden[f"{name}_{b}_tgt"], *block.shape)
        assert A.total(block, src, tgt) == golden[f"{name}_{b}_total"].item(), "integer costs add exactly: the optimum is one number"


@pytest.mark.parametrize("name", UNIQUE)
def test_every_unique_optimum_is_separated_by_the_margin(golden, name):
    for b, block in _images(name):
        m = golden[f"{name}_{b}_margin"].item()
        print(f"{name} image {b}: margin {m:.3g}")
        assert m >= A.MIN_MARGIN
        if block.size and block.size <= 64 * 64:                  # the stored figure is what ``margin`` gives, with scipy and with ``exact``
            for again in (A.margin(block), A.margin(block, A.exact)):
                assert again == m or abs(again - m) <= 1e-9      # == for the 1 x 1 block, whose margin is inf


def test_the_near_duplicate_case_is_the_hard_one(golden):
    """Near-duplicate queries put the runner-up within 1e-4 of the optimum: fp32 duals (2^-24 * 100 = 6e-6 per sum) would be too close to call."""
    assert A.MIN_MARGIN <= golden["dup_0_margin"].item() < 1e-4 < 1e-2 * golden["u900x20_0_margin"].item()


@pytest.mark.parametrize("sw", ["greedy", "no_dual", "swap_output", "unsorted"])
def test_each_wrong_variant_fails_at_least_one_case(golden, sw):
    failed = [name for name in UNIQUE if _fails(golden, name, **{sw: True})]
    print(f"{sw}: fails {len(failed)} of {len(UNIQUE)} cases")
    assert failed


def test_is_assignment_and_total():
    assert A.is_assignment([0, 2], [1, 0], 3, 2) and A.is_assignment([], [], 3, 0)
    assert not A.is_assignment([2, 0], [1, 0], 3, 2), "src must ascend"
    assert not A.is_assignment([0, 2], [1, 1], 3, 2), "tgt must be distinct"
    assert not A.is_assignment([0, 3], [1, 0], 3, 2) and not A.is_assignment([0, 2], [2, 0], 3, 2) and not A.is_assignment([0], [1], 3, 2)
    assert A.total(np.array([[1.0, 2.0], [3.0, 4.5]], np.float32), [0, 1], [1, 0]) == 5.0


# ------------------------------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_declares_the_assignment_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    for s in ("fvit_det_assign_workspace", "fvit_det_assign"):
        assert re.search(r"\b%s\s*\(" % s, hdr) and s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert "#define FVIT_ABI_VERSION 10" in hdr and lib.fvit_abi_version() == 10
    assert ctypes.sizeof(_lib.FvitDetAssignSet) == 3 * 8 + 4 * 4
    assert [n for n, _ in _lib.FvitDetAssignSet._fields_] == ["cost", "src", "tgt", "Q", "T", "n_pairs", "_pad"]
    assert lib.fvit_det_assign.argtypes[0]._type_ is _lib.FvitDetAssignSet and len(lib.fvit_det_assign.argtypes) == 10
    assert lib.fvit_det_assign_workspace.restype is ctypes.c_size_t
    assert "fvit_assign.hip" in open(os.path.join(ROOT, "fastervit_amd", "csrc", "Makefile")).read()
    import fastervit_amd
    from fastervit_amd import detection_ops
    assert fastervit_amd.hungarian_assign is detection_ops.hungarian_assign and detection_ops.ASSIGN_MAX_SIDE == 2048


def test_abi_refusals_that_need_no_device(lib):
    """Every refusal comes before a launch: the pointers below are not device memory."""
    p = 0x7f0000001000
    S = _lib.FvitDetAssignSet
    sets = lambda n, **k: (S * n)(*[S(**{**dict(cost=p, src=p, tgt=p, Q=7, T=5, n_pairs=5), **k}) for _ in range(n)])
    run = lambda t, n, B=2, toff=p, poff=p, max_nb=5, status=p, ws=p, nbytes=1 << 20: lib.fvit_det_assign(t, n, B, toff, poff, max_nb, status, ws, nbytes, None)
    err = lambda: lib.fvit_last_error()
    assert run(sets(1), 0) == -1 and b"n_sets=0" in err()
    assert run(sets(17), 17) == -1 and b"n_sets=17" in err()
    assert lib.fvit_det_assign_workspace(sets(17), 17, 2) == 0 and b"n_sets=17" in err()
    assert run(sets(1), 1, B=0) == -1 and b"B=0" in err()
    assert lib.fvit_det_assign_workspace(sets(1), 1, 0) == 0 and b"B=0" in err()
    assert run(sets(1, Q=0), 1) == -1 and b"Q=0" in err()
    assert run(sets(1, T=-1), 1) == -1 and b"T=-1" in err()
    assert run(sets(1, n_pairs=-1), 1) == -1 and b"n_pairs=-1" in err()
    assert run(sets(1, Q=2049), 1) == -1 and b"Q=2049" in err() and b"2048" in err()
    assert run(sets(1), 1, max_nb=2049) == -1 and b"max_nb=2049" in err() and b"2048" in err()
    assert run(sets(1), 1, max_nb=-1) == -1 and b"max_nb=-1" in err()
    assert run(None, 1) == -1 and b"null" in err()
    for k in ("cost", "src", "tgt"):
        assert run(sets(1, **{k: None}), 1) == -1 and b"null" in err(), k
        assert run(sets(1, **{k: p + 2}), 1) == -1 and b"misaligned" in err(), k
    assert run(sets(1, src=p + 4), 1) == -1 and b"misaligned" in err(), "int64 outputs are 8-byte aligned"
    for k in ("toff", "poff", "status", "ws"):
        assert run(sets(1), 1, **{k: None}) == -1 and b"null" in err(), k
        assert run(sets(1), 1, **{k: p + 2}) == -1 and b"misaligned" in err(), k
    assert run(sets(1), 1, ws=p + 8) == -1 and b"misaligned" in err(), "the workspace is 16-byte aligned"
    assert lib.fvit_det_assign_workspace(sets(3), 3, 2) == 3 * 7 * 5 * 4 + 12      # 4 * sum Q * T, rounded up to 16
    assert run(sets(3), 3, nbytes=3 * 7 * 5 * 4) == -2 and b"workspace" in err()
    assert lib.fvit_det_assign_workspace(sets(1, Q=2048, T=6000), 1, 3) == 2048 * 6000 * 4, "Q at the cap, T above it: only an image's n_b is capped"
    assert run(sets(2, T=0, cost=None, src=None, tgt=None, n_pairs=0), 2, toff=None, poff=None, status=None, ws=None, nbytes=0) == 0      # T = 0: no launch


def test_python_refusals_that_need_no_device():
    from fastervit_amd import HungarianMatcher, hungarian_assign
    with pytest.raises(RuntimeError, match="HIP device"):
        hungarian_assign(torch.zeros(1, 7, 5), [5])
    with pytest.raises(RuntimeError, match="float64"):
        hungarian_assign(torch.zeros(1, 7, 5, dtype=torch.float64), [5])
    with pytest.raises(TypeError, match="tensor"):
        hungarian_assign(np.zeros((1, 7, 5), np.float32), [5])
    with pytest.raises(ValueError, match="solver"):
        HungarianMatcher(solver="auction")
    m = HungarianMatcher()
    assert m.solver == "scipy" and m.last_status is None and m.check_status() is None
    assert HungarianMatcher(solver="device").solver == "device"


# ------------------------------------------------------------------------------------------------------------------------------ the scipy path stays
class _Costs:
    """cost_matrix of a matcher replaced by stored matrices: the host half of the scipy path runs without a device."""

    def __init__(self, mats):
        self.mats, self.calls = list(mats), 0

    def __call__(self, outputs, targets):
        self.calls += 1
        return self.mats[outputs["set"]]


@pytest.mark.parametrize("name", ["mixed", "hole", "none", "u65x3", "int33"])
def test_solver_scipy_returns_what_the_parent_commit_returns(golden, name):
    """The parent's forward is ``linear_sum_assignment`` of every block of the cost matrix copied to the host, as CPU int64 tensors; so is its
    SetCriterion._match.  The goldens are scipy's own answers (ties included: the same scipy, the same input, the same answer)."""
    from fastervit_amd import HungarianMatcher, SetCriterion
    cost, sizes = A.draw(name)
    targets = [{"labels": torch.zeros(n, dtype=torch.int64), "boxes": torch.zeros(n, 4)} for n in sizes]
    for matcher in (HungarianMatcher(), HungarianMatcher(solver="scipy")):
        matcher.cost_matrix = _Costs([torch.from_numpy(cost), torch.from_numpy(cost).to(torch.float16)])
        got = matcher({"set": 0}, targets)
        again = SetCriterion(5, matcher, {}, 0.25, [])._match([{"set": 0}, {"set": 1}], targets)
        assert matcher.cost_matrix.calls == 3 and matcher.last_status is None
        half = A.blocks(cost.astype(np.float16).astype(np.float32), sizes)
        from scipy.optimize import linear_sum_assignment
        for b, (i, j) in enumerate(got):
            for t in (i, j, *again[0][b]):
                assert t.dtype == torch.int64 and t.device.type == "cpu"
            assert torch.equal(i, torch.from_numpy(golden[f"{name}_{b}_src"])) and torch.equal(j, torch.from_numpy(golden[f"{name}_{b}_tgt"]))
            assert torch.equal(again[0][b][0], i) and torch.equal(again[0][b][1], j)
            hi, hj = linear_sum_assignment(half[b])                 # a 16-bit cost matrix is widened once: the solver sees the rounded values
            assert np.array_equal(again[1][b][0].numpy(), hi) and np.array_equal(again[1][b][1].numpy(), hj)
