"""The device assignment solver on the GPU (csrc/fvit_assign.hip through the C ABI, hungarian_assign, HungarianMatcher(solver="device") and SetCriterion on
top of it), held to tests/assignment_refs.py and the scipy goldens of tests/golden/assignment_cases.npz: indices to torch.equal on every case with one
optimum (tests/test_assignment_refs_cpu.py shows each separated from its runner-up by at least 1e-6), the fp64 total exactly on the tie cases.

Conventions as in test_gpu_criterion.py: every input is a view inside a larger NaN-filled (floats) / -1-filled (integers) buffer, every output starts as
NaN / -1 with a guard in front of and behind it that must survive (profiles/assignment_tests.log: a run on an MI355X)."""
import contextlib

import numpy as np
import pytest
import torch

from fastervit_amd import HungarianMatcher, SetCriterion, _lib, hungarian_assign
from fastervit_amd.detection_ops import assign_launch
from tests import assignment_refs as A
from tests import criterion_refs as R

pytestmark = pytest.mark.gpu

F32, I64, I32 = torch.float32, torch.int64, torch.int32
NAN = float("nan")
PAD = 64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dt):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), NAN if dt.is_floating_point else -1, dtype=dt, device="cuda")
    return buf[PAD:PAD + n].view(shape), buf


def _embed(t, dt=None):
    view, _ = _guarded(tuple(t.shape), dt or t.dtype)
    view.copy_(t.to(dt or t.dtype))
    return view


def _guards_intact(*bufs):
    for buf in bufs:
        for g in (buf[:PAD], buf[-PAD:]):
            assert (torch.isnan(g).all() if buf.dtype.is_floating_point else (g == -1).all()), "a guard region next to an output was written"


def _untouched(*bufs):
    for buf in bufs:
        assert (torch.isnan(buf).all() if buf.dtype.is_floating_point else (buf == -1).all()), "a refused call wrote an output"


def _prefix(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return out


@pytest.fixture(scope="module")
def golden():
    return A.load_golden()


class _Call:
    """One fvit_det_assign call on guarded buffers: costs is a list of (B, Q, T) fp32 arrays that share ``sizes`` and min(Q, n_b)."""

    def __init__(self, costs, sizes):
        self.lib, self.n, self.B, self.sizes = _lib.lib(), len(costs), len(sizes), list(sizes)
        self.ks = [min(costs[0].shape[1], n) for n in sizes]
        assert all([min(c.shape[1], n) for n in sizes] == self.ks for c in costs)
        self.P, self.T = sum(self.ks), sum(sizes)
        self.cost = [_embed(torch.as_tensor(c)) for c in costs]
        self.toff, self.poff = _embed(torch.tensor(_prefix(sizes), dtype=I32)), _embed(torch.tensor(_prefix(self.ks), dtype=I32))
        self.out = [(_guarded((self.P,), I64), _guarded((self.P,), I64)) for _ in costs]
        self.status, self.sb = _guarded((self.n, self.B), I32)
        S = _lib.FvitDetAssignSet
        self.table = (S * self.n)(*[S(cost=c.data_ptr(), src=o[0][0].data_ptr(), tgt=o[1][0].data_ptr(), Q=c.shape[1], T=self.T, n_pairs=self.P)
                                    for c, o in zip(self.cost, self.out)])
        self.need = self.lib.fvit_det_assign_workspace(self.table, self.n, self.B)
        assert self.need > 0 and self.need % 16 == 0, self.lib.fvit_last_error()
        self.ws, self.wb = _guarded((self.need // 4,), F32)

    def launch(self):
        return self.lib.fvit_det_assign(self.table, self.n, self.B, self.toff.data_ptr(), self.poff.data_ptr(), max(self.sizes), self.status.data_ptr(),
                                        self.ws.data_ptr(), self.need, _stream())

    def buffers(self):
        return [self.sb, self.wb] + [b for o in self.out for _, b in o]

    def run(self):
        rc = self.launch()
        torch.cuda.synchronize()
        assert rc == 0, self.lib.fvit_last_error()
        _guards_intact(*self.buffers())
        return self

    def pairs(self, s, b):
        lo, hi = _prefix(self.ks)[b], _prefix(self.ks)[b + 1]
        return self.out[s][0][0][lo:hi].cpu(), self.out[s][1][0][lo:hi].cpu()


def _scipy(block):
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(np.asarray(block))
    return torch.as_tensor(i, dtype=I64), torch.as_tensor(j, dtype=I64)


# ------------------------------------------------------------------------------------------------------------------------------------ 1: the goldens
@pytest.mark.parametrize("name", [n for n in A.case_names() if n not in A.TIE_CASES])
def test_indices_equal_the_golden(golden, name):
    cost, sizes = A.draw(name)
    assert A.checksum(cost) == golden[f"{name}_sum"].item()
    call = _Call([cost], sizes)
    if sum(sizes) == 0:                                           # no target at all: no launch, nothing written
        assert call.launch() == 0
        torch.cuda.synchronize()
        _untouched(*call.buffers())
        return
    call.run()
    assert (call.status == 0).all(), call.status
    for b in range(len(sizes)):
        src, tgt = call.pairs(0, b)
        assert torch.equal(src, torch.from_numpy(golden[f"{name}_{b}_src"])) and torch.equal(tgt, torch.from_numpy(golden[f"{name}_{b}_tgt"])), (name, b)


# --------------------------------------------------------------------------------------------------------------------------------------------- 2: ties
@pytest.mark.parametrize("name", list(A.TIE_CASES))
def test_ties_give_an_optimal_assignment_and_terminate(golden, name):
    cost, sizes = A.draw(name)
    call = _Call([cost], sizes).run()
    assert (call.status == 0).all()
    src, tgt = call.pairs(0, 0)
    assert A.is_assignment(src.numpy(), tgt.numpy(), cost.shape[1], sizes[0])
    assert A.total(cost[0], src.numpy(), tgt.numpy()) == golden[f"{name}_0_total"].item()


# --------------------------------------------------------------------------------------------------------------------------------------- 3: many sets
def _many_sets(n_sets, sizes=(4, 9, 2), seed=7900):
    g = np.random.default_rng(seed + n_sets)
    qs = [max(sizes) + 7 * s for s in range(n_sets)]              # 9 .. 114: every set has min(Q, n_b) = n_b, and Q passes 64
    return [(g.standard_normal((len(sizes), q, sum(sizes))) * 2).astype(np.float32) for q in qs]


@pytest.mark.parametrize("n_sets", [1, 3, 16])
def test_many_sets_of_different_q_in_one_launch(n_sets):
    sizes = [4, 9, 2]
    costs = _many_sets(n_sets)
    call = _Call(costs, sizes).run()
    assert (call.status == 0).all()
    for s, c in enumerate(costs):
        for b, block in enumerate(A.blocks(c, sizes)):
            src, tgt = call.pairs(s, b)
            want = _scipy(block)
            assert torch.equal(src, want[0]) and torch.equal(tgt, want[1]), (s, b)


def test_seventeen_sets_from_python_make_two_launches():
    sizes = [4, 9, 2]
    costs = _many_sets(16) + _many_sets(1, seed=7950)
    _lib.prof_enable(True)
    pairs, status = assign_launch([torch.from_numpy(c).cuda() for c in costs], sizes)
    torch.cuda.synchronize()
    launches = [r["name"] for r in _lib.prof_records()]
    _lib.prof_enable(False)
    assert launches.count("assign_kernel") == 2
    assert status.shape == (17, 3) and (status == 0).all()
    off = _prefix(sizes)
    for s, c in enumerate(costs):
        for b, block in enumerate(A.blocks(c, sizes)):
            want = _scipy(block)
            assert torch.equal(pairs[s][0, off[b]:off[b + 1]].cpu(), want[0]) and torch.equal(pairs[s][1, off[b]:off[b + 1]].cpu(), want[1]), (s, b)


# ------------------------------------------------------------------------------------------------------------------------------------- 4: non-finite
def _poison(block, kind):
    if kind == "nan":
        block[5, 3] = np.nan
    elif kind == "neg_inf":
        block[0, 0] = -np.inf
    elif kind == "inf_row":
        block[7, :] = np.inf
    else:                                                         # one +inf entry: scipy routes around it, the device solver does not look further
        block[32, 8] = np.inf


@pytest.mark.parametrize("kind", ["nan", "neg_inf", "inf_row", "inf_entry"])
def test_a_non_finite_cost_gives_status_1_and_the_identity_and_spares_the_neighbours(kind):
    cost, sizes = A.draw("mixed")                                 # Q = 33, targets 4, 9, 2
    clean = cost.copy()
    _poison(cost[1][:, 4:13], kind)
    call = _Call([cost, clean], sizes).run()
    assert call.status.cpu().tolist() == [[0, 1, 0], [0, 0, 0]]
    src, tgt = call.pairs(0, 1)
    assert torch.equal(src, torch.arange(9)) and torch.equal(tgt, torch.arange(9)), "the identity pairing"
    for s, b in ((0, 0), (0, 2), (1, 0), (1, 1), (1, 2)):
        src, tgt = call.pairs(s, b)
        want = _scipy(A.blocks(clean, sizes)[b])
        assert torch.equal(src, want[0]) and torch.equal(tgt, want[1]), (s, b)


# ------------------------------------------------------------------------------------------------------------------------------ 5: graphs, repeats
def test_captured_once_and_replayed_with_new_costs_and_two_launches_agree_bitwise():
    sizes = [20, 3]
    g = np.random.default_rng(7990)
    draw = lambda: [(g.standard_normal((2, q, 23)) * 2).astype(np.float32) for q in (65, 130)]
    call = _Call(draw(), sizes)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call.launch() == 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    outs = lambda: [t.clone() for o in call.out for (t, _) in o] + [call.status.clone()]
    for _ in range(2):
        costs = draw()
        for dst, c in zip(call.cost, costs):
            dst.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        replayed = outs()
        for o in call.out:
            o[0][0].fill_(-1), o[1][0].fill_(-1)
        call.run()
        plain = outs()
        call.run()
        assert all(torch.equal(x, y) for x, y in zip(replayed, plain)), "a replay and a plain launch differ"
        assert all(torch.equal(x, y) for x, y in zip(plain, outs())), "two plain launches differ"
        for s, c in enumerate(costs):
            for b, block in enumerate(A.blocks(c, sizes)):
                src, tgt = call.pairs(s, b)
                want = _scipy(block)
                assert torch.equal(src, want[0]) and torch.equal(tgt, want[1]), (s, b)


# ------------------------------------------------------------------------------------------------------------------------------------- 6: refusals
def test_abi_refusals_leave_the_outputs_untouched():
    cost, sizes = A.draw("mixed")
    call = _Call([cost], sizes)
    lib, S = call.lib, _lib.FvitDetAssignSet
    base = dict(cost=call.cost[0].data_ptr(), src=call.out[0][0][0].data_ptr(), tgt=call.out[0][1][0].data_ptr(), Q=33, T=15, n_pairs=15)
    sets = lambda n, **k: (S * n)(*[S(**{**base, **k}) for _ in range(n)])
    args = dict(B=3, toff=call.toff.data_ptr(), poff=call.poff.data_ptr(), max_nb=9, status=call.status.data_ptr(), ws=call.ws.data_ptr(), nbytes=call.need)

    def run(t, n, **k):
        a = {**args, **k}
        return lib.fvit_det_assign(t, n, a["B"], a["toff"], a["poff"], a["max_nb"], a["status"], a["ws"], a["nbytes"], _stream())

    for fn, code, word in ((lambda: run(sets(1), 0), -1, b"n_sets=0"), (lambda: run(sets(17), 17), -1, b"n_sets=17"), (lambda: run(sets(1), 1, B=0), -1, b"B=0"),
                           (lambda: run(sets(1, Q=0), 1), -1, b"Q=0"), (lambda: run(sets(1, T=-1), 1), -1, b"T=-1"),
                           (lambda: run(sets(1, Q=2049), 1), -1, b"Q=2049"), (lambda: run(sets(1), 1, max_nb=2049), -1, b"max_nb=2049"),
                           (lambda: run(sets(1, cost=None), 1), -1, b"null"), (lambda: run(sets(1, tgt=None), 1), -1, b"null"),
                           (lambda: run(sets(1, src=base["src"] + 4), 1), -1, b"misaligned"), (lambda: run(sets(1, cost=base["cost"] + 2), 1), -1, b"misaligned"),
                           (lambda: run(sets(1), 1, status=None), -1, b"null"), (lambda: run(sets(1), 1, toff=args["toff"] + 2), -1, b"misaligned"),
                           (lambda: run(sets(1), 1, ws=args["ws"] + 8), -1, b"misaligned"), (lambda: run(sets(1), 1, nbytes=call.need - 16), -2, b"workspace")):
        rc = fn()
        assert rc == code and word in lib.fvit_last_error(), (rc, word, lib.fvit_last_error())
    torch.cuda.synchronize()
    _untouched(*call.buffers())
    # offsets that contradict the call are seen on the device: status 3, no pair written
    assert run(sets(1), 1, max_nb=8) == 0
    torch.cuda.synchronize()
    assert call.status.cpu().tolist() == [[0, 3, 0]]
    _guards_intact(*call.buffers())
    assert (call.pairs(0, 1)[0] == -1).all() and (call.pairs(0, 1)[1] == -1).all()
    assert torch.equal(call.pairs(0, 0)[0], _scipy(A.blocks(cost, sizes)[0])[0])


# ----------------------------------------------------------------------------------------------------------------------------------- 7, 8: Python
def _cuda_case(case, dtype=F32):
    outputs, targets, indices = R.forward_inputs(case)
    dev = R.convert(outputs, lambda v: v.to(dtype).cuda().requires_grad_(True))
    tg = R.convert_targets(targets, lambda v: (v.to(dtype) if v.is_floating_point() else v).cuda())
    return outputs, targets, dev, tg


def _criterion(case, solver):
    c = R.FORWARD_CASES[case]
    return SetCriterion(c["C"], HungarianMatcher(**R.MATCH_WEIGHTS, solver=solver), R.weight_dict(c["aux"], c["interm"]), R.FOCAL_ALPHA, list(R.LOSSES))


CASES = range(len(R.FORWARD_CASES))
IDS = [c["name"] for c in R.FORWARD_CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_matcher_gives_the_stored_matcher_indices_as_device_tensors(case):
    crit_golden = R.load_golden()
    name = R.FORWARD_CASES[case]["name"]
    outputs, _, dev, tg = _cuda_case(case)
    matcher = HungarianMatcher(**R.MATCH_WEIGHTS, solver="device")
    for s, o in enumerate(R.matched_sets(dev)):
        ind = matcher(o, tg)
        assert len(ind) == len(tg) and matcher.last_status.shape == (1, len(tg)) and matcher.last_status.is_cuda
        matcher.check_status()
        for b, (i, j) in enumerate(ind):
            assert i.is_cuda and j.is_cuda and i.dtype == I64 and j.dtype == I64
            assert torch.equal(i.cpu(), crit_golden[f"{name}_idx{s}_{b}_src"]) and torch.equal(j.cpu(), crit_golden[f"{name}_idx{s}_{b}_tgt"]), (s, b)


def _raise_on_host_read(*_a, **_k):
    raise RuntimeError("a device tensor was read on the host")


@contextlib.contextmanager
def _no_host_sync():
    """torch's sync debug mode at "error" when this build flags a plain .cpu() under it; otherwise .cpu / .item / .tolist / .numpy of device tensors raise."""
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.cpu()
            flags = False
        except RuntimeError:
            flags = True
    finally:
        torch.cuda.set_sync_debug_mode(before)
    print(f"sync debug mode flags a plain .cpu(): {flags}")
    if flags:
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield "sync_debug_mode"
        finally:
            torch.cuda.set_sync_debug_mode(before)
        return
    saved = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}

    def guard(fn):
        return lambda self, *a, **k: _raise_on_host_read() if self.is_cuda else fn(self, *a, **k)
    for n, fn in saved.items():
        setattr(torch.Tensor, n, guard(fn))
    try:
        yield "patched"
    finally:
        for n, fn in saved.items():
            setattr(torch.Tensor, n, fn)


def test_the_sync_guard_catches_a_host_read():
    x = torch.ones(3, device="cuda")
    with _no_host_sync():
        with pytest.raises(RuntimeError):
            x.cpu()
    assert x.cpu().sum().item() == 3.0                           # and is gone afterwards


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_set_criterion_with_the_device_matcher(case):
    from tests import test_gpu_criterion as TC                   # its bars and shared references, as they are
    crit_golden = R.load_golden()
    c = R.FORWARD_CASES[case]
    name = c["name"]
    outputs, _, dev, tg = _cuda_case(case)
    _, _, dev2, _ = _cuda_case(case)
    weights = R.weight_dict(c["aux"], c["interm"])
    ref_losses, ref_ind = _criterion(case, "scipy")(dev2, tg, return_indices=True)
    crit = _criterion(case, "device")
    _lib.prof_enable(True)
    with _no_host_sync():
        losses, ind_list = crit(dev, tg, return_indices=True)
    torch.cuda.synchronize()
    launches = [r["name"] for r in _lib.prof_records()]
    _lib.prof_enable(False)
    n_matched = len(R.matched_sets(outputs))
    assert launches.count("assign_kernel") == (-(-n_matched // 16) if sum(c["nt"]) else 0)
    crit.matcher.check_status()
    assert crit.matcher.last_status.shape == (n_matched, c["B"])
    TC._check_losses(name, losses, crit_golden, case)
    assert sorted(losses) == sorted(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses), "not bitwise the scipy path's losses"
    assert len(ind_list) == len(ref_ind)
    for got, want in zip(ind_list, ref_ind):
        for (i, j), (wi, wj) in zip(got, want):
            assert i.is_cuda and j.is_cuda and torch.equal(i.cpu(), wi) and torch.equal(j.cpu(), wj)
    sum(losses[k] * weights[k] for k in losses if k in weights).backward()
    sum(ref_losses[k] * weights[k] for k in ref_losses if k in weights).backward()
    (_, _, gex), (_, _, g32) = TC._case_refs(case)
    leaves = [(s, k, o[k], o2[k]) for (s, o), (_, o2) in zip(R.pred_sets(dev), R.pred_sets(dev2)) for k in ("pred_logits", "pred_boxes")]
    for (s, k, leaf, leaf2), ge, gp in zip(leaves, gex, g32):
        got = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        ref = leaf2.grad if leaf2.grad is not None else torch.zeros_like(leaf2)
        assert torch.equal(got, ref), f"d{s}.{k} is not bitwise the scipy path's gradient"
        TC._elementwise(f"device matcher {name} d{s}.{k}", got.cpu(), crit_golden[f"{name}_grad_{s}_{k[5:]}"], gp)


# ------------------------------------------------------------------------------------------------------------------------------- 9, 10: dtypes, refusals
def test_fp16_costs_are_widened_once():
    cost, sizes = A.draw("mixed")
    half = torch.from_numpy(cost).to(torch.float16)
    ind, status = hungarian_assign(half.cuda(), sizes)
    assert status.dtype == I32 and status.is_cuda and (status == 0).all()
    for b, block in enumerate(A.blocks(half.float().numpy(), sizes)):
        i, j = ind[b][0].cpu().numpy(), ind[b][1].cpu().numpy()
        want = _scipy(block)
        assert ind[b][0].dtype == I64 and A.is_assignment(i, j, *block.shape)
        assert A.total(block, i, j) == A.total(block, want[0].numpy(), want[1].numpy()), "fp16 values add exactly in fp64: the optimum of the rounded costs"


def test_python_refusals():
    cost, sizes = A.draw("mixed")
    c = torch.from_numpy(cost).cuda()
    with pytest.raises(RuntimeError, match="float64"):
        hungarian_assign(c.double(), sizes)
    with pytest.raises(RuntimeError, match="HIP device"):
        hungarian_assign(c.cpu(), sizes)
    with pytest.raises(RuntimeError, match="dtype"):
        hungarian_assign(c.to(torch.int32), sizes)
    with pytest.raises(RuntimeError, match=r"\(B, Q, T\)"):
        hungarian_assign(c[0], sizes)
    with pytest.raises(RuntimeError, match="sum of sizes"):
        hungarian_assign(c, [4, 9, 3])
    with pytest.raises(RuntimeError, match="sizes"):
        hungarian_assign(c, [])
    with pytest.raises(RuntimeError, match="2048"):
        hungarian_assign(torch.zeros(1, 2049, 1, device="cuda"), [1])
    with pytest.raises(RuntimeError, match="min"):
        assign_launch([c, c[:, :8].contiguous()], sizes)
    ind, status = hungarian_assign(c, sizes)
    assert [tuple(i.shape) for i, _ in ind] == [(4,), (9,), (2,)] and status.tolist() == [0, 0, 0]
    # a NaN prediction: the solver does not run on that image, and check_status says so on request, in scipy's words
    _, _, dev, tg = _cuda_case(1)
    with torch.no_grad():
        dev["pred_boxes"][1, 3, 0] = NAN
    matcher = HungarianMatcher(**R.MATCH_WEIGHTS, solver="device")
    ind = matcher(dev, tg)
    assert matcher.last_status.tolist() == [[0, 1]] and torch.equal(ind[1][0].cpu(), torch.arange(5)) and torch.equal(ind[1][1].cpu(), torch.arange(5))
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        matcher.check_status()
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        matcher.check_status()
