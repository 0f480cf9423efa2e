"""Detection post-processing on the GPU (csrc/fvit_boxes.hip through the C ABI, and fastervit_amd/detection_ops.py on top of it), held to
tests/detection_refs.py: values (scores, IoU, GIoU, cost) to the float64 restatement at the bar of backward_primitive_refs, indices, labels, keeps, counts
and fp32 boxes to torch.equal (tests/test_detection_refs_cpu.py shows the restatements equal the reference's programs and that wrong variants fail).

Conventions: every input is a view inside a larger NaN-filled (floats) / -1-filled (integers) buffer, every output starts as NaN / -1 with such a guard
in front of and behind it that must survive, every result of a finite case must be finite.  Each value test prints its worst |err| / bound; 1.0 is the
bar (profiles/detection_tests.log: a run on an MI355X)."""
import pytest
import torch

from fastervit_amd import _lib, detection_ops as D
from tests import detection_refs as R

pytestmark = pytest.mark.gpu

F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32
NAN = float("nan")
PAD = 64      # guard elements in front of and behind every buffer (a multiple of 16 bytes for every type used)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fill(dt):
    return NAN if dt.is_floating_point else -1


def _guarded(shape, dt):
    """A dense device tensor of ``shape`` in the middle of a buffer whose every element (the tensor's too) is NaN / -1."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), _fill(dt), dtype=dt, device="cuda")
    return buf[PAD:PAD + n].view(shape), buf


def _embed(t, dt=None):
    dt = dt or t.dtype
    view, buf = _guarded(tuple(t.shape), dt)
    view.copy_(t.to(dt))
    return view


def _guards_intact(*bufs):
    for buf in bufs:
        for g in (buf[:PAD], buf[-PAD:]):
            ok = torch.isnan(g).all() if buf.dtype.is_floating_point else (g == -1).all()
            assert ok, "a guard region next to an output was written"


def _untouched(*bufs):
    for buf in bufs:
        assert (torch.isnan(buf).all() if buf.dtype.is_floating_point else (buf == -1).all()), "a refused call wrote an output"


def _under_bar(name, got, exact, plain32):
    assert got.dtype == F32 and torch.isfinite(got).all(), f"{name}: a non-finite result"
    r = R.worst_ratio(got.reshape(exact.shape), exact, plain32, F32)
    print(f"{name}: worst |err|/bound = {r:.3f}")
    assert r <= 1.0, f"{name}: {r:.3f} x the bar"


# ------------------------------------------------------------------------------------------------------------------------------------------- select
def _select_abi(logits, boxes, sizes, K, raw=False, test=False):
    B, Q, C = logits.shape
    dl, db, ds = _embed(logits), _embed(boxes), _embed(sizes)
    (s, sb), (l, lb), (q, qb), (b, bb) = _guarded((B, K), F32), _guarded((B, K), I64), _guarded((B, K), I64), _guarded((B, K, 4), F32)
    rc = _lib.lib().fvit_det_select(dl.data_ptr(), db.data_ptr(), ds.data_ptr(), s.data_ptr(), l.data_ptr(), q.data_ptr(), b.data_ptr(), B, Q, C, K,
                                    int(raw), int(test), _stream())
    torch.cuda.synchronize()
    return rc, (s, l, q, b), (sb, lb, qb, bb)


@pytest.mark.parametrize("case,raw,test", R.SELECT_RUNS, ids=[R.run_name(*r) for r in R.SELECT_RUNS])
def test_select_value_cases(case, raw, test):
    golden = R.load_golden()
    name = R.run_name(case, raw, test)
    logits, boxes, sizes, K = R.select_inputs(case)
    ex = R.select(logits, boxes, sizes, K, F64, raw, test)
    p32 = R.select(logits, boxes, sizes, K, F32, raw, test)
    rc, (s, l, q, b), bufs = _select_abi(logits, boxes, sizes, K, raw, test)
    assert rc == 0, _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    _under_bar(f"abi {name} scores", s.cpu(), golden[f"{name}_scores"], p32[0])
    assert torch.equal(l.cpu(), golden[f"{name}_labels"]) and torch.equal(q.cpu(), ex[2])
    assert torch.isfinite(b).all() and torch.equal(b.cpu(), golden[f"{name}_boxes32"]), "fp32 boxes differ from the reference's"
    res = D.PostProcess(num_select=K)({"pred_logits": _embed(logits), "pred_boxes": _embed(boxes)}, _embed(sizes), not_to_xyxy=raw, test=test)
    assert len(res) == logits.shape[0] and all(set(r) == {"scores", "labels", "boxes"} for r in res)
    _under_bar(f"api {name} scores", torch.stack([r["scores"] for r in res]).cpu(), golden[f"{name}_scores"], p32[0])
    assert torch.equal(torch.stack([r["labels"] for r in res]).cpu(), golden[f"{name}_labels"])
    assert torch.equal(torch.stack([r["boxes"] for r in res]).cpu(), golden[f"{name}_boxes32"])


@pytest.mark.parametrize("name", R.SELECT_EXACT)
def test_select_ties_go_to_the_lower_index_and_nan_ranks_first(name):
    logits, boxes, sizes, K = R.select_exact_inputs(name)
    ex = R.select(logits, boxes, sizes, K, F64)
    p32 = R.select(logits, boxes, sizes, K, F32)
    rc, (s, l, q, b), bufs = _select_abi(logits, boxes, sizes, K)
    assert rc == 0, _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    assert torch.equal(l.cpu(), ex[1]) and torch.equal(q.cpu(), ex[2]) and torch.equal(b.cpu(), p32[3])
    nan = torch.isnan(ex[0])
    assert torch.equal(torch.isnan(s.cpu()), nan)
    _under_bar(f"abi {name} scores", torch.where(nan, torch.zeros_like(s.cpu()), s.cpu()), torch.where(nan, torch.zeros_like(ex[0]), ex[0]),
               torch.where(nan, torch.zeros_like(p32[0]), p32[0]))
    res = D.PostProcess(num_select=K)({"pred_logits": logits.cuda(), "pred_boxes": boxes.cuda()}, sizes.cuda())
    assert torch.equal(torch.stack([r["labels"] for r in res]).cpu(), ex[1]) and torch.equal(torch.stack([r["boxes"] for r in res]).cpu(), p32[3])


def test_select_accepts_16_bit_inputs_and_integer_sizes():
    logits, boxes, sizes, K = R.select_inputs(2)
    for dt in (torch.float16, torch.bfloat16):
        lg, bx = logits.to(dt), boxes.to(dt)
        res = D.PostProcess(num_select=K)({"pred_logits": lg.cuda(), "pred_boxes": bx.cuda()}, sizes.long().cuda())
        ex = R.select(lg.float(), bx.float(), sizes, K, F32)
        idx = torch.stack([r["labels"] for r in res]).cpu()
        assert res[0]["scores"].dtype == dt and res[0]["boxes"].dtype == dt and idx.dtype == I64
        assert torch.equal(torch.stack([r["boxes"] for r in res]).cpu(), ex[3].to(dt))      # widened, computed in fp32, narrowed once
        assert torch.equal(idx, ex[1])


# ---------------------------------------------------------------------------------------------------------------------------------------------- NMS
def _nms_abi(boxes, order, idxs, thr):
    G, N = boxes.shape[:2]
    lib = _lib.lib()
    db = _embed(boxes)
    do = _embed(order) if order is not None else None
    di = _embed(idxs) if idxs is not None else None
    (keep, kb), (count, cb) = _guarded((G, N), I64), _guarded((G,), I32)
    nbytes = lib.fvit_box_nms_workspace(G, N)
    assert nbytes == G * N * ((N + 63) // 64) * 8
    ws, wsb = _guarded((nbytes // 8,), I64)
    rc = lib.fvit_box_nms(db.data_ptr(), do.data_ptr() if do is not None else None, di.data_ptr() if di is not None else None, thr, keep.data_ptr(),
                          count.data_ptr(), ws.data_ptr(), nbytes, G, N, _stream())
    torch.cuda.synchronize()
    return rc, keep, count, (kb, cb, wsb)


@pytest.mark.parametrize("with_order", [False, True], ids=["sorted", "order"])
@pytest.mark.parametrize("with_idxs", [False, True], ids=["nms", "batched"])
@pytest.mark.parametrize("G", R.NMS_G)
@pytest.mark.parametrize("N", R.NMS_N)
def test_nms_value_cases(N, G, with_idxs, with_order):
    boxes, order, idxs, scores = R.nms_inputs(N, G, with_idxs, with_order)
    want_keep, want_count = R.nms_groups(boxes, order, R.NMS_THR, F64, idxs)
    rc, keep, count, bufs = _nms_abi(boxes, order, idxs, R.NMS_THR)
    assert rc == 0, _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    assert torch.equal(count.cpu(), want_count) and torch.equal(keep.cpu(), want_keep)
    for g in range(G):      # the torchvision signatures; without scores of its own a case gets descending ones (its boxes are in score order)
        sc = scores[g] if scores is not None else -torch.arange(N, dtype=F32)
        got = D.batched_nms(_embed(boxes[g]), sc.cuda(), idxs[g].cuda(), R.NMS_THR) if with_idxs else D.nms(_embed(boxes[g]), sc.cuda(), R.NMS_THR)
        assert got.dtype == I64 and torch.equal(got.cpu(), want_keep[g, :int(want_count[g])])


@pytest.mark.parametrize("name", R.NMS_EXACT)
def test_nms_exact_cases(name):
    b, want, thr = R.nms_exact_inputs(name)
    rc, keep, count, bufs = _nms_abi(b[None].to(F32), None, None, thr)
    assert rc == 0, _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    assert int(count[0]) == len(want) and keep[0, :len(want)].tolist() == want and (keep[0, len(want):] == -1).all()
    got = D.nms(b.cuda(), -torch.arange(b.shape[0], dtype=F32).cuda(), thr)
    assert got.tolist() == want
    assert D.nms(torch.zeros(0, 4, device="cuda"), torch.zeros(0, device="cuda"), 0.5).shape == (0,)


def test_nms_ignores_order_entries_out_of_range():
    """An order entry outside [0, N) is never used as an address: its position behaves like a box that overlaps nothing."""
    boxes = torch.tensor([[[0.0, 0.0, 10.0, 10.0], [0.0, 1.0, 10.0, 11.0], [50.0, 50.0, 60.0, 60.0]]])
    order = torch.tensor([[0, 7, 1]])
    rc, keep, count, bufs = _nms_abi(boxes, order, None, 0.5)
    assert rc == 0
    _guards_intact(*bufs)
    assert int(count[0]) == 2 and keep[0].tolist() == [0, 7, -1]


# ------------------------------------------------------------------------------------------------------------------------------- pairwise and cost
@pytest.mark.parametrize("case", range(len(R.PAIR_CASES)))
def test_pairwise_iou_and_giou(case):
    golden = R.load_golden()
    b1, b2 = R.pair_inputs(case)
    N, M = R.PAIR_CASES[case]
    p_iou, p_union = R.pair_iou(b1, b2, F32)
    p_giou = R.pair_giou(b1, b2, F32)
    lib = _lib.lib()
    d1, d2 = _embed(b1), _embed(b2)
    (iou, ib), (union, ub), (giou, gb) = _guarded((N, M), F32), _guarded((N, M), F32), _guarded((N, M), F32)
    rc1 = lib.fvit_box_pairwise(_lib.FVIT_BOX_IOU, d1.data_ptr(), d2.data_ptr(), iou.data_ptr(), union.data_ptr(), N, M, _stream())
    rc2 = lib.fvit_box_pairwise(_lib.FVIT_BOX_GIOU, d1.data_ptr(), d2.data_ptr(), giou.data_ptr(), None, N, M, _stream())
    torch.cuda.synchronize()
    assert (rc1, rc2) == (0, 0), lib.fvit_last_error()
    _guards_intact(ib, ub, gb)
    a_iou, a_union = D.box_iou(d1, d2)
    a_giou = D.generalized_box_iou(d1, d2)
    for who, g_iou, g_union, g_giou in (("abi", iou, union, giou), ("api", a_iou, a_union, a_giou)):
        _under_bar(f"{who} pair{case} iou", g_iou.cpu(), golden[f"pair{case}_iou"], p_iou)
        _under_bar(f"{who} pair{case} union", g_union.cpu(), golden[f"pair{case}_union"], p_union)
        _under_bar(f"{who} pair{case} giou", g_giou.cpu(), golden[f"pair{case}_giou"], p_giou)


def _cost_abi(logits, pred, ids, tgt):
    R_, C = logits.shape
    T = tgt.shape[0]
    w = R.COST_WEIGHTS
    cost, cb = _guarded((R_, T), F32)
    dl, dp, di, dt_ = _embed(logits), _embed(pred), _embed(ids), _embed(tgt)      # kept alive until the synchronize below
    rc = _lib.lib().fvit_det_matcher_cost(dl.data_ptr(), dp.data_ptr(), di.data_ptr(), dt_.data_ptr(), cost.data_ptr(),
                                          R_, C, T, w["cost_class"], w["cost_bbox"], w["cost_giou"], w["focal_alpha"], _stream())
    torch.cuda.synchronize()
    return rc, cost, cb


@pytest.mark.parametrize("case", range(len(R.COST_CASES)))
def test_matcher_cost(case):
    golden = R.load_golden()
    logits, pred, ids, tgt = R.cost_inputs(case)
    p32 = R.matcher_cost(logits, pred, ids, tgt, F32, **R.COST_WEIGHTS)
    rc, cost, cb = _cost_abi(logits, pred, ids, tgt)
    assert rc == 0, _lib.lib().fvit_last_error()
    _guards_intact(cb)
    _under_bar(f"abi cost{case}", cost.cpu(), golden[f"cost{case}_C"], p32)
    m = D.HungarianMatcher(**R.COST_WEIGHTS)
    api = m.cost_matrix({"pred_logits": _embed(logits)[None], "pred_boxes": _embed(pred)[None]}, [{"labels": ids.cuda(), "boxes": _embed(tgt)}])
    assert tuple(api.shape) == (1, logits.shape[0], tgt.shape[0])
    _under_bar(f"api cost{case}", api[0].cpu(), golden[f"cost{case}_C"], p32)
    # one target id out of range: its column is NaN, every other column is unchanged, nothing is read out of bounds
    bad = ids.clone()
    col = int(tgt.shape[0]) // 2
    bad[col] = logits.shape[1] if case % 2 == 0 else -1
    rc, cost2, cb = _cost_abi(logits, pred, bad, tgt)
    assert rc == 0
    _guards_intact(cb)
    assert torch.isnan(cost2[:, col]).all()
    others = [t for t in range(tgt.shape[0]) if t != col]
    assert torch.equal(cost2[:, others], cost[:, others])


# ------------------------------------------------------------------------------------------------------------------------------------- the modules
def test_postprocess_with_nms_equals_the_golden():
    golden = R.load_golden()
    logits, boxes, sizes, K = R.select_inputs(R.PP_NMS_CASE)
    p32 = R.select(logits, boxes, sizes, K, F32)
    res = D.PostProcess(num_select=K, nms_iou_threshold=R.PP_NMS_THR)({"pred_logits": _embed(logits), "pred_boxes": _embed(boxes)}, _embed(sizes))
    counts = golden["ppnms_counts"].tolist()
    assert [len(r["scores"]) for r in res] == counts
    keep, _ = R.nms_groups(p32[3], None, R.PP_NMS_THR, F32)
    p32_scores = torch.cat([p32[0][i][keep[i, :n]] for i, n in enumerate(counts)])
    _under_bar("api postprocess+nms scores", torch.cat([r["scores"] for r in res]).cpu(), golden["ppnms_scores"], p32_scores)
    assert torch.equal(torch.cat([r["labels"] for r in res]).cpu(), golden["ppnms_labels"])
    got_boxes = torch.cat([r["boxes"] for r in res]).cpu()
    assert torch.equal(got_boxes, torch.cat([p32[3][i][keep[i, :n]] for i, n in enumerate(counts)])), "fp32 boxes differ from the reference's"
    assert (got_boxes.double() - golden["ppnms_boxes"]).abs().max().item() <= 2.0 ** -20 * golden["ppnms_boxes"].abs().max().item()


def test_hungarian_matcher_finds_an_optimal_assignment():
    scipy_opt = pytest.importorskip("scipy.optimize")
    golden = R.load_golden()
    for case in range(len(R.COST_CASES)):
        logits, pred, ids, tgt = R.cost_inputs(case)
        Cg = golden[f"cost{case}_C"]
        m = D.HungarianMatcher(**R.COST_WEIGHTS)
        out = m({"pred_logits": logits.cuda()[None], "pred_boxes": pred.cuda()[None]}, [{"labels": ids.cuda(), "boxes": tgt.cuda()}])
        assert len(out) == 1
        i, j = out[0]
        n = min(Cg.shape)
        assert i.dtype == I64 and j.dtype == I64 and i.numel() == n and len(set(i.tolist())) == n and len(set(j.tolist())) == n
        ri, rj = scipy_opt.linear_sum_assignment(Cg.numpy())
        best = Cg.numpy()[ri, rj].sum()
        p32 = R.matcher_cost(logits, pred, ids, tgt, F32, **R.COST_WEIGHTS)
        bar = R.bound(Cg, p32, F32).max().item()
        got = Cg[i, j].sum().item()
        print(f"matcher case {case}: total cost {got:.9f} vs optimum {best:.9f} (bar {bar * n:.2e})")
        assert abs(got - best) <= bar * n      # the cost bar times the number of matches


def _replay_inputs(B, Q, C, K, seed):
    """New logits for a replay whose candidate boxes keep every IoU away from the NMS threshold (so fp32 and float64 keeps agree)."""
    _, boxes, sizes, _ = R.select_inputs(R.PP_NMS_CASE)
    for attempt in range(64):
        g = torch.Generator().manual_seed(9000 + 64 * seed + attempt)
        logits = (torch.randn(B, Q, C, generator=g) - 2.0).to(F32)
        if R.nms_condition(R.select(logits, boxes, sizes, K, F32)[3], R.PP_NMS_THR):
            return logits
    raise AssertionError("no seed")


def test_postprocess_launch_is_captured_and_replayed_with_new_logits():
    B, Q, C, K = R.SELECT_CASES[R.PP_NMS_CASE]
    _, boxes, sizes, _ = R.select_inputs(R.PP_NMS_CASE)
    d_logits, d_boxes, d_sizes = _embed(torch.zeros(B, Q, C)), _embed(boxes), _embed(sizes)
    (s, sb), (l, lb), (q, qb), (b, bb) = _guarded((B, K), F32), _guarded((B, K), I64), _guarded((B, K), I64), _guarded((B, K, 4), F32)
    (keep, kb), (count, cb) = _guarded((B, K), I64), _guarded((B,), I32)
    ws = D.nms_workspace(B, K, "cuda")
    launch = lambda: D.postprocess_launch(d_logits, d_boxes, d_sizes, s, l, b, q, nms_iou_threshold=R.PP_NMS_THR, keep=keep, count=count, workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for seed in range(3):
        logits = _replay_inputs(B, Q, C, K, seed)
        d_logits.copy_(logits)
        graph.replay()
        torch.cuda.synchronize()
        ex = R.select(logits, boxes, sizes, K, F64)
        p32 = R.select(logits, boxes, sizes, K, F32)
        want_keep, want_count = R.nms_groups(p32[3], None, R.PP_NMS_THR, F64)
        _guards_intact(sb, lb, qb, bb, kb, cb)
        _under_bar(f"replay {seed} scores", s.cpu(), ex[0], p32[0])
        assert torch.equal(l.cpu(), ex[1]) and torch.equal(q.cpu(), ex[2]) and torch.equal(b.cpu(), p32[3])
        assert torch.equal(count.cpu(), want_count) and torch.equal(keep.cpu(), want_keep)


def test_every_output_repeats_bitwise():
    logits, boxes, sizes, K = R.select_inputs(6)
    a, b = _select_abi(logits, boxes, sizes, K)[1], _select_abi(logits, boxes, sizes, K)[1]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    nb, order, idxs, _ = R.nms_inputs(300, 3, True, True)
    (_, k1, c1, _), (_, k2, c2, _) = _nms_abi(nb, order, idxs, R.NMS_THR), _nms_abi(nb, order, idxs, R.NMS_THR)
    assert torch.equal(k1, k2) and torch.equal(c1, c2)
    b1, b2 = (t.cuda() for t in R.pair_inputs(2))
    assert torch.equal(D.generalized_box_iou(b1, b2), D.generalized_box_iou(b1, b2)) and torch.equal(D.box_iou(b1, b2)[0], D.box_iou(b1, b2)[0])
    ci = R.cost_inputs(2)
    assert torch.equal(_cost_abi(*ci)[1], _cost_abi(*ci)[1])


def test_unsupported_calls_are_refused_by_name_before_a_launch():
    lib = _lib.lib()
    logits, boxes, sizes, K = R.select_inputs(1)
    B, Q, C = logits.shape
    dl, db, ds = _embed(logits), _embed(boxes), _embed(sizes)
    (s, sb), (l, lb), (q, qb), (b, bb) = _guarded((B, 64), F32), _guarded((B, 64), I64), _guarded((B, 64), I64), _guarded((B, 64, 4), F32)
    sel = lambda B_, Q_, C_, K_, raw=0, test=0: lib.fvit_det_select(dl.data_ptr(), db.data_ptr(), ds.data_ptr(), s.data_ptr(), l.data_ptr(), q.data_ptr(),
                                                                    b.data_ptr(), B_, Q_, C_, K_, raw, test, _stream())
    for args, word in (((0, Q, C, K), b"B=0"), ((B, Q, C, 0), b"K=0"), ((B, Q, C, Q * C + 1), b"K=36"), ((B, 4096, 4096, 3), b"2^24"),
                       ((B, Q, C, K, 1, 1), b"not_to_xyxy")):
        assert sel(*args) == -1 and word in lib.fvit_last_error(), (args, lib.fvit_last_error())
    (keep, kb), (count, cb) = _guarded((1, 64), I64), _guarded((1,), I32)
    assert lib.fvit_box_nms(db.data_ptr(), None, None, 0.5, keep.data_ptr(), count.data_ptr(), keep.data_ptr(), 1 << 30, 1, 8193, _stream()) == -1
    assert b"N=8193" in lib.fvit_last_error()
    assert lib.fvit_box_nms(db.data_ptr(), None, None, 0.5, keep.data_ptr(), count.data_ptr(), keep.data_ptr(), 8, 1, 14, _stream()) == -2
    assert lib.fvit_box_nms(db.data_ptr(), None, None, 0.5, keep.data_ptr(), count.data_ptr(), keep.data_ptr(), 0, 1, 0, _stream()) == 0      # N = 0
    assert lib.fvit_box_pairwise(7, db.data_ptr(), db.data_ptr(), s.data_ptr(), None, 2, 2, _stream()) == -1 and b"mode 7" in lib.fvit_last_error()
    assert lib.fvit_det_matcher_cost(dl.data_ptr(), db.data_ptr(), l.data_ptr(), db.data_ptr(), s.data_ptr(), 2, 0, 2, 1.0, 1.0, 1.0, 0.25, _stream()) == -1
    torch.cuda.synchronize()
    _untouched(sb, lb, qb, bb, kb, cb)
    # the Python side: float64 by name, forward only, sizes
    bx = torch.rand(4, 4, device="cuda")
    with pytest.raises(RuntimeError, match="float64"):
        D.box_iou(bx.double(), bx)
    with pytest.raises(RuntimeError, match="float64"):
        D.nms(bx.double(), torch.rand(4, device="cuda"), 0.5)
    with pytest.raises(RuntimeError, match="float64"):
        D.PostProcess(2)({"pred_logits": dl.double(), "pred_boxes": db}, ds)
    with pytest.raises(RuntimeError, match="float64"):
        D.HungarianMatcher()({"pred_logits": dl.double(), "pred_boxes": db}, [{"labels": torch.zeros(1, dtype=I64, device="cuda"), "boxes": bx[:1]}])
    with pytest.raises(RuntimeError, match="forward only"):
        D.generalized_box_iou(bx.clone().requires_grad_(True), bx)
    with torch.no_grad():
        D.generalized_box_iou(bx.clone().requires_grad_(True), bx)      # allowed: grad mode is off
    with pytest.raises(RuntimeError, match="8192"):
        D.nms(torch.rand(8193, 4, device="cuda"), torch.rand(8193, device="cuda"), 0.5)
    with pytest.raises(RuntimeError, match="K=1025"):
        D.PostProcess(1025)({"pred_logits": torch.zeros(1, 600, 4, device="cuda"), "pred_boxes": torch.zeros(1, 600, 4, device="cuda")}, torch.ones(1, 2, device="cuda"))
    with pytest.raises(RuntimeError, match="float32"):
        D.postprocess_launch(dl.half(), db, ds, s[:, :K], l[:, :K], b[:, :K])
