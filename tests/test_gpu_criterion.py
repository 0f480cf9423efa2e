"""The training criterion on the GPU (csrc/fvit_loss.hip through the C ABI, and fastervit_amd/criterion.py on top of it), held to tests/criterion_refs.py:
scalar sums to ``scalar_bar`` (8 x the fp32 error of the unreduced terms + a chain of 48 fp32 additions), gradients to ``bound`` / ``worst_ratio`` of
backward_primitive_refs, counts, hits and indices to torch.equal; tests/test_criterion_refs_cpu.py shows that the restatement equals the reference's own
SetCriterion and that wrong variants fail.

Conventions as in test_gpu_detection.py: every input is a view inside a larger NaN-filled (floats) / -1-filled (integers) buffer, every output starts as
NaN / -1 with a guard in front of and behind it that must survive.  Each value test prints its worst |err| / bar; 1.0 is the bar
(profiles/criterion_tests.log: a run on an MI355X)."""
import pytest
import torch

from fastervit_amd import HungarianMatcher, SetCriterion, _lib, sigmoid_focal_loss
from tests import criterion_refs as R

pytestmark = pytest.mark.gpu

F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32
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


def _scalar(name, got, exact_terms, plain_terms):
    r = R.scalar_ratio(got, exact_terms, plain_terms)
    print(f"{name}: |err|/bar = {r:.4f}")
    assert r <= 1.0, f"{name}: {r:.3f} x the bar (got {float(got)!r}, exact {exact_terms.sum().item()!r})"


def _elementwise(name, got, exact, plain32):
    assert got.dtype == F32
    r = R.worst_ratio(got.reshape(exact.shape), exact, plain32, F32)
    print(f"{name}: worst |err|/bound = {r:.4f}")
    assert r <= 1.0, f"{name}: {r:.3f} x the bar"


# ------------------------------------------------------------------------------------------------------------------------------------- label loss
def _label_abi(sets, C, g, alpha=R.FOCAL_ALPHA, gamma=2.0, dense=None):
    """sets: [(logits (B, Q, C), classes (B * Q,), scale)]; g: the incoming gradient per set.  Returns rc's, (loss, card, hits, grads), buffers."""
    lib, n = _lib.lib(), len(sets)
    stride = max(lg.shape[0] for lg, _, _ in sets)
    dl = [_embed(lg.reshape(-1, C)) for lg, _, _ in sets]
    dc = [_embed(cl, I32) for _, cl, _ in sets]
    dd = [_embed(d.reshape(-1, C)) if d is not None else None for d in (dense or [None] * n)]
    gr = [_guarded(tuple(d.shape), F32) for d in dl]
    table = (_lib.FvitDetLabelSet * n)(*[_lib.FvitDetLabelSet(logits=dl[s].data_ptr(), classes=dc[s].data_ptr(), targets=dd[s].data_ptr() if dd[s] is not None else None,
                                                              grad_logits=gr[s][0].data_ptr(), R=lg.shape[0] * lg.shape[1], Q=lg.shape[1], B=lg.shape[0], scale=sc)
                                         for s, (lg, _, sc) in enumerate(sets)])
    (loss, lb), (card, cb), (hits, hb) = _guarded((n,), F32), _guarded((n, stride), I32), _guarded((n,), I32)
    need = lib.fvit_det_label_loss_workspace(table, n, C)
    assert need > 0 and need % 16 == 0, lib.fvit_last_error()
    ws, wb = _guarded((need // 4,), F32)
    dg = _embed(torch.as_tensor(g, dtype=F32))
    rc1 = lib.fvit_det_label_loss(table, n, C, alpha, gamma, loss.data_ptr(), card.data_ptr(), stride, hits.data_ptr(), ws.data_ptr(), need, _stream())
    rc2 = lib.fvit_det_label_loss_backward(table, n, C, alpha, gamma, dg.data_ptr(), _stream())
    torch.cuda.synchronize()
    return (rc1, rc2), (loss, card, hits, [v for v, _ in gr]), [lb, cb, hb, wb] + [b for _, b in gr]


def _label_check(name, sets, C, g, **kw):
    (rc1, rc2), (loss, card, hits, grads), bufs = _label_abi(sets, C, g, **kw)
    assert (rc1, rc2) == (0, 0), _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    for s, (lg, cl, sc) in enumerate(sets):
        nb = 1.0 / sc
        refs = []
        for dt in (F64, F32):
            x = lg.to(dt).requires_grad_(True)
            ref = R.label_ref(x, cl, nb, dt, **kw)
            (gx,) = torch.autograd.grad(ref["terms"].sum() * g[s], x)
            refs.append((ref, gx))
        (ex, gex), (p32, g32) = refs
        B = lg.shape[0]
        _scalar(f"{name} set {s} loss", loss[s].item(), ex["terms"], p32["terms"])
        assert torch.equal(card[s, :B].cpu(), ex["card"]) and (card[s, B:] == -1).all(), f"{name} set {s}: cardinality"
        assert hits[s].item() == ex["hits"], f"{name} set {s}: hits {hits[s].item()} != {ex['hits']}"
        _elementwise(f"{name} set {s} grad", grads[s].cpu().view(lg.shape), gex, g32)
    return loss, card, hits, grads


@pytest.mark.parametrize("case", range(len(R.LABEL_CASES)), ids=["x".join(map(str, c)) for c in R.LABEL_CASES])
def test_label_loss_value_cases(case):
    logits, classes, nb = R.label_inputs(case)
    _label_check(f"label {R.LABEL_CASES[case]}", [(logits, classes, 1.0 / nb)], logits.shape[2], [1.0])


def test_label_loss_without_any_target():
    logits, classes, nb = R.label_inputs(R.LABEL_EMPTY_CASE, empty=True)
    assert nb == 1.0 and (classes == logits.shape[2]).all()
    _, _, hits, _ = _label_check("label no targets", [(logits, classes, 1.0)], logits.shape[2], [0.75])
    assert hits.item() == 0


@pytest.mark.parametrize("n_sets", R.LABEL_SET_COUNTS)
def test_label_loss_many_sets_of_different_sizes(n_sets):
    C = 31
    shapes = [(2, 33), (1, 65), (3, 7), (2, 1), (1, 130)]
    sets, g = [], []
    for s in range(n_sets):
        B, Q = shapes[s % len(shapes)]
        logits, classes, nb = R.label_draw(B, Q, C, [(3 * s + b) % 6 for b in range(B)], 8600 + s)
        sets.append((logits, classes, 1.0 / (nb * (1 + s % 3))))      # the denoising sets divide by num_boxes * groups
        g.append(0.5 + 0.25 * s)
    _label_check(f"label {n_sets} sets", sets, C, g)


@pytest.mark.parametrize("kw", [dict(gamma=1.0), dict(gamma=3.0, alpha=-1.0), dict(alpha=0.6)], ids=["gamma1", "gamma3_no_alpha", "alpha06"])
def test_label_loss_other_gamma_and_alpha(kw):
    logits, classes, nb = R.label_inputs(2)
    _label_check(f"label {kw}", [(logits, classes, 1.0 / nb)], logits.shape[2], [1.0], **kw)


def test_label_loss_saturated_logits_stay_finite():
    B, Q, C = 1, 6, 3
    logits = (200.0 * torch.eye(3)[[0, 1, 2, 0, 1, 2]] - 100.0).view(B, Q, C)      # one +100 per row: every (sign, target) combination, a unique maximum
    classes = torch.tensor([0, 0, 3, 2, 1, 3])
    loss, _, _, grads = _label_check("label +-100", [(logits, classes, 0.25)], C, [1.0])
    assert torch.isfinite(loss).all() and torch.isfinite(grads[0]).all()


def test_label_loss_bad_class_id_gives_nan_and_stays_in_bounds():
    a, b = R.label_inputs(1), R.label_inputs(1, seed=1)
    for bad in (-1, 6, 1 << 20):
        cl = a[1].clone()
        cl[4] = bad
        (rc1, rc2), (loss, card, hits, grads), bufs = _label_abi([(a[0], cl, 1.0), (b[0], b[1], 1.0)], 5, [1.0, 1.0])
        assert (rc1, rc2) == (0, 0)
        _guards_intact(*bufs)
        assert torch.isnan(loss[0]) and torch.isfinite(loss[1]), "only the set with the bad id is NaN"
        assert torch.isnan(grads[0].view(14, 5)[4]).all() and torch.isfinite(grads[1]).all()
        ex = R.label_ref(b[0], b[1], 1.0, F64)
        assert torch.equal(card[1].cpu(), ex["card"]) and hits[1].item() == ex["hits"]


# --------------------------------------------------------------------------------------------------------------------------------------- box loss
G_BOX = [0.5, 0.25, 2.0, 5.0]      # incoming gradients of (loss_xy, loss_hw, loss_giou, loss_bbox)


def _box_abi(sets, g):
    """sets: [(src (M, 4), tgt (M, 4), scale)]; g: (n, 4) incoming gradients."""
    lib, n = _lib.lib(), len(sets)
    ds, dt_ = [_embed(s) for s, _, _ in sets], [_embed(t) for _, t, _ in sets]
    gr = [_guarded((s.shape[0], 4), F32) for s, _, _ in sets]
    table = (_lib.FvitDetBoxSet * n)(*[_lib.FvitDetBoxSet(src=ds[k].data_ptr(), tgt=dt_[k].data_ptr(), grad_src=gr[k][0].data_ptr(), M=s.shape[0], scale=sc)
                                       for k, (s, _, sc) in enumerate(sets)])
    out, ob = _guarded((n, 4), F32)
    dg = _embed(torch.as_tensor(g, dtype=F32))
    rc1 = lib.fvit_det_box_loss(table, n, out.data_ptr(), _stream())
    rc2 = lib.fvit_det_box_loss_backward(table, n, dg.data_ptr(), _stream())
    torch.cuda.synchronize()
    return (rc1, rc2), out, [v for v, _ in gr], [ob] + [b for _, b in gr]


def _box_refs(src, tgt, nb, g):
    res = []
    for dt in (F64, F32):
        s = src.to(dt).requires_grad_(True)
        ref = R.box_ref(s, tgt, nb, dt)
        l1 = ref["loss_bbox"]
        tot = g[0] * l1[:, :2].sum() + g[1] * l1[:, 2:].sum() + g[2] * ref["loss_giou"].sum() + g[3] * l1.sum()
        res.append((ref, torch.autograd.grad(tot, s)[0] if src.shape[0] else torch.zeros_like(s)))
    return res


def _box_check(name, sets, g):
    (rc1, rc2), out, grads, bufs = _box_abi(sets, g)
    assert (rc1, rc2) == (0, 0), _lib.lib().fvit_last_error()
    _guards_intact(*bufs)
    for k, (src, tgt, sc) in enumerate(sets):
        (ex, gex), (p32, g32) = _box_refs(src, tgt, 1.0 / sc, g[k])
        for col, key in enumerate(("loss_xy", "loss_hw", "loss_giou", "loss_bbox")):
            if src.shape[0] == 0:
                assert out[k, col].item() == 0.0
            else:
                _scalar(f"{name} set {k} {key}", out[k, col].item(), ex[key], p32[key])
        if src.shape[0]:
            _elementwise(f"{name} set {k} grad", grads[k].cpu(), gex, g32)
    return out, grads


@pytest.mark.parametrize("M", [m for m in R.BOX_M if m] + ["small"])
def test_box_loss_value_cases(M):
    src, tgt = R.box_inputs(R.BOX_SMALL_M, small=True) if M == "small" else R.box_inputs(M)
    _box_check(f"box M={M}", [(src, tgt, 1.0 / 3.0)], [G_BOX])


def test_box_loss_all_sizes_in_one_launch_and_no_pairs_at_all():
    sets = [(*R.box_inputs(M, seed=1), 1.0 / (2 + k)) for k, M in enumerate(R.BOX_M)] * 2 + [(*R.box_inputs(0), 1.0)]
    assert len(sets) == 13 and sets[0][0].shape[0] == 0
    _box_check("box 13 sets", sets, [[g * (1 + 0.1 * k) for g in G_BOX] for k in range(13)])
    (rc1, rc2), out, _, bufs = _box_abi([(*R.box_inputs(0), 1.0)] * 2, [G_BOX] * 2)      # M = 0 in every set: no launch, nothing written
    assert (rc1, rc2) == (0, 0)
    _untouched(*bufs)


def test_box_loss_exact_cases():
    box = torch.tensor([[0.4, 0.5, 0.2, 0.3], [0.6, 0.3, 0.1, 0.1], [0.5, 0.5, 0.25, 0.125]])
    # identical boxes: the L1 sums are exactly 0 and so is their gradient (sign(0) = 0); the GIoU part is finite
    (rc1, rc2), out, grads, bufs = _box_abi([(box, box.clone(), 1.0)], [[0.5, 0.25, 0.0, 5.0]])
    assert (rc1, rc2) == (0, 0)
    _guards_intact(*bufs)
    assert out[0, 0].item() == 0.0 and out[0, 1].item() == 0.0 and out[0, 3].item() == 0.0 and torch.isfinite(out[0, 2])
    assert abs(out[0, 2].item()) < 1e-3, "1 - GIoU of a box with itself is 1e-6 / area"
    assert (grads[0] == 0).all(), "the L1 gradient at src == tgt must be exactly 0"
    (rc1, rc2), out, grads, _ = _box_abi([(box, box.clone(), 1.0)], [G_BOX])
    assert (rc1, rc2) == (0, 0) and torch.isfinite(out).all() and torch.isfinite(grads[0]).all()
    # zero-area boxes, on top of each other and apart
    flat = torch.tensor([[0.4, 0.5, 0.0, 0.0], [0.6, 0.3, 0.0, 0.2], [0.5, 0.5, 0.0, 0.0]])
    other = torch.tensor([[0.4, 0.5, 0.0, 0.0], [0.2, 0.3, 0.1, 0.0], [0.1, 0.7, 0.0, 0.0]])
    (rc1, rc2), out, grads, bufs = _box_abi([(flat, other, 0.5)], [G_BOX])
    assert (rc1, rc2) == (0, 0) and torch.isfinite(out).all() and torch.isfinite(grads[0]).all()
    _guards_intact(*bufs)


def test_all_four_entry_points_captured_once_and_replayed_with_new_inputs():
    """No allocation, no host read: label and box loss, forward and backward, sit in one captured graph; a replay follows the new logits and boxes."""
    lib = _lib.lib()
    B, Q, C, M = 2, 33, 31, 65
    _, classes, nb = R.label_draw(B, Q, C, [5, 9], 8800)
    dl, dc = _embed(torch.zeros(B * Q, C)), _embed(classes, I32)
    ds, dt_ = _embed(torch.zeros(M, 4)), _embed(R.box_inputs(M)[1])
    (gl, glb), (gs, gsb), (loss, lb), (card, cb), (hits, hb), (out, ob) = (_guarded((B * Q, C), F32), _guarded((M, 4), F32), _guarded((1,), F32),
                                                                           _guarded((1, B), I32), _guarded((1,), I32), _guarded((1, 4), F32))
    lt = (_lib.FvitDetLabelSet * 1)(_lib.FvitDetLabelSet(logits=dl.data_ptr(), classes=dc.data_ptr(), targets=None, grad_logits=gl.data_ptr(), R=B * Q, Q=Q, B=B,
                                                         scale=1.0 / nb))
    bt = (_lib.FvitDetBoxSet * 1)(_lib.FvitDetBoxSet(src=ds.data_ptr(), tgt=dt_.data_ptr(), grad_src=gs.data_ptr(), M=M, scale=1.0 / nb))
    need = lib.fvit_det_label_loss_workspace(lt, 1, C)
    ws, wb = _guarded((need // 4,), F32)
    g_lab, g_box = _embed(torch.tensor([0.75])), _embed(torch.tensor([G_BOX]))

    def launch():
        rcs = (lib.fvit_det_label_loss(lt, 1, C, R.FOCAL_ALPHA, 2.0, loss.data_ptr(), card.data_ptr(), B, hits.data_ptr(), ws.data_ptr(), need, _stream()),
               lib.fvit_det_label_loss_backward(lt, 1, C, R.FOCAL_ALPHA, 2.0, g_lab.data_ptr(), _stream()),
               lib.fvit_det_box_loss(bt, 1, out.data_ptr(), _stream()), lib.fvit_det_box_loss_backward(bt, 1, g_box.data_ptr(), _stream()))
        assert rcs == (0, 0, 0, 0), lib.fvit_last_error()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for seed in range(2):
        logits = R.label_draw(B, Q, C, [5, 9], 8810 + seed)[0]
        src = R.box_inputs(M, seed=2 + seed)[0]
        dl.copy_(logits.reshape(-1, C))
        ds.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (loss, card, hits, out, gl, gs)]
        launch()
        torch.cuda.synchronize()
        _guards_intact(glb, gsb, lb, cb, hb, ob, wb)
        assert all(torch.equal(a, b) for a, b in zip(replayed, (loss, card, hits, out, gl, gs))), "a replay and a plain launch differ"
        ex, p32 = R.label_ref(logits, classes, nb, F64), R.label_ref(logits, classes, nb, F32)
        _scalar(f"replay {seed} loss", replayed[0].item(), ex["terms"], p32["terms"])
        assert torch.equal(replayed[1][0].cpu(), ex["card"]) and replayed[2].item() == ex["hits"]


def test_abi_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    logits, classes, _ = R.label_inputs(1)
    dl, dc = _embed(logits.reshape(-1, 5)), _embed(classes, I32)
    (gr, gb), (loss, lb), (card, cb), (hits, hb), (ws, wb) = _guarded((14, 5), F32), _guarded((17,), F32), _guarded((17, 2), I32), _guarded((17,), I32), _guarded((256,), F32)
    mk = lambda n, **k: (_lib.FvitDetLabelSet * n)(*[_lib.FvitDetLabelSet(**{**dict(logits=dl.data_ptr(), classes=dc.data_ptr(), targets=None,
                                                                                     grad_logits=gr.data_ptr(), R=14, Q=7, B=2, scale=1.0), **k}) for _ in range(n)])
    fwd = lambda t, n, C=5, stride=2, nbytes=1024: lib.fvit_det_label_loss(t, n, C, 0.25, 2.0, loss.data_ptr(), card.data_ptr(), stride, hits.data_ptr(),
                                                                              ws.data_ptr(), nbytes, _stream())
    bwd = lambda t, n, C=5: lib.fvit_det_label_loss_backward(t, n, C, 0.25, 2.0, loss.data_ptr(), _stream())
    for call, word in ((lambda: fwd(mk(1), 0), b"n_sets=0"), (lambda: fwd(mk(17), 17), b"n_sets=17"), (lambda: bwd(mk(17), 17), b"n_sets=17"),
                       (lambda: fwd(mk(1), 1, C=0), b"C=0"), (lambda: fwd(mk(1, R=1 << 27, Q=1 << 26), 1, C=16), b"2^31"),
                       (lambda: fwd(mk(1, logits=dl.data_ptr() + 2), 1), b"misaligned"), (lambda: bwd(mk(1, grad_logits=gr.data_ptr() + 1), 1), b"misaligned"),
                       (lambda: fwd(mk(1), 1, stride=1), b"card_stride"), (lambda: fwd(mk(1), 1, nbytes=16), b"workspace")):
        rc = call()
        assert rc < 0 and word in lib.fvit_last_error(), (rc, word, lib.fvit_last_error())
    src, (out, ob), (gs, gsb) = _embed(R.box_inputs(3)[0]), _guarded((17, 4), F32), _guarded((3, 4), F32)
    bx = lambda n, **k: (_lib.FvitDetBoxSet * n)(*[_lib.FvitDetBoxSet(**{**dict(src=src.data_ptr(), tgt=src.data_ptr(), grad_src=gs.data_ptr(), M=3, scale=1.0), **k})
                                                   for _ in range(n)])
    for call, word in ((lambda: lib.fvit_det_box_loss(bx(17), 17, out.data_ptr(), _stream()), b"n_sets=17"),
                       (lambda: lib.fvit_det_box_loss(bx(1, M=-2), 1, out.data_ptr(), _stream()), b"M=-2"),
                       (lambda: lib.fvit_det_box_loss(bx(1, src=src.data_ptr() + 4), 1, out.data_ptr(), _stream()), b"16-byte"),
                       (lambda: lib.fvit_det_box_loss_backward(bx(1, grad_src=gs.data_ptr() + 8), 1, out.data_ptr(), _stream()), b"16-byte"),
                       (lambda: lib.fvit_det_box_loss_backward(bx(1), 0, out.data_ptr(), _stream()), b"n_sets=0")):
        rc = call()
        assert rc == -1 and word in lib.fvit_last_error(), (rc, word, lib.fvit_last_error())
    torch.cuda.synchronize()
    _untouched(gb, lb, cb, hb, wb, ob, gsb)


# ---------------------------------------------------------------------------------------------------------------------------------- Python layer
def _cuda_case(case, dtype=F32):
    outputs, targets, indices = R.forward_inputs(case)
    dev = R.convert(outputs, lambda v: v.to(dtype).cuda().requires_grad_(True))
    tg = R.convert_targets(targets, lambda v: (v.to(dtype) if v.is_floating_point() else v).cuda())
    return outputs, targets, indices, dev, tg


_refs = {}


def _case_refs(case):
    """exact and plain32 (terms, scalars, grads) of a forward case from the restatement, computed once and shared."""
    if case not in _refs:
        c = R.FORWARD_CASES[case]
        outputs, targets, indices = R.forward_inputs(case)
        weights = R.weight_dict(c["aux"], c["interm"])
        res = []
        for dt in (F64, F32):
            o = R.convert(outputs, lambda v: v.to(dt).requires_grad_(True))
            terms, scalars = R.criterion(o, targets, indices, dt)
            leaves = [s[k] for _, s in R.pred_sets(o) for k in ("pred_logits", "pred_boxes")]
            grads = torch.autograd.grad(R.total(terms, weights), leaves, allow_unused=True)
            res.append((terms, scalars, [g if g is not None else torch.zeros_like(l) for g, l in zip(grads, leaves)]))
        _refs[case] = res
    return _refs[case]


def _criterion(case, matcher=None):
    c = R.FORWARD_CASES[case]
    return SetCriterion(c["C"], matcher or HungarianMatcher(**R.MATCH_WEIGHTS), R.weight_dict(c["aux"], c["interm"]), R.FOCAL_ALPHA, list(R.LOSSES))


def _check_losses(name, losses, golden, case):
    (terms, scalars, _), (terms32, _, _) = _case_refs(case)
    assert sorted(losses) == golden[f"{name}_keys"], "the key set differs from the reference's"
    for k, v in losses.items():
        assert v.dim() == 0 and v.is_cuda
        want = golden[f"{name}_loss_{k}"].item()
        if k in terms:
            assert abs(terms[k].sum().item() - want) <= 1e-9 * max(abs(want), 1e-3)
            _scalar(f"forward {name} {k}", v.item(), terms[k], terms32[k])
        else:
            assert abs(v.item() - want) <= R.COUNT_RTOL * abs(want), (k, v.item(), want)


@pytest.mark.parametrize("case", range(len(R.FORWARD_CASES)), ids=[c["name"] for c in R.FORWARD_CASES])
def test_set_criterion_forward_and_backward_on_the_golden_cases(case):
    golden = R.load_golden()
    c = R.FORWARD_CASES[case]
    name = c["name"]
    outputs, targets, indices, dev, tg = _cuda_case(case)
    crit = _criterion(case)
    _lib.prof_enable(True)
    losses, ind_list = crit(dev, tg, return_indices=True)
    torch.cuda.synchronize()
    launches = [r["name"] for r in _lib.prof_records()]
    _lib.prof_enable(False)
    n_sets = len(R.pred_sets(outputs))
    assert launches.count("label_loss_kernel") == -(-n_sets // 16) and launches.count("label_finish_kernel") == -(-n_sets // 16)
    assert launches.count("box_loss_kernel") == (-(-n_sets // 16) if sum(c["nt"]) else 0)
    _check_losses(name, losses, golden, case)
    got_ind = [ind_list[-1]] + ind_list[:-1]
    assert len(got_ind) == len(indices)
    for s, ind in enumerate(got_ind):
        for b, (i, j) in enumerate(ind):
            assert torch.equal(i.cpu(), golden[f"{name}_idx{s}_{b}_src"]) and torch.equal(j.cpu(), golden[f"{name}_idx{s}_{b}_tgt"])
    weights = crit.weight_dict
    total = sum(losses[k] * weights[k] for k in losses if k in weights)
    total.backward()
    (_, _, gex), (_, _, g32) = _case_refs(case)
    leaves = [(s, k, o[k]) for s, o in R.pred_sets(dev) for k in ("pred_logits", "pred_boxes")]
    for (s, k, leaf), ge, gp in zip(leaves, gex, g32):
        want = golden[f"{name}_grad_{s}_{k[5:]}"]
        assert (ge - want).abs().max().item() <= 1e-9 * max(want.abs().max().item(), 1e-3)
        got = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        _elementwise(f"forward {name} d{s}.{k}", got.cpu(), want, gp)
    # eval mode: the denoising sets are not used, their keys are zero
    if c["dn"]:
        ev = crit.eval()(dev, tg)
        assert sorted(ev) == sorted(losses) and all(ev[k].item() == 0.0 for k in ev if "_dn" in k)
        assert ev["loss_ce"].item() == losses["loss_ce"].item()


def test_each_loss_method_given_the_golden_indices():
    golden = R.load_golden()
    case = 1
    name = R.FORWARD_CASES[case]["name"]
    outputs, targets, indices, dev, tg = _cuda_case(case)
    crit = _criterion(case)
    nb = float(sum(R.FORWARD_CASES[case]["nt"]))
    ind = [(golden[f"{name}_idx0_{b}_src"], golden[f"{name}_idx0_{b}_tgt"]) for b in range(2)]
    got = {}
    got.update(crit.loss_labels(dev, tg, ind, nb))
    got.update(crit.loss_boxes(dev, tg, ind, nb))
    got.update(crit.loss_cardinality(dev, tg, ind, nb))
    got2 = {}
    for loss in R.LOSSES:
        got2.update(crit.get_loss(loss, dev, tg, ind, nb))
    assert sorted(got) == ["cardinality_error", "class_error", "loss_bbox", "loss_ce", "loss_giou", "loss_hw", "loss_xy"]
    assert all(torch.equal(got[k], got2[k]) for k in got)
    (terms, _, _), (terms32, _, _) = _case_refs(case)
    for k, v in got.items():
        if k in terms:
            _scalar(f"method {k}", v.item(), terms[k], terms32[k])
        else:
            want = golden[f"{name}_loss_{k}"].item()
            assert abs(v.item() - want) <= R.COUNT_RTOL * abs(want), (k, v.item(), want)
    assert got["loss_ce"].requires_grad and got["loss_bbox"].requires_grad and got["loss_giou"].requires_grad
    assert not got["loss_xy"].requires_grad and not got["loss_hw"].requires_grad and not got["cardinality_error"].requires_grad
    assert "class_error" not in crit.loss_labels(dev, tg, ind, nb, log=False)


@pytest.mark.parametrize("case", [1, 2, 5], ids=["2x7x5", "2x33x31", "2x900x91"])
def test_sigmoid_focal_loss_on_dense_targets(case):
    golden = R.load_golden()
    logits, classes, nb = R.label_inputs(case)
    B, Q, C = logits.shape
    t = R.onehot(classes, C, F32).view(B, Q, C)
    t[0, 0] = 1.0                                     # dense targets need not be one-hot: a row of ones, which no class map can express
    x = logits.cuda().requires_grad_(True)
    got = sigmoid_focal_loss(x, t.cuda(), nb, alpha=R.FOCAL_ALPHA, gamma=2)
    got.backward()
    refs = []
    for dt in (F64, F32):
        xr = logits.to(dt).requires_grad_(True)
        terms = R.focal_terms(xr, t, dt) / (Q * nb)
        refs.append((terms, torch.autograd.grad(terms.sum(), xr)[0]))
    _scalar(f"sigmoid_focal_loss {case}", got.item(), refs[0][0], refs[1][0])
    _elementwise(f"sigmoid_focal_loss {case} grad", x.grad.cpu(), refs[0][1], refs[1][1])
    one_hot = sigmoid_focal_loss(logits.cuda(), R.onehot(classes, C, F32).view(B, Q, C).cuda(), nb)
    ex, p32 = R.label_ref(logits, classes, nb, F64)["terms"] / Q, R.label_ref(logits, classes, nb, F32)["terms"] / Q
    assert abs(ex.sum().item() - golden[f"focal{case}"].item()) <= 1e-12 * golden[f"focal{case}"].item()
    _scalar(f"sigmoid_focal_loss {case} one-hot vs the reference", one_hot.item(), ex, p32)
    with pytest.raises(RuntimeError, match="0 and 1"):
        sigmoid_focal_loss(logits.cuda(), (0.5 * t).cuda(), nb)


class _PlainMatcher:
    """A matcher object without cost_matrix: SetCriterion calls it per set, as the reference does."""

    def __init__(self):
        self.inner, self.calls = HungarianMatcher(**R.MATCH_WEIGHTS), 0

    def __call__(self, outputs, targets):
        self.calls += 1
        return self.inner(outputs, targets)


def test_one_copy_matching_equals_a_plain_matcher_and_backward_repeats_bitwise():
    case = 2
    _, _, _, dev, tg = _cuda_case(case)
    plain = _PlainMatcher()
    a, b = _criterion(case)(dev, tg), _criterion(case, plain)(dev, tg)
    assert plain.calls == 4 and sorted(a) == sorted(b)          # main, 2 aux, interm
    assert all(torch.equal(a[k], b[k]) for k in a)
    weights = R.weight_dict(2, True)
    leaves = [o[k] for _, o in R.pred_sets(dev) for k in ("pred_logits", "pred_boxes")]
    runs = []
    for _ in range(2):
        losses = _criterion(case)(dev, tg)
        runs.append((losses, torch.autograd.grad(sum(losses[k] * weights[k] for k in losses if k in weights), leaves)))
    assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in a) and all(torch.equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_inputs_give_gradients_in_their_dtype(dt):
    case = 2
    outputs, targets, _, dev, tg = _cuda_case(case, dt)
    losses = _criterion(case)(dev, tg)
    weights = R.weight_dict(2, True)
    sum(losses[k] * weights[k] for k in losses if k in weights).backward()
    # the same rounded inputs in fp32: same indices expected only when the 16-bit cost matrix keeps the assignment, so compare the denoising part,
    # whose indices are fixed, and the dtypes of everything
    wide = R.convert(dev, lambda v: v.detach().float().requires_grad_(True))
    ref = _criterion(case)(wide, R.convert_targets(tg, lambda v: v.float() if v.is_floating_point() else v))
    sum(ref[k] * weights[k] for k in ref if k in weights).backward()
    for (name, o), (_, w) in zip(R.pred_sets(dev), R.pred_sets(wide)):
        for k in ("pred_logits", "pred_boxes"):
            assert o[k].grad is not None and o[k].grad.dtype == dt and o[k].grad.shape == o[k].shape
            if name.startswith("dn"):
                assert torch.equal(o[k].grad, w[k].grad.to(dt)), "a 16-bit input is widened once, computed in fp32 and its gradient narrowed once"
    for k in ref:
        assert losses[k].dtype == F32
        if "_dn" in k:
            assert torch.equal(losses[k], ref[k])


def test_python_refusals():
    case = 0
    _, _, indices, dev, tg = _cuda_case(case)
    crit = _criterion(case)
    with pytest.raises(RuntimeError, match="float64"):
        crit(R.convert(dev, lambda v: v.detach().double()), tg)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit(R.convert(dev, lambda v: v.detach().cpu()), tg)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.loss_labels(dev, R.convert_targets(tg, lambda v: v.cpu()), indices[0], 2.0)
    with pytest.raises(NotImplementedError, match="masks"):
        crit.get_loss("masks", dev, tg, indices[0], 2.0)
    with pytest.raises(RuntimeError, match="float64"):
        sigmoid_focal_loss(dev["pred_logits"].double(), dev["pred_logits"].double(), 1.0)
