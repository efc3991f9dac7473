"""GPU: the training criterion's fused route (csrc/criterion.hip: dfx_match_cost_f32, dfx_set_loss_forward_f32,
dfx_set_loss_backward_f32, assignment on the host) on the cases of tests/_criterion_cases.py against the reference's own fp64
results, within the project's yardstick rule: per output, error relative to the reference's largest magnitude (absolute where
the reference is identically zero) at most YARDSTICK_FACTOR x the error of the reference's own fp32 run.  The two
integer-valued outputs, class_error and cardinality_error, are instead equal to the reference to 1e-6, measured the same
way (relative to the reference's magnitude: 100 - 100 * 1 / 3 has no exact fp32 value).

Below those, the hand-built families of tests/_criterion_cases.py straight on dfx.ops.set_loss_forward / set_loss_backward /
match_cost against this project's torch formulation in fp64 on the CPU (which tests/test_criterion_cpu.py pins to the
reference within 1e-10), and the contracts of include/dfx_criterion.h at the entries and on the route."""
import numpy as np
import pytest
import torch

from tests import _criterion_cases as cc

pytestmark = pytest.mark.gpu

CASES = list(cc.CASES)


def _criterion(name):
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    return SetCriterion(cc.NUM_CLASSES, HungarianMatcher(**cc.COST), cc.weight_dict(cc.CASES[name]), cc.LOSSES)


def _run(name, monkeypatch=None, expect_fused=True):
    """-> (losses, grads, {set: assignment} of the fused route | None): one forward + backward on cuda in fp32"""
    inputs, _, _ = cc.prepared(name)
    crit = _criterion(name)
    seen = []
    inner = crit.assign

    def recording(*a):
        res = inner(*a)
        seen.append(res[2].clone())
        return res

    crit.assign = recording
    losses, grads = cc.run(name, inputs, crit, torch.float32, "cuda")
    torch.cuda.synchronize()
    assert len(seen) == (1 if expect_fused else 0), "one assignment round trip per criterion call on the fused route, none on the torch route"
    return losses, grads, (cc.row_target_to_assignments(name, seen[0].numpy()) if seen else None)


def _compare(name, losses, grads):
    _, ref, yard = cc.prepared(name)
    assert list(losses) == ref["keys"]
    worst = []
    for k, got in [(f"loss.{k}", v) for k, v in losses.items()] + list(grads.items()):
        assert got.shape == ref[k].shape and got.dtype == torch.float32, k
        if k.startswith(("loss.class_error", "loss.cardinality_error")):
            err = cc.rel_err(got, ref[k])
            print(f"  {name} {k}: {got.item():.6f} against {ref[k].item():.6f}")
            if not err <= 1e-6:
                worst.append(f"{k}: {got.item()} against {ref[k].item()}")
            continue
        y, err = cc.rel_err(yard[k], ref[k]), cc.rel_err(got, ref[k])
        print(f"  {name} {k}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, max |ref| {ref[k].abs().max().item() if ref[k].numel() else 0:.3e}")
        if not err <= cc.YARDSTICK_FACTOR * y:
            worst.append(f"{k}: gpu {err:.3e} against {cc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


def _exact_zeros(name, grads):
    """column 0 of every logit gradient; box gradients of unmatched rows"""
    _, ref, _ = cc.prepared(name)
    for n in cc.set_names(cc.CASES[name]):
        assert (grads[f"grad.{n}.logits"][..., 0] == 0).all(), n
        unmatched = torch.ones(grads[f"grad.{n}.boxes"].shape[:2], dtype=torch.bool)
        for b, q, _ in ref[f"assign.{n}"].tolist():
            unmatched[b, q] = False
        assert (grads[f"grad.{n}.boxes"][unmatched] == 0).all(), n
        assert (grads[f"grad.{n}.boxes"][~unmatched] != 0).any() or unmatched.all(), n


@pytest.mark.parametrize("name", CASES)
def test_fused_route_matches_the_reference_within_the_yardstick(name):
    _, ref, _ = cc.prepared(name)
    losses, grads, assign = _run(name)
    for n, a in assign.items():
        assert np.array_equal(a, ref[f"assign.{n}"].numpy()), n
    _compare(name, losses, grads)
    _exact_zeros(name, grads)
    assert all(torch.isfinite(v).all() for v in grads.values())


@pytest.mark.parametrize("name", CASES)
def test_matcher_alone_returns_the_stored_assignments(name):
    inputs, ref, _ = cc.prepared(name)
    for n, a in cc.assignments(name, inputs, _criterion(name).matcher, torch.float32, "cuda").items():
        assert np.array_equal(a, ref[f"assign.{n}"].numpy()), n


@pytest.mark.parametrize("name", ["ragged", "enc", "stride"])
def test_two_calls_give_the_same_bits(name):
    """No atomics, every sum in an order fixed by the shapes; outputs come from ``empty``."""
    la, ga, _ = _run(name)
    junk = torch.full((1 << 20,), float("nan"), device="cuda")      # what the next ``empty`` may hand out
    del junk
    lb, gb, _ = _run(name)
    for k in la:
        assert torch.equal(la[k], lb[k]) and torch.isfinite(lb[k]).all(), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]) and torch.isfinite(gb[k]).all(), k


def _flat_operands(name):
    """the operands of the kernels as the criterion lays them out, with the reference's stored assignment as row_target"""
    from dfx import ops
    from models.matcher import target_tensors
    case = cc.CASES[name]
    inputs, ref, _ = cc.prepared(name)
    outputs, tg, leaves = cc.build_outputs(name, inputs, torch.float32, "cuda")
    names = cc.set_names(case)
    logits = torch.cat([leaves[n][0].detach().reshape(-1, 3) for n in names])
    boxes = torch.cat([leaves[n][1].detach().reshape(-1, 4) for n in names])
    labels, tboxes, counts = target_tensors(tg, logits.device)
    desc, dims = ops.criterion_layout([leaves[n][0].shape[1] for n in names], [n == "enc" for n in names], counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    rt = torch.full((dims[2],), -1, dtype=torch.int32)
    for s, n in enumerate(names):
        for b, q, t in ref[f"assign.{n}"].tolist():
            rt[desc[3 * s + 1] + b * desc[3 * s] + q] = int(off[b]) + t
    return logits, boxes, labels, tboxes, rt.cuda(), torch.tensor(desc, dtype=torch.int32).cuda(), dims, desc


@pytest.mark.parametrize("name", ["ragged", "empty"])
def test_backward_null_outputs_keep_the_bits(name):
    from dfx import ops
    logits, boxes, labels, tboxes, rt, desc, dims, _ = _flat_operands(name)
    go = torch.randn(dims[0], 5, generator=torch.Generator().manual_seed(1)).cuda()
    inv = 1.0 / max(sum(cc.CASES[name]["targets"]), 1)
    full = ops.set_loss_backward(go, logits, boxes, labels, tboxes, rt, desc, dims, inv)
    assert all(torch.isfinite(t).all() for t in full)
    for need in ((True, False), (False, True), (False, False)):
        got = ops.set_loss_backward(go, logits, boxes, labels, tboxes, rt, desc, dims, inv, need_logits=need[0], need_boxes=need[1])
        for g, f, asked in zip(got, full, need):
            assert (g is not None) == asked and (not asked or torch.equal(g, f)), need
    # columns 1 and 4 of grad_out are not read: NaN there changes nothing
    go2 = go.clone()
    go2[:, 1] = float("nan")
    go2[:, 4] = float("nan")
    again = ops.set_loss_backward(go2, logits, boxes, labels, tboxes, rt, desc, dims, inv)
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])


@pytest.mark.parametrize("name", ["ragged", "recipe", "stride", "images"])
def test_match_cost_blocks_equal_the_torch_formulation(name):
    """every (set, image) block of the case at its documented offset, against the op-by-op cost matrix in fp64: fp32
    arithmetic on costs of order 1 to 10 - 1e-5 absolute is 20 ulp of the largest cost.  A set whose descriptor says "labels
    all zero" (enc_outputs) is compared with the cost matrix of zeroed labels, as the criterion matches it."""
    from dfx import ops
    from models.matcher import HungarianMatcher
    logits, boxes, labels, tboxes, _, desc, dims, d = _flat_operands(name)
    m = HungarianMatcher(**cc.COST)
    cost = ops.match_cost(logits, boxes, labels, tboxes, desc, dims, m.cost_class, m.cost_bbox, m.cost_giou).cpu()
    S, B, rows, Ttot = dims
    assert cost.numel() == (rows // B) * Ttot and torch.isfinite(cost).all()
    off, base, worst = d[3 * S:], 0, 0.0
    for s in range(S):
        Q, row0 = d[3 * s], d[3 * s + 1]
        lg = logits[row0:row0 + B * Q].view(B, Q, 3).double().cpu()
        bx = boxes[row0:row0 + B * Q].view(B, Q, 4).double().cpu()
        ids = labels.long().cpu() * (1 - d[3 * s + 2])          # the enc set of ``recipe`` is matched against zeroed labels
        want = m.cost_matrix(lg, bx, ids, tboxes.double().cpu()).view(B, Q, Ttot)
        for b in range(B):
            got = cost[base + Q * off[b]:base + Q * off[b + 1]].view(Q, off[b + 1] - off[b])
            err = (got.double() - want[b][:, off[b]:off[b + 1]]).abs().max().item() if got.numel() else 0.0
            worst = max(worst, err)
            assert err <= 1e-5, (s, b, err)
        base += Q * Ttot
    print(f"  {name} match_cost: worst block {worst:.3e} against 1e-5, max |cost| {cost.abs().max().item():.3e}")


@pytest.mark.parametrize("name", CASES)
def test_torch_route_on_the_gpu_meets_the_same_bounds(name, monkeypatch):
    """DFX_CRITERION=0: the op-by-op route serves cuda tensors"""
    monkeypatch.setenv("DFX_CRITERION", "0")
    _, ref, _ = cc.prepared(name)
    inputs = cc.prepared(name)[0]
    for n, a in cc.assignments(name, inputs, _criterion(name).matcher, torch.float32, "cuda").items():
        assert np.array_equal(a, ref[f"assign.{n}"].numpy()), n
    losses, grads, _ = _run(name, expect_fused=False)
    _compare(name, losses, grads)


def test_fused_route_refuses_graph_capture(monkeypatch):
    """the documented error, before any capture-time call (nothing is captured here: the query is monkeypatched)"""
    from dfx import ops
    name = "one"
    inputs, _, _ = cc.prepared(name)
    crit = _criterion(name)
    outputs, tg, _ = cc.build_outputs(name, inputs, torch.float32, "cuda")
    torch.cuda.synchronize()

    def forbidden(*a, **k):
        raise AssertionError("a library call was made under capture")

    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for entry in ("match_cost", "set_loss_forward", "lsap_ragged", "lsap"):
        monkeypatch.setattr(ops, entry, forbidden)
    with pytest.raises(RuntimeError, match="graph capture"):
        crit(outputs, tg)
    with pytest.raises(RuntimeError, match="graph capture"):
        crit.matcher(outputs, tg)


# ---- hand-built families straight on the kernels (tests/_criterion_cases.py) ------------------------------------------
def _operands(sets, targets, indices=None, zero=None):
    """``sets``: [(logits [B,Q,3], boxes [B,Q,4])] fp64 on the CPU, ``targets``: [(labels, boxes)] per image, ``indices``:
    per set, per image (rows, cols) | None -> the kernels' operands in fp32 on cuda, as the criterion lays them out"""
    from dfx import ops
    B = sets[0][0].shape[0]
    counts = [len(l) for l, _ in targets]
    logits = torch.cat([lg.float().reshape(-1, 3) for lg, _ in sets]).cuda()
    boxes = torch.cat([bx.float().reshape(-1, 4) for _, bx in sets]).cuda()
    labels = torch.cat([l for l, _ in targets]).to(torch.int32).cuda()
    tboxes = torch.cat([b for _, b in targets]).float().reshape(-1, 4).cuda()
    desc, dims = ops.criterion_layout([lg.shape[1] for lg, _ in sets], zero or [False] * len(sets), counts)
    off = desc[3 * len(sets):]
    rt = torch.full((dims[2],), -1, dtype=torch.int32)
    for s, per_image in enumerate(indices or []):
        Q, row0 = desc[3 * s], desc[3 * s + 1]
        for b, (ii, jj) in enumerate(per_image):
            for i, j in zip(ii.tolist(), jj.tolist()):
                rt[row0 + b * Q + i] = off[b] + j
    return logits, boxes, labels, tboxes, rt.cuda(), torch.tensor(desc, dtype=torch.int32).cuda(), dims, desc


def _family_run(fam, row_target=None):
    """forward + backward of the one-set family on the kernels -> (out [5], grad_logits [B,Q,3], grad_boxes [B,Q,4], the
    row_target used) on the cpu"""
    from dfx import ops
    logits, boxes, labels, tboxes, rt, desc, dims, _ = _operands([(fam["logits"], fam["boxes"])], fam["targets"], [fam["indices"]])
    rt = rt if row_target is None else row_target.cuda()
    inv = 1.0 / max(float(labels.numel()), 1.0)
    out = ops.set_loss_forward(logits, boxes, labels, tboxes, rt, desc, dims, inv)
    go = torch.tensor([cc.GRAD_OUT], dtype=torch.float32).cuda()
    gl, gb = ops.set_loss_backward(go, logits, boxes, labels, tboxes, rt, desc, dims, inv)
    torch.cuda.synchronize()
    shape = fam["logits"].shape[:2]
    return out[0].cpu(), gl.cpu().view(*shape, 3), gb.cpu().view(*shape, 4), rt.cpu()


def _matched_mask(fam):
    mask = torch.zeros(fam["logits"].shape[:2], dtype=torch.bool)
    for b, (ii, _) in enumerate(fam["indices"]):
        mask[b, ii] = True
    return mask


def _integer_outputs(tag, out, values):
    for k, name in ((1, "class_error"), (4, "cardinality_error")):
        print(f"  {tag} {name}: {out[k].item():.6f} against {values[k].item():.6f}")
        assert cc.rel_err(out[k], values[k]) <= 1e-6, name


@pytest.mark.parametrize("layout", ["dense", "spread"])
def test_giou_geometries_row_by_row(layout):
    """Every branch of giou_loss_grad by name (tests/_criterion_cases.GIOU_CONFIGS), one matched pair per row, against the
    torch formulation in fp64: loss values and every row of grad_boxes - the row's error over the ROW's largest reference
    magnitude - within 2^-23 (evaluated in fp64, rounded once on store).  ``spread`` lays the pairs over all 18 waves of the
    forward's strided walk over 1100 rows.

    What this test found: zero_width_straddling / zero_height_straddling (a prediction with one side of zero, between the
    target's edges on that axis and across a target edge on the other) had d(1 - GIoU)/d(that side) off by 10 % (-1.2346
    against -1.3642 for d/dw of the first; 2.5e-02 of the row's largest gradient here, the bound being 1.2e-07).  giou_loss_grad let the intersection's gradient through its clamp only where the clamped
    extent was > 0; at extent == 0 exactly the reference's clamp(min=0) passes it (the intersection grows with the side at
    the rate of the other extent, the only derivative there is on w >= 0).  With the prediction inside the target (the
    zero_*_inside rows) the dropped term is multiplied by g_inter = 0 - enclosure = union = target - and nothing shows.
    Fixed in csrc/criterion.hip: the gate is the unclamped extent >= 0."""
    fam = cc.giou_family(layout)
    values, _, ref_gb = cc.family_reference_fp64(cc.giou_family, layout)
    out, gl, gb, _ = _family_run(fam)
    assert torch.isfinite(out).all() and torch.isfinite(gl).all() and torch.isfinite(gb).all()
    failed = []
    for k, name in ((0, "loss_ce"), (2, "loss_bbox"), (3, "loss_giou")):
        err = cc.rel_err(out[k], values[k])
        print(f"  giou {layout} {name}: {out[k].item():.9g} against {values[k].item():.9g}, error {err:.3e}, bound {cc.ROW_BOUND:.3e}")
        if not err <= cc.ROW_BOUND:
            failed.append(f"{name} {err:.3e}")
    _integer_outputs(f"giou {layout}", out, values)
    rows = fam["indices"][0][0].tolist()
    errs = cc.row_rel_err(gb[0, rows], ref_gb[0, rows]).tolist()
    worst = {}
    for n, r, e in zip(fam["names"], rows, errs):
        if e >= worst.get(n, (-1.0, 0))[0]:
            worst[n] = (e, r)
    for n, (e, r) in worst.items():
        print(f"  giou {layout} {n}: worst row {r} error {e:.3e}, bound {cc.ROW_BOUND:.3e}")
        if not e <= cc.ROW_BOUND:
            failed.append(f"{n} (row {r}) {e:.3e}: gpu {gb[0, r].tolist()} against {ref_gb[0, r].tolist()}")
    assert not failed, "; ".join(failed)
    assert (gb[~_matched_mask(fam)] == 0).all() and (gl[..., 0] == 0).all()


def test_saturated_logits():
    """Columns 1 and 2 at 0, +-1e-3 ... +-1e4 in every role (matched to label 1, to label 0 or 2, unmatched) and rows whose
    arg-max ties exactly: loss_ce and grad_logits against the torch formulation in fp64, relative to the tensor's largest
    magnitude (the reference's 1 - (1 - p) cancels in fp64, so errors relative to a tiny gradient would measure the reference),
    within YARDSTICK_FACTOR x max(the error of the same formulation run in fp32 on the CPU, 2^-24: half an ulp of the one
    rounding, which keeps an exact yardstick from demanding bit equality)."""
    fam = cc.saturated_family()
    values, ref_gl, _ = cc.family_reference_fp64(cc.saturated_family)
    yard_values, yard_gl, _ = cc.family_reference(fam, torch.float32)
    out, gl, gb, _ = _family_run(fam)
    assert torch.isfinite(out).all() and torch.isfinite(gl).all() and torch.isfinite(gb).all()
    failed = []
    for what, got, ref, yard in (("loss_ce", out[0], values[0], yard_values[0]), ("grad_logits", gl, ref_gl, yard_gl)):
        y, err = cc.rel_err(yard, ref), cc.rel_err(got, ref)
        bound = cc.YARDSTICK_FACTOR * max(y, cc.HALF_ULP)
        print(f"  saturated {what}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, bound {bound:.3e}, max |ref| {ref.abs().max().item():.3e}")
        if not err <= bound:
            failed.append(f"{what}: gpu {err:.3e} against {bound:.3e}")
    assert not failed, "; ".join(failed)
    assert (gl[..., 0] == 0).all()
    _integer_outputs("saturated", out, values)


def test_match_cost_at_wide_logits():
    """Logits uniform in +-12: in fp32 the reference's -log(1 - p + 1e-8) loses digits as p nears 1 (at x = 8 half an ulp of p
    moves the cost by about 1e-4), so the bound per block is YARDSTICK_FACTOR x max(the error of cost_matrix run in fp32 on
    the CPU, 1e-5), both against cost_matrix in fp64.  Assignments are NOT compared at these logits: fp32 and fp64 costs
    differ by more than the gaps between them, so neither the reference nor the project has a stable answer there."""
    from dfx import ops
    from models.matcher import HungarianMatcher
    lg, bx, targets = cc.wide_cost_inputs()
    logits, boxes, labels, tboxes, _, desc, dims, d = _operands([(lg, bx)], targets)
    m = HungarianMatcher(**cc.COST)
    cost = ops.match_cost(logits, boxes, labels, tboxes, desc, dims, m.cost_class, m.cost_bbox, m.cost_giou).cpu()
    (S, B, rows, Ttot), Q, off = dims, lg.shape[1], d[3:]
    assert cost.numel() == Q * Ttot and torch.isfinite(cost).all()
    ids, tb = torch.cat([l for l, _ in targets]), torch.cat([b for _, b in targets])
    want = m.cost_matrix(lg, bx, ids, tb).view(B, Q, Ttot)
    yard = m.cost_matrix(lg.float(), bx.float(), ids, tb.float()).view(B, Q, Ttot)
    failed = []
    for b in range(B):
        ref = want[b][:, off[b]:off[b + 1]]
        got = cost[Q * off[b]:Q * off[b + 1]].view(Q, off[b + 1] - off[b]).double()
        y, err = (yard[b][:, off[b]:off[b + 1]].double() - ref).abs().max().item(), (got - ref).abs().max().item()
        bound = cc.YARDSTICK_FACTOR * max(y, 1e-5)
        print(f"  wide logits block {b}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, bound {bound:.3e}, max |cost| {ref.abs().max().item():.3e}")
        if not err <= bound:
            failed.append(f"block {b}: gpu {err:.3e} against {bound:.3e}")
    assert not failed, "; ".join(failed)


# ---- contracts at the entries and on the route ----------------------------------------------------------------------
def test_labels_outside_the_table_make_their_costs_nan():
    """labels 3 and -1 among valid ones: NaN in exactly those targets' columns of every block of a set with stored labels,
    every other entry finite and bit-equal to the run with valid labels in their place; a set whose labels are all zero
    (enc_outputs) does not read them"""
    from dfx import ops
    fam = cc.bad_label_family()
    g = torch.Generator().manual_seed(5)
    sets = [(fam["logits"], fam["boxes"]), (torch.randn(2, 3, 3, generator=g, dtype=torch.float64), cc.random_boxes(g, 2, 3)),
            (torch.randn(2, 4, 3, generator=g, dtype=torch.float64), cc.random_boxes(g, 2, 4))]
    zero = [False, False, True]
    logits, boxes, labels, tboxes, _, desc, dims, d = _operands(sets, fam["targets"], zero=zero)
    bad = ((labels < 0) | (labels > 2)).cpu()
    assert bad.sum() == 2
    valid = torch.where(bad.cuda(), torch.ones_like(labels), labels)
    cost = ops.match_cost(logits, boxes, labels, tboxes, desc, dims, 2, 5, 2).cpu()
    clean = ops.match_cost(logits, boxes, valid, tboxes, desc, dims, 2, 5, 2).cpu()
    assert torch.isfinite(clean).all()
    (S, B, rows, Ttot), off, base = dims, d[3 * len(sets):], 0
    for s in range(S):
        Q = d[3 * s]
        for b in range(B):
            blk = slice(base + Q * off[b], base + Q * off[b + 1])
            got, want = cost[blk].view(Q, -1), clean[blk].view(Q, -1)
            cols = bad[off[b]:off[b + 1]] & (not zero[s])
            assert torch.isnan(got[:, cols]).all() and torch.equal(got[:, ~cols], want[:, ~cols]), (s, b)
        base += Q * Ttot


def test_labels_outside_the_table_raise_on_the_fused_route():
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    fam = cc.bad_label_family()
    crit = SetCriterion(cc.NUM_CLASSES, HungarianMatcher(**cc.COST), dict(cc.COEF), cc.LOSSES)
    outputs = {"pred_logits": fam["logits"].float().cuda(), "pred_boxes": fam["boxes"].float().cuda()}
    targets = [{"labels": l.cuda(), "boxes": b.float().cuda()} for l, b in fam["targets"]]
    with pytest.raises(ValueError, match="invalid numeric"):
        crit(outputs, targets)
    with pytest.raises(ValueError, match="invalid numeric"):
        crit.matcher(outputs, targets)


def test_rows_matched_to_labels_outside_the_table_have_no_column():
    """a hand-written row_target pointing at targets with labels 3 and -1: matched for the box terms and class_error, "no
    column" for the classification - the torch formulation in fp64 fed label 3, whose one-hot is all zero.  Loss values and
    rows of grad_boxes within 2^-23 as in the GIoU families, grad_logits under the rule of the saturated family; and the
    logit gradients are bit-equal to those of the same rows left unmatched."""
    fam = cc.bad_label_family()
    values, ref_gl, ref_gb = cc.family_reference_fp64(cc.bad_label_family)
    _, yard_gl, _ = cc.family_reference(fam, torch.float32)
    out, gl, gb, rt = _family_run(fam)
    for k, name in ((0, "loss_ce"), (2, "loss_bbox"), (3, "loss_giou")):
        err = cc.rel_err(out[k], values[k])
        print(f"  bad labels {name}: {out[k].item():.9g} against {values[k].item():.9g}, error {err:.3e}, bound {cc.ROW_BOUND:.3e}")
        assert err <= cc.ROW_BOUND, name
    _integer_outputs("bad labels", out, values)
    mask = _matched_mask(fam)
    errs = cc.row_rel_err(gb[mask], ref_gb[mask])
    print(f"  bad labels grad_boxes: worst row {errs.max().item():.3e}, bound {cc.ROW_BOUND:.3e}")
    assert (errs <= cc.ROW_BOUND).all() and (gb[~mask] == 0).all()
    y, err = cc.rel_err(yard_gl, ref_gl), cc.rel_err(gl, ref_gl)
    bound = cc.YARDSTICK_FACTOR * max(y, cc.HALF_ULP)
    print(f"  bad labels grad_logits: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, bound {bound:.3e}")
    assert err <= bound and (gl[..., 0] == 0).all()
    labels = torch.cat([l for l, _ in fam["targets"]])
    rt2 = rt.clone()
    outside = (rt >= 0) & ((labels[rt.clamp(min=0).long()] < 0) | (labels[rt.clamp(min=0).long()] > 2))
    assert outside.sum() == 2
    rt2[outside] = -1
    _, gl2, gb2, _ = _family_run(fam, rt2)
    assert torch.equal(gl2, gl) and (gb2.view(-1, 4)[outside] == 0).all() and (gb.view(-1, 4)[outside] != 0).any()


@pytest.mark.parametrize("fused", [True, False])
def test_zero_area_pair_at_one_place_raises(fused, monkeypatch):
    """a prediction and its image's only target both of zero area at the same place: union 0, GIoU 0 / 0, a NaN cost, which
    the assignment refuses - ValueError on the fused route and on the torch route on the GPU"""
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    if not fused:
        monkeypatch.setenv("DFX_CRITERION", "0")
    g = torch.Generator().manual_seed(6)
    boxes = cc.random_boxes(g, 1, 4)
    boxes[0, 2] = torch.tensor([0.5, 0.5, 0.0, 0.0], dtype=torch.float64)
    outputs = {"pred_logits": torch.randn(1, 4, 3, generator=g).cuda(), "pred_boxes": boxes.float().cuda()}
    targets = [{"labels": torch.tensor([1]).cuda(), "boxes": torch.tensor([[0.5, 0.5, 0.0, 0.0]]).cuda()}]
    crit = SetCriterion(cc.NUM_CLASSES, HungarianMatcher(**cc.COST), dict(cc.COEF), cc.LOSSES)
    with pytest.raises(ValueError, match="invalid numeric"):
        crit(outputs, targets)
    with pytest.raises(ValueError, match="invalid numeric"):
        crit.matcher(outputs, targets)


def test_gpu_entries_refuse_what_the_header_says():
    """the three GPU entries called through the library with real device buffers: each refusal returns its documented code
    without a launch (every output keeps its NaN) and dfx_last_error() names the entry"""
    from dfx import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    EINVAL, ERANGE = _lib.CONSTANTS["DFX_EINVAL"], _lib.CONSTANTS["DFX_ERANGE"]
    S, B, Q, T = 1, 1, 4, 2
    rows = B * Q
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")      # noqa: E731
    g = torch.Generator().manual_seed(7)
    logits, boxes = torch.randn(rows, 3, generator=g).cuda(), cc.random_boxes(g, rows).float().cuda()
    labels, tboxes = torch.tensor([1, 2], dtype=torch.int32).cuda(), cc.random_boxes(g, T).float().cuda()
    desc = torch.tensor([Q, 0, 0, 0, T], dtype=torch.int32).cuda()
    rt = torch.tensor([-1, 0, -1, 1], dtype=torch.int32).cuda()
    go = torch.ones(S, 5).cuda()
    cost, out, gl, gb = nan(Q * T), nan(S, 5), nan(rows, 3), nan(rows, 4)
    p = lambda t: None if t is None else t.data_ptr()                         # noqa: E731

    def mc(S=S, B=B, rows=rows, T=T, cost=cost):
        return lib.dfx_match_cost_f32(p(logits), p(boxes), p(labels), p(tboxes), p(desc), S, B, rows, T, 2.0, 5.0, 2.0, p(cost), st)

    def fw(S=S, B=B, rows=rows, T=T, out=out, desc=desc):
        return lib.dfx_set_loss_forward_f32(p(logits), p(boxes), p(labels), p(tboxes), p(rt), p(desc), S, B, rows, T, 0.5, p(out), st)

    def bw(S=S, B=B, rows=rows, T=T, gl=gl, gb=gb):
        return lib.dfx_set_loss_backward_f32(p(go), p(logits), p(boxes), p(labels), p(tboxes), p(rt), p(desc), S, B, rows, T, 0.5,
                                             p(gl), p(gb), st)

    for name, fn in ((b"match_cost", mc), (b"set_loss_forward", fw), (b"set_loss_backward", bw)):
        for kw, code, text in ((dict(S=65), ERANGE, b"at most 64 sets"), (dict(B=4097), ERANGE, b"4096 images"),
                               (dict(rows=-1), EINVAL, b"bad dimension"), (dict(T=-1), EINVAL, b"bad dimension")):
            assert fn(**kw) == code, (name, kw)
            msg = lib.dfx_last_error()
            assert name in msg and text in msg, (name, kw, msg)
    assert mc(B=3) == EINVAL and b"match_cost: rows must be B * sum(Q)" in lib.dfx_last_error()
    assert mc(cost=None) == EINVAL and b"match_cost: null pointer" in lib.dfx_last_error()
    assert fw(out=None) == EINVAL and b"set_loss_forward: null pointer" in lib.dfx_last_error()
    assert bw(gl=None, gb=None) == 0
    # nothing to do: no set, no row
    assert mc(S=0) == 0 and fw(S=0) == 0 and bw(S=0) == 0
    assert mc(rows=0) == 0 and bw(rows=0) == 0
    torch.cuda.synchronize()
    for t in (cost, out, gl, gb):
        assert torch.isnan(t).all(), "a refused or empty call wrote to an output"
    # a set without rows still has its five results: the forward launches and returns 0
    empty_out = nan(S, 5)
    assert fw(rows=0, out=empty_out, desc=torch.tensor([0, 0, 0, 0, T], dtype=torch.int32).cuda()) == 0
    torch.cuda.synchronize()
    assert empty_out.cpu().tolist() == [[0.0, 100.0, 0.0, 0.0, float(T)]]
    # and the calls above were refusals of their arguments, not of the buffers
    assert mc() == 0 and fw() == 0 and bw() == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in (cost, out, gl, gb))


def test_one_criterion_object_over_growing_and_shrinking_calls():
    """recipe, one, stride, ragged, recipe through ONE SetCriterion: its pinned staging buffers grow, are reused larger than
    needed, and grow again (the cost buffer at ``stride``).  Every call's losses and gradients are bit-equal to a fresh
    object's on the same case, and the two recipe calls to each other."""
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    order = ["recipe", "one", "stride", "ragged", "recipe"]
    weights = {k: v for n in order for k, v in cc.weight_dict(cc.CASES[n]).items()}
    new = lambda: SetCriterion(cc.NUM_CLASSES, HungarianMatcher(**cc.COST), weights, cc.LOSSES)      # noqa: E731
    shared, seen, sizes = new(), {}, []
    for name in order:
        inputs = cc.prepared(name)[0]
        got = cc.run(name, inputs, shared, torch.float32, "cuda")
        (staging,) = shared._staging.values()
        sizes.append((staging.cost.numel(), staging.cost.data_ptr(), staging.row_target.numel()))
        want = cc.run(name, inputs, new(), torch.float32, "cuda")
        for a, b in zip(got, want):
            assert list(a) == list(b)
            for k in a:
                assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all(), (name, k)
        if name in seen:
            for a, b in zip(got, seen[name]):
                assert all(torch.equal(a[k], b[k]) for k in a), name
        seen[name] = got
    assert sizes[1][:2] == sizes[0][:2], "the small call reuses the larger buffer"
    assert sizes[2][0] > sizes[1][0] and sizes[3] == sizes[2] and sizes[4] == sizes[2], sizes
