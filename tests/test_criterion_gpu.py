"""GPU: the training criterion's fused route (csrc/criterion.hip: dfx_match_cost_f32, dfx_set_loss_forward_f32,
dfx_set_loss_backward_f32, assignment on the host) on the cases of tests/_criterion_cases.py against the reference's own fp64
results, within the project's yardstick rule: per output, error relative to the reference's largest magnitude (absolute where
the reference is identically zero) at most YARDSTICK_FACTOR x the error of the reference's own fp32 run.  The two
integer-valued outputs, class_error and cardinality_error, are instead equal to the reference to 1e-6, measured the same
way (relative to the reference's magnitude: 100 - 100 * 1 / 3 has no exact fp32 value)."""
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


@pytest.mark.parametrize("name", ["ragged", "enc"])
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


def test_match_cost_blocks_equal_the_torch_formulation():
    """every (set, image) block of the ragged case at its documented offset, against the op-by-op cost matrix in fp64: fp32
    arithmetic on costs of order 1 to 10 - 1e-5 absolute is 20 ulp of the largest cost"""
    from dfx import ops
    from models.matcher import HungarianMatcher
    name = "ragged"
    case = cc.CASES[name]
    logits, boxes, labels, tboxes, _, desc, dims, d = _flat_operands(name)
    m = HungarianMatcher(**cc.COST)
    cost = ops.match_cost(logits, boxes, labels, tboxes, desc, dims, m.cost_class, m.cost_bbox, m.cost_giou).cpu()
    S, B, rows, Ttot = dims
    assert cost.numel() == (rows // B) * Ttot and torch.isfinite(cost).all()
    off, base = d[3 * S:], 0
    for s in range(S):
        Q, row0 = d[3 * s], d[3 * s + 1]
        lg = logits[row0:row0 + B * Q].view(B, Q, 3).double().cpu()
        bx = boxes[row0:row0 + B * Q].view(B, Q, 4).double().cpu()
        want = m.cost_matrix(lg, bx, labels.long().cpu(), tboxes.double().cpu()).view(B, Q, Ttot)
        for b in range(B):
            got = cost[base + Q * off[b]:base + Q * off[b + 1]].view(Q, off[b + 1] - off[b])
            assert (got.double() - want[b][:, off[b]:off[b + 1]]).abs().max().item() <= 1e-5 if got.numel() else True, (s, b)
        base += Q * Ttot


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
