"""CPU: the training criterion's op-by-op torch route against the reference's own results (tests/golden/criterion.npz,
tools/gen_golden_criterion.py), the host-side assignment solver against brute force and scipy, and the public surface."""
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _criterion_cases as cc


def _criterion(name):
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    return SetCriterion(cc.NUM_CLASSES, HungarianMatcher(**cc.COST), cc.weight_dict(cc.CASES[name]), cc.LOSSES)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_torch_route_in_fp64_is_the_reference(name):
    """every key in the reference's order, equal assignments, values and gradients within 1e-10 relative"""
    inputs, ref, _ = cc.prepared(name)
    crit = _criterion(name)
    losses, grads = cc.run(name, inputs, crit, torch.float64)
    assert list(losses) == ref["keys"]
    for n, a in cc.assignments(name, inputs, crit.matcher, torch.float64).items():
        assert np.array_equal(a, ref[f"assign.{n}"].numpy()), n
    for k, v in losses.items():
        assert v.dtype == torch.float64 or k.startswith(("class_error", "cardinality_error")), k
        assert cc.rel_err(v, ref[f"loss.{k}"]) <= 1e-10, (k, v.item(), ref[f"loss.{k}"].item())
    for k, v in grads.items():
        assert v.shape == ref[k].shape and cc.rel_err(v, ref[k]) <= 1e-10, k


def test_fixture_names_its_seeds_within_the_rule():
    z = cc.golden()
    for name, case in cc.CASES.items():
        assert case["base_seed"] <= int(z[f"{name}.seed"]) < case["base_seed"] + cc.MAX_SEEDS


def _brute_force(cost):
    """-> (total, rows, cols) of the cheapest assignment of min(Q, T) pairs, by enumeration"""
    Q, T = cost.shape
    best = None
    if Q <= T:
        for cols in itertools.permutations(range(T), Q):
            total = sum(cost[i, j] for i, j in enumerate(cols))
            if best is None or total < best[0]:
                best = (total, list(range(Q)), list(cols))
    else:
        for rows in itertools.permutations(range(Q), T):
            total = sum(cost[i, j] for j, i in enumerate(rows))
            if best is None or total < best[0]:
                order = sorted(range(T), key=lambda j: rows[j])
                best = (total, [rows[j] for j in order], order)
    return best


@pytest.mark.parametrize("Q,T", [(q, t) for q in range(1, 7) for t in range(1, 5)] + [(q, t) for q in range(1, 5) for t in (5, 6)])
def test_lsap_equals_brute_force(Q, T):
    """every shape up to 6 x 4 and 4 x 6, 20 seeds each: the total cost is equal and the pairs are identical"""
    from dfx import ops
    for seed in range(20):
        cost = torch.randn(Q, T, generator=torch.Generator().manual_seed(1000 * Q + 10 * T + seed))
        total, rows, cols = _brute_force(cost.double().numpy())
        i, j = ops.lsap(cost)
        assert i.dtype == torch.int64 and j.dtype == torch.int64 and len(i) == min(Q, T)
        assert i.tolist() == rows and j.tolist() == cols, (seed, cost)
        assert cost.double()[i, j].sum().item() == pytest.approx(total, rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("Q,T", [(300, 12), (5, 7), (70, 0)])
def test_lsap_equals_scipy(Q, T):
    scipy_optimize = pytest.importorskip("scipy.optimize")
    from dfx import ops
    cost = torch.randn(Q, T, generator=torch.Generator().manual_seed(Q + T))
    i, j = ops.lsap(cost)
    ri, rj = scipy_optimize.linear_sum_assignment(cost.numpy())
    assert i.tolist() == ri.tolist() and j.tolist() == rj.tolist()


def test_lsap_without_columns_or_rows_returns_no_pairs():
    from dfx import ops
    for shape in ((70, 0), (0, 5)):
        i, j = ops.lsap(torch.zeros(shape))
        assert i.numel() == 0 and j.numel() == 0 and i.dtype == torch.int64


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_lsap_refuses_non_finite_costs(bad):
    from dfx import ops
    cost = torch.randn(5, 3, generator=torch.Generator().manual_seed(0))
    cost[2, 1] = bad
    with pytest.raises(ValueError, match="invalid numeric"):
        ops.lsap(cost)
    desc, dims = ops.criterion_layout([5], [False], [3])
    with pytest.raises(ValueError, match="invalid numeric"):
        ops.lsap_ragged(cost.flatten().contiguous(), torch.tensor(desc, dtype=torch.int32), dims)


def test_lsap_ragged_fills_row_target_like_the_blocks():
    """two sets (7 and 2 queries) x three images with 0, 3 and 4 targets: every block solved as ``lsap`` solves it alone"""
    from dfx import ops
    queries, counts = [7, 2], [0, 3, 4]
    desc, dims = ops.criterion_layout(queries, [False, True], counts)
    S, B, rows, Ttot = dims
    assert (S, B, rows, Ttot) == (2, 3, 27, 7) and desc == [7, 0, 0, 2, 21, 1, 0, 0, 3, 7]
    cost = torch.randn(sum(queries) * Ttot, generator=torch.Generator().manual_seed(3))
    rt = ops.lsap_ragged(cost, torch.tensor(desc, dtype=torch.int32), dims)
    want = torch.full((rows,), -1, dtype=torch.int32)
    base, off = 0, [0, 0, 3, 7]
    for s, Q in enumerate(queries):
        for b, T in enumerate(counts):
            block = cost[base + Q * off[b]:base + Q * off[b + 1]].view(Q, T)
            for i, j in zip(*ops.lsap(block)):
                want[desc[3 * s + 1] + b * Q + i] = off[b] + j
        base += Q * Ttot
    assert torch.equal(rt, want) and (rt >= 0).sum() == 3 + 4 + 2 + 2


def test_constructor_refuses_what_the_loss_cannot_do():
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    m = HungarianMatcher(**cc.COST)
    with pytest.raises(ValueError, match="three-column alpha table"):
        SetCriterion(4, m, {}, cc.LOSSES)
    with pytest.raises(AssertionError, match="do you really want"):
        SetCriterion(3, m, {}, ["labels", "colours"])
    with pytest.raises(NotImplementedError):
        SetCriterion(3, m, {}, ["labels", "masks"])
    with pytest.raises(AssertionError):
        HungarianMatcher(0, 0, 0)


def test_matcher_has_the_reference_contract():
    """per image (int64 idx_i, int64 idx_j), min(Q, T) pairs sorted by query; more targets than queries is legal"""
    from models.matcher import HungarianMatcher
    g = torch.Generator().manual_seed(5)
    box = lambda *s: torch.cat([0.2 + 0.6 * torch.rand(*s, 2, generator=g), 0.05 + 0.3 * torch.rand(*s, 2, generator=g)], -1)  # noqa: E731
    out = {"pred_logits": torch.randn(3, 4, 3, generator=g), "pred_boxes": box(3, 4)}
    targets = [{"labels": torch.randint(0, 3, (T,), generator=g), "boxes": box(T)} for T in (0, 2, 6)]
    res = HungarianMatcher(**cc.COST)(out, targets)
    assert [len(i) for i, _ in res] == [0, 2, 4]
    for (i, j), T in zip(res, (0, 2, 6)):
        assert i.dtype == torch.int64 and j.dtype == torch.int64 and not i.is_cuda
        assert i.tolist() == sorted(i.tolist()) and len(set(j.tolist())) == len(j) and all(0 <= x < T for x in j.tolist())


def test_build_model_returns_a_working_criterion(golden_dir):
    """TransVOD++ namespace of tests/golden/args.json: SetCriterion with the weight_dict of loss_weight_dict(args); one
    forward + backward through it on CPU gives finite gradients on pred_logits and pred_boxes"""
    from models import build_model
    from models.criterion import SetCriterion
    from models.detector_common import TrainingOnly, loss_weight_dict     # noqa: F401  (stays importable)
    import models.deformable_detr_multi_plusplus as mpp
    import models.deformable_detr_multi as mm
    import models.deformable_detr_single as ms
    assert mpp.SetCriterion is SetCriterion and mm.SetCriterion is SetCriterion and ms.SetCriterion is SetCriterion
    ns = dict(json.load(open(os.path.join(golden_dir, "args.json")))["configs"]["TransVOD++.sh"]["namespace"])
    ns.update(device="cpu", dformer_weights=None)
    args = SimpleNamespace(**ns)
    _, criterion, _ = build_model(args)
    assert isinstance(criterion, SetCriterion) and criterion.weight_dict == loss_weight_dict(args)
    assert criterion.losses == ["labels", "boxes", "cardinality"] and criterion.matcher.cost_bbox == ns["set_cost_bbox"]

    g = torch.Generator().manual_seed(0)
    box = lambda *s: torch.cat([0.2 + 0.6 * torch.rand(*s, 2, generator=g), 0.05 + 0.3 * torch.rand(*s, 2, generator=g)], -1)  # noqa: E731
    logits = torch.randn(1, 30, 3, generator=g).requires_grad_(True)
    boxes = box(1, 30).requires_grad_(True)
    aux_l = torch.randn(1, 12, 3, generator=g).requires_grad_(True)
    aux_b = box(1, 12).requires_grad_(True)
    outputs = {"pred_logits": logits, "pred_boxes": boxes, "aux_outputs": [{"pred_logits": aux_l, "pred_boxes": aux_b}]}
    targets = [{"labels": torch.randint(0, 3, (2,), generator=g), "boxes": box(2)}]
    losses = criterion(outputs, targets)
    assert list(losses) == ["loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error",
                            "loss_ce_0", "loss_bbox_0", "loss_giou_0", "cardinality_error_0"]
    sum(losses[k] * criterion.weight_dict[k] for k in losses if k in criterion.weight_dict).backward()
    for t in (logits, boxes, aux_l, aux_b):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0
    assert not losses["cardinality_error"].requires_grad and not losses["class_error"].requires_grad


# ---- the hand-built families of tests/_criterion_cases.py: what their names claim, computed in fp64 ----------------------
def _built_pairs(layout="dense"):
    fam = cc.giou_family(layout)
    rows = fam["indices"][0][0].tolist()
    return [(n, fam["boxes"][0, r], fam["targets"][0][1][k]) for k, (n, r) in enumerate(zip(fam["names"], rows))]


def test_giou_configurations_have_the_property_their_name_claims():
    """on the fp32-representable values the kernels are given: no edge of a prediction coincides with an edge of its target,
    no coordinate equals the target's, sides are at least 0.01 unless zero is the point, and each kind is what it says"""
    kinds = set()
    pairs = _built_pairs()
    assert [n for n, _, _ in pairs] == list(cc.GIOU_CONFIGS)
    for name, pred, tgt in pairs:
        kind = cc.GIOU_CONFIGS[name][0]
        kinds.add(kind)
        f = cc.giou_facts(pred, tgt)
        rx, ry = f["raw"]
        assert f["coincidences"] == 0 and f["target_area"] > 0 and f["enclosure"] > 0, name
        assert all(s >= 0.01 or (s == 0 and kind.startswith("zero")) for s in f["sides"]), name
        if kind in ("partial", "corner"):
            assert rx > 0 and ry > 0 and 0 < f["inter"] < min(f["area"], f["target_area"]), name
            assert not f["pred_inside"] and not f["target_inside"], name
            assert (f["inter"] < 0.05 * f["area"]) == (kind == "corner"), name
        elif kind == "disjoint_x":
            assert rx < 0 < ry and f["inter"] == 0, name
        elif kind == "disjoint_y":
            assert ry < 0 < rx and f["inter"] == 0, name
        elif kind == "disjoint_both":
            assert rx < 0 and ry < 0 and f["inter"] == 0, name
        elif kind == "pred_inside":
            assert f["pred_inside"] and f["area"] > 0 and f["inter"] == pytest.approx(f["area"], rel=1e-12), name
        elif kind == "target_inside":
            assert f["target_inside"] and f["inter"] == pytest.approx(f["target_area"], rel=1e-12), name
        elif kind == "zero_side_inside":
            assert f["pred_inside"] and f["area"] == 0 and f["inter"] == 0 and sorted(f["sides"])[0] == 0 < sorted(f["sides"])[1], name
            assert min(rx, ry) == 0 < max(rx, ry), name
        elif kind == "zero_side_straddling":
            assert not f["pred_inside"] and f["area"] == 0 and f["inter"] == 0 and min(rx, ry) == 0, name
            assert 0 < max(rx, ry) < max(f["sides"]), name           # the other axis overlaps in part
        elif kind == "zero_area_away":
            assert f["sides"] == [0, 0] and min(rx, ry) < 0 and f["inter"] == 0, name
        elif kind == "far_apart":
            assert rx < -0.8 and ry < -0.8 and f["enclosure"] > 100 * (f["area"] + f["target_area"]), name
        else:
            raise AssertionError(f"{name}: unknown kind {kind}")
    assert kinds == {"partial", "corner", "disjoint_x", "disjoint_y", "disjoint_both", "pred_inside", "target_inside",
                     "zero_side_inside", "zero_side_straddling", "zero_area_away", "far_apart"}
    # both axis orders and both sides of every max / min: which edge of the prediction lies beyond the target's, per axis
    sides = {(d, bool(p[d] - 0.5 * p[2 + d] < t[d] - 0.5 * t[2 + d]), bool(p[d] + 0.5 * p[2 + d] > t[d] + 0.5 * t[2 + d]))
             for _, p, t in pairs for d in range(2)}
    assert sides == {(d, lo, hi) for d in range(2) for lo in (False, True) for hi in (False, True)}


def test_spread_layout_puts_the_pairs_in_every_wave_of_every_pass():
    """1100 rows under 512 threads: passes at 0, 512, 1024, waves of 64 lanes - 18 (pass, wave) slots, each with two matched
    rows; every configuration appears, with the dense layout's boxes"""
    fam = cc.giou_family("spread")
    rows = fam["indices"][0][0].tolist()
    assert fam["logits"].shape == (1, cc.SPREAD_Q, 3) and len(set(rows)) == len(rows) == 36 and max(rows) == cc.SPREAD_Q - 1
    slots = {}
    for r in rows:
        slots.setdefault((r // 512, (r % 512) // 64), []).append(r)
    assert sorted(slots) == [(p, w) for p in range(2) for w in range(8)] + [(2, 0), (2, 1)] and all(len(v) == 2 for v in slots.values())
    assert set(fam["names"]) == set(cc.GIOU_CONFIGS)
    dense = {n: (p, t) for n, p, t in _built_pairs("dense")}
    for n, p, t in _built_pairs("spread"):
        assert torch.equal(p, dense[n][0]) and torch.equal(t, dense[n][1]), n


def test_saturated_family_uses_every_value_in_every_role():
    fam = cc.saturated_family()
    logits, (matched, cols) = fam["logits"][0], fam["indices"][0]
    labels = fam["targets"][0][0][cols]
    role = torch.full((logits.shape[0],), 2)
    role[matched] = torch.where(labels == 1, 0, 1)
    values = sorted(torch.tensor(cc.SATURATED, dtype=torch.float32).double().tolist())
    assert len(values) == 15 and 1e4 in values and -1e4 in values
    plain = torch.arange(logits.shape[0]) < 3 * len(values)
    for r in range(3):
        for c in (1, 2):
            assert sorted(logits[plain & (role == r), c].tolist()) == values, (r, c)
        assert (role[~plain] == r).sum() == len(cc.TIE_ROWS)
    assert set(labels[role[matched] == 1].tolist()) == {0, 2}
    ties = logits[~plain]
    top = ties.max(-1, keepdim=True).values
    assert ((ties == top).sum(-1) >= 2).all()
    assert ((ties[:, 0] == top[:, 0]) & (ties[:, 1] == top[:, 0])).any() and ((ties[:, 1] == top[:, 0]) & (ties[:, 2] == top[:, 0]) & (ties[:, 0] < top[:, 0])).any()


@pytest.mark.parametrize("builder,args", [(cc.giou_family, ("dense",)), (cc.giou_family, ("spread",)), (cc.saturated_family, ()),
                                          (cc.bad_label_family, ())])
def test_family_references_are_finite_and_their_fp32_run_is_a_rounding(builder, args):
    """the fp64 torch formulation the GPU tests compare with, and the same in fp32 (evaluated in fp64, rounded once): within a
    few ulp of it relative to each tensor's largest magnitude"""
    ref = cc.family_reference_fp64(builder, *args)
    f32 = cc.family_reference(builder(*args), torch.float32)
    for a, b in zip(ref[0] + ref[1:], f32[0] + f32[1:]):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert cc.rel_err(b, a) <= 4 * cc.HALF_ULP


def test_wide_cost_inputs_reach_the_saturated_log():
    logits, boxes, targets = cc.wide_cost_inputs()
    assert logits.shape == (2, 40, 3) and [len(l) for l, _ in targets] == [3, 9]
    assert logits.max() > 11 and logits.min() < -11 and torch.equal(logits, logits.float().double())
