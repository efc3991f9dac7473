"""Cases of the training criterion shared by tools/gen_golden_criterion.py (which runs the REFERENCE's SetCriterion +
HungarianMatcher on them, once in fp64 -> ``ref.*`` and once in fp32 -> ``f32.*``, the yardstick) and by
tests/test_criterion_{cpu,gpu}.py (which run this project's).  tests/golden/criterion.npz holds the reference's results
only; inputs are regenerated here from the seed the fixture names.

The smallest shapes that can still go wrong:
  ragged   a wave tail (70 = 64 + 6), an image without targets, more targets than queries in the 5-query set, differing Q
  empty    no target in the whole batch: the num_boxes clamp, class_error = 100, zero box losses and gradients
  enc      enc_outputs against zeroed labels under ``*_enc`` keys next to an aux set
  one      one query, one target
  recipe   the recipes' shape: 7 sets of 300 queries with enc_outputs, 12 targets in one image
  stride   the forward's strided walk: 1100 = two full strides of 512 and a tail of 76, 513 = one stride and one row, 20
           targets against 5 queries
  images   nine images of 3 and 1 queries: a sum over the workgroup per image, T > Q, T = 0 in the middle and next to the end

The hand-built families at the end of the file go straight to the kernels with a row_target written by hand: every branch of
the GIoU backward by name (GIOU_CONFIGS, dense and spread over 1100 rows), logits from 0 to +-1e4 in every role
(saturated_family), labels outside 0..2 (bad_label_family), matching costs at logits of +-12 (wide_cost_inputs).

The assignment is discrete, so a case only counts where the reference alone is stable on it: the generator takes the first
seed (counting up from ``base_seed``, at most MAX_SEEDS - the rule of tests/_inference_kernel_cases.py) for which the fp64
and fp32 assignments agree for every set and still agree under N_PERTURB seeded relative perturbations of PERTURB of the
fp64 cost matrices.
"""
import functools
import os

import numpy as np
import torch

from tests import _golden

YARDSTICK_FACTOR = 4
MAX_SEEDS = 64
N_PERTURB, PERTURB = 16, 1e-4
NUM_CLASSES = 3
COST = dict(cost_class=2, cost_bbox=5, cost_giou=2)
COEF = {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2}
LOSSES = ["labels", "boxes", "cardinality"]

# name -> B, main Q, aux Qs, enc Q | None, targets per image, base seed
CASES = {
    "ragged": dict(B=3, main=70, aux=(30, 5), enc=None, targets=(0, 1, 7), base_seed=1000),
    "empty": dict(B=2, main=70, aux=(), enc=None, targets=(0, 0), base_seed=2000),
    "enc": dict(B=2, main=70, aux=(70,), enc=70, targets=(2, 3), base_seed=3000),
    "one": dict(B=1, main=1, aux=(), enc=None, targets=(1,), base_seed=4000),
    "recipe": dict(B=2, main=300, aux=(300, 300, 300, 300, 300), enc=300, targets=(12, 1), base_seed=5000),
    "stride": dict(B=2, main=1100, aux=(513, 5), enc=None, targets=(20, 2), base_seed=6000),
    "images": dict(B=9, main=3, aux=(1,), enc=None, targets=(0, 1, 2, 3, 4, 0, 1, 5, 2), base_seed=7000),
}


def set_names(case):
    """names of the case's prediction sets in the criterion's order: main, aux0.., enc"""
    return ["main"] + [f"aux{i}" for i in range(len(case["aux"]))] + (["enc"] if case["enc"] is not None else [])


def set_suffixes(case):
    return [""] + [f"_{i}" for i in range(len(case["aux"]))] + (["_enc"] if case["enc"] is not None else [])


def weight_dict(case):
    return {k + sfx: v for sfx in set_suffixes(case) for k, v in COEF.items()}


def _f32(t):
    return t.float().double()


def random_boxes(g, *lead):
    """(cx, cy, w, h): centres in 0.2 .. 0.8, sides in 0.05 .. 0.35"""
    centre = 0.2 + 0.6 * torch.rand(*lead, 2, generator=g, dtype=torch.float64)
    size = 0.05 + 0.3 * torch.rand(*lead, 2, generator=g, dtype=torch.float64)
    return _f32(torch.cat([centre, size], dim=-1))


def make_inputs(name, seed):
    """fp64 tensors holding fp32-representable values: {set: (logits [B,Q,3], boxes [B,Q,4])}, [(labels int64 [T], boxes [T,4])]"""
    case = CASES[name]
    g = torch.Generator().manual_seed(seed)

    def boxes(*lead):
        return random_boxes(g, *lead)

    sets = {}
    for n, Q in zip(set_names(case), (case["main"],) + tuple(case["aux"]) + ((case["enc"],) if case["enc"] is not None else ())):
        sets[n] = (_f32(torch.randn(case["B"], Q, NUM_CLASSES, generator=g, dtype=torch.float64)), boxes(case["B"], Q))
    targets = [(torch.randint(0, NUM_CLASSES, (T,), generator=g), boxes(T)) for T in case["targets"]]
    return sets, targets


def build_outputs(name, inputs, dtype, device="cpu"):
    """-> (outputs dict as a detector returns it, targets list, {set: (logits leaf, boxes leaf)})"""
    case = CASES[name]
    sets, targets = inputs
    leaves = {n: tuple(t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for t in pair) for n, pair in sets.items()}
    as_set = lambda n: {"pred_logits": leaves[n][0], "pred_boxes": leaves[n][1]}      # noqa: E731
    outputs = as_set("main")
    if case["aux"]:
        outputs["aux_outputs"] = [as_set(f"aux{i}") for i in range(len(case["aux"]))]
    if case["enc"] is not None:
        outputs["enc_outputs"] = as_set("enc")
    tg = [{"labels": l.to(device), "boxes": b.to(device=device, dtype=dtype)} for l, b in targets]
    return outputs, tg, leaves


def run(name, inputs, criterion, dtype, device="cpu"):
    """One forward + backward of ``criterion`` on the case -> (ordered loss dict of python floats, {``grad.<set>.logits`` /
    ``grad.<set>.boxes``: cpu tensors}); the differentiated scalar is sum(weight_dict[k] * loss[k])."""
    outputs, tg, leaves = build_outputs(name, inputs, dtype, device)
    losses = criterion(outputs, tg)
    wd = criterion.weight_dict
    total = sum(losses[k] * wd[k] for k in losses if k in wd)
    total.backward()
    grads = {}
    for n, (lg, bx) in leaves.items():
        grads[f"grad.{n}.logits"] = (torch.zeros_like(lg) if lg.grad is None else lg.grad).detach().cpu()
        grads[f"grad.{n}.boxes"] = (torch.zeros_like(bx) if bx.grad is None else bx.grad).detach().cpu()
    return {k: v.detach().cpu() for k, v in losses.items()}, grads


def assignment_array(indices):
    """[(i, j)] per image -> int64 [n, 3] rows (image, query, target)"""
    rows = [(b, int(i), int(j)) for b, (ii, jj) in enumerate(indices) for i, j in zip(ii.tolist(), jj.tolist())]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def assignments(name, inputs, matcher, dtype, device="cpu"):
    """``matcher`` on every set of the case (zeroed labels for enc) -> {set: int64 [n,3]}"""
    outputs, tg, leaves = build_outputs(name, inputs, dtype, device)
    out = {}
    for n, (lg, bx) in leaves.items():
        t = [{**x, "labels": torch.zeros_like(x["labels"])} for x in tg] if n == "enc" else tg
        out[n] = assignment_array(matcher({"pred_logits": lg.detach(), "pred_boxes": bx.detach()}, t))
    return out


def row_target_to_assignments(name, row_target):
    """the fused route's row_target [rows] (global target index or -1) -> {set: int64 [n,3]}"""
    case = CASES[name]
    off = np.concatenate([[0], np.cumsum(case["targets"])])
    qs = (case["main"],) + tuple(case["aux"]) + ((case["enc"],) if case["enc"] is not None else ())
    out, row = {}, 0
    rt = np.asarray(row_target)
    for n, Q in zip(set_names(case), qs):
        rows = []
        for b in range(case["B"]):
            for q in range(Q):
                if rt[row] >= 0:
                    rows.append((b, q, int(rt[row] - off[b])))
                row += 1
        out[n] = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    assert row == rt.size
    return out


def rel_err(got, ref):
    """largest absolute error relative to the reference's largest magnitude; the absolute error where the reference is
    identically zero (tests/_mha_cases.rel_err)"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    if ref.numel() == 0:
        return 0.0
    err, top = (got - ref).abs().max().item(), ref.abs().max().item()
    return err if top == 0 else err / top


@functools.lru_cache(maxsize=None)
def golden():
    return _golden.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "criterion")


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> (inputs regenerated from the fixture's seed, ref, f32): the two mappings hold ``keys`` (the ordered loss keys),
    ``loss.<key>``, ``assign.<set>`` and ``grad.<set>.{logits,boxes}`` as torch tensors.  Shared by the tests, never written."""
    z = golden()
    seed = int(z[f"{name}.seed"])
    out = []
    for tag in ("ref", "f32"):
        pre = f"{tag}.{name}."
        m = {k[len(pre):]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(pre) and not k.endswith(".keys")}
        m["keys"] = [str(k) for k in z[pre + "keys"]]
        out.append(m)
    return make_inputs(name, seed), out[0], out[1]


# ---- hand-built families, run straight on the kernels with a row_target written by hand -----------------------------
# Their reference is this project's own torch formulation in fp64 on the CPU (SetCriterion._set_losses with explicit indices,
# HungarianMatcher.cost_matrix), which tests/test_criterion_cpu.py pins to the reference's results within 1e-10.  A family is
#   logits [B,Q,3], boxes [B,Q,4]        fp64 tensors holding fp32-representable values, one prediction set
#   targets [(labels int64 [T], boxes [T,4])] per image;  indices [(rows, cols)] per image: the hand-written assignment
#   names                                 one string per matched pair, image after image, pair after pair
#   ref_labels (optional)                 per image, the labels the torch formulation is fed where the kernel's differ
GRAD_OUT = (COEF["loss_ce"], 0.0, COEF["loss_bbox"], COEF["loss_giou"], 0.0)       # d(total) / d(out[s, :]) of one set
ROW_BOUND = 2.0 ** -23      # per row and per loss value: half an ulp of the one rounding on store, and as much again for the
                            # fp64 evaluation on both sides (include/dfx_criterion.h: evaluated in fp64, rounded once)
HALF_ULP = 2.0 ** -24

# name -> (kind, prediction, target), boxes as (cx, cy, w, h).  No edge of a prediction coincides with an edge of its target
# and no coordinate equals the target's: the sub-gradient is not unique there.  Sides are at least 0.01 except
# where zero is the point.  Target (0.5, 0.5, 0.3, 0.2) spans x 0.35 .. 0.65, y 0.40 .. 0.60.
_T0 = (0.5, 0.5, 0.3, 0.2)
GIOU_CONFIGS = {
    "partial_right_up": ("partial", (0.58, 0.55, 0.22, 0.26), _T0),                # x 0.47 .. 0.69, y 0.42 .. 0.68
    "partial_left_down": ("partial", (0.42, 0.44, 0.26, 0.22), _T0),               # x 0.29 .. 0.55, y 0.33 .. 0.55
    "disjoint_x_left": ("disjoint_x", (0.15, 0.52, 0.10, 0.12), _T0),              # y inside the target's
    "disjoint_x_right": ("disjoint_x", (0.85, 0.47, 0.12, 0.30), _T0),             # y covers the target's
    "disjoint_y_below": ("disjoint_y", (0.52, 0.15, 0.16, 0.10), _T0),
    "disjoint_y_above": ("disjoint_y", (0.47, 0.85, 0.40, 0.12), _T0),
    "disjoint_both_low": ("disjoint_both", (0.15, 0.20, 0.10, 0.12), _T0),
    "disjoint_both_high": ("disjoint_both", (0.85, 0.82, 0.14, 0.10), _T0),
    "disjoint_both_mixed": ("disjoint_both", (0.14, 0.84, 0.12, 0.10), _T0),
    "pred_inside_target": ("pred_inside", (0.48, 0.52, 0.10, 0.06), _T0),
    "target_inside_pred": ("target_inside", (0.52, 0.47, 0.50, 0.40), _T0),
    "zero_width_inside": ("zero_side_inside", (0.45, 0.53, 0.0, 0.10), _T0),
    "zero_height_inside": ("zero_side_inside", (0.56, 0.45, 0.12, 0.0), _T0),
    "zero_width_straddling": ("zero_side_straddling", (0.45, 0.62, 0.0, 0.10), _T0),      # y 0.57 .. 0.67 across the target's 0.60
    "zero_height_straddling": ("zero_side_straddling", (0.62, 0.45, 0.12, 0.0), _T0),     # x 0.56 .. 0.68 across the target's 0.65
    "zero_area_away": ("zero_area_away", (0.10, 0.90, 0.0, 0.0), _T0),
    "zero_area_above": ("zero_area_away", (0.45, 0.90, 0.0, 0.0), _T0),            # inside the target's x range
    "corner_top_right": ("corner", (0.70, 0.65, 0.16, 0.14), _T0),                 # x 0.62 .. 0.78, y 0.58 .. 0.72
    "corner_bottom_left": ("corner", (0.30, 0.36, 0.14, 0.16), _T0),               # x 0.23 .. 0.37, y 0.28 .. 0.44
    "corner_top_left": ("corner", (0.31, 0.64, 0.12, 0.14), _T0),                  # x 0.25 .. 0.37, y 0.57 .. 0.71
    "corner_bottom_right": ("corner", (0.69, 0.37, 0.12, 0.10), _T0),              # x 0.63 .. 0.75, y 0.32 .. 0.42
    "far_apart": ("far_apart", (0.04, 0.05, 0.03, 0.02), (0.95, 0.94, 0.06, 0.08)),
    "far_apart_swapped": ("far_apart", (0.96, 0.03, 0.02, 0.04), (0.05, 0.93, 0.07, 0.05)),
}
SPREAD_Q = 1100
# two rows in every wave of every pass of the forward's strided walk over 1100 rows (8 waves x 64 lanes, passes at 0, 512
# and 1024; the last wave holds rows 1088 .. 1099)
SPREAD_ROWS = tuple(r for w in range(18) for r in (64 * w + 5, min(64 * w + 40, SPREAD_Q - 1)))

SATURATED = (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0, 17.0, -17.0, 40.0, -40.0, 90.0, -90.0, 1e4, -1e4)
# (x0, x1, x2): exact ties for the arg-max, which go to the lowest index
TIE_ROWS = ((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (2.0, 2.0, 2.0), (-1e4, 1e4, 1e4), (1e4, 1e4, -1e4))


def giou_facts(pred, tgt):
    """fp64 facts about one (prediction, target) pair of (cx, cy, w, h) boxes"""
    p, t = torch.as_tensor(pred, dtype=torch.float64), torch.as_tensor(tgt, dtype=torch.float64)
    lo, hi, blo, bhi = p[:2] - 0.5 * p[2:], p[:2] + 0.5 * p[2:], t[:2] - 0.5 * t[2:], t[:2] + 0.5 * t[2:]
    raw = torch.minimum(hi, bhi) - torch.maximum(lo, blo)              # per axis, before the clamp at 0
    enc = torch.maximum(hi, bhi) - torch.minimum(lo, blo)
    return dict(
        raw=raw.tolist(), inter=(raw.clamp(min=0)[0] * raw.clamp(min=0)[1]).item(), enclosure=(enc[0] * enc[1]).item(),
        area=(p[2] * p[3]).item(), target_area=(t[2] * t[3]).item(), sides=p[2:].tolist(),
        pred_inside=bool(((lo > blo) & (hi < bhi)).all()), target_inside=bool(((lo < blo) & (hi > bhi)).all()),
        coincidences=int(sum((a == b).sum().item() for a in (lo, hi) for b in (blo, bhi)) + (p == t).sum().item()))


def _family(logits, boxes, targets, indices, names, ref_labels=None):
    return dict(logits=_f32(logits), boxes=_f32(boxes), targets=[(l, _f32(b)) for l, b in targets],
                indices=[(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in indices],
                names=list(names), ref_labels=ref_labels)


@functools.lru_cache(maxsize=None)
def giou_family(layout):
    """``dense``: one image, one set of Q = len(GIOU_CONFIGS) rows, row i matched to target i.  ``spread``: the same pairs,
    cyclically, at SPREAD_ROWS of a 1100-query set with unmatched random rows in between."""
    g = torch.Generator().manual_seed(77)
    names = list(GIOU_CONFIGS)
    if layout == "dense":
        rows, Q = list(range(len(names))), len(names)
    else:
        rows, Q = list(SPREAD_ROWS), SPREAD_Q
        names = [names[k % len(names)] for k in range(len(rows))]
    logits = torch.randn(1, Q, NUM_CLASSES, generator=g, dtype=torch.float64)
    boxes = random_boxes(g, 1, Q)
    for r, n in zip(rows, names):
        boxes[0, r] = torch.tensor(GIOU_CONFIGS[n][1], dtype=torch.float64)
    tboxes = torch.tensor([GIOU_CONFIGS[n][2] for n in names], dtype=torch.float64)
    labels = torch.randint(0, NUM_CLASSES, (len(names),), generator=g)
    return _family(logits, boxes, [(labels, tboxes)], [(rows, list(range(len(rows))))], names)


@functools.lru_cache(maxsize=None)
def saturated_family():
    """One image.  Per value v of SATURATED three rows with x1 = v - matched to label 1, matched to label 0 or 2 (in turn),
    unmatched - whose x2 walks SATURATED from another start, so that both columns take every value in every role; then
    TIE_ROWS in the same three roles.  x0 is 0.5 except in the tie rows."""
    rows, roles = [], []
    n = len(SATURATED)
    for i, v in enumerate(SATURATED):
        for role in range(3):
            rows.append((0.5, v, SATURATED[(i + 4 * role + 1) % n]))
            roles.append(role)
    for x in TIE_ROWS:
        for role in range(3):
            rows.append(x)
            roles.append(role)
    logits = torch.tensor(rows, dtype=torch.float64)[None]
    matched = [r for r, role in enumerate(roles) if role != 2]
    other = iter([0, 2] * len(rows))
    labels = torch.tensor([1 if roles[r] == 0 else next(other) for r in matched])
    g = torch.Generator().manual_seed(78)
    names = [f"row {r} {tuple(rows[r])} label {l}" for r, l in zip(matched, labels.tolist())]
    return _family(logits, random_boxes(g, 1, len(rows)), [(labels, random_boxes(g, len(matched)))],
                   [(matched, list(range(len(matched))))], names)


@functools.lru_cache(maxsize=None)
def bad_label_family():
    """Two images of 6 queries; targets (3, 4) with labels (0, 3, 1) and (2, -1, 1, 0): rows matched by hand to every target,
    the two with a label outside 0..2 among them.  The torch formulation is fed label 3 for both, whose one-hot (cut to
    three columns) is all zero: "no column"."""
    g = torch.Generator().manual_seed(79)
    labels = [torch.tensor([0, 3, 1]), torch.tensor([2, -1, 1, 0])]
    targets = [(l, random_boxes(g, len(l))) for l in labels]
    indices = [([0, 2, 5], [1, 0, 2]), ([1, 2, 3, 4], [3, 1, 0, 2])]
    names = [f"image {b} row {i} target {j} label {labels[b][j].item()}" for b, (ii, jj) in enumerate(indices) for i, j in zip(ii, jj)]
    return _family(torch.randn(2, 6, NUM_CLASSES, generator=g, dtype=torch.float64), random_boxes(g, 2, 6), targets, indices, names,
                   ref_labels=[torch.where((l < 0) | (l >= NUM_CLASSES), NUM_CLASSES, l) for l in labels])


def wide_cost_inputs():
    """-> logits [2,40,3] uniform in +-12, boxes [2,40,4], [(labels, boxes)] with (3, 9) targets"""
    g = torch.Generator().manual_seed(80)
    logits = _f32(24.0 * torch.rand(2, 40, NUM_CLASSES, generator=g, dtype=torch.float64) - 12.0)
    return logits, random_boxes(g, 2, 40), [(torch.randint(0, NUM_CLASSES, (T,), generator=g), random_boxes(g, T)) for T in (3, 9)]


def family_reference(fam, dtype=torch.float64):
    """The project's torch formulation on a family, on the CPU in ``dtype`` -> (values: loss_ce, class_error, loss_bbox,
    loss_giou, cardinality_error as tensors, grad_logits [B,Q,3], grad_boxes [B,Q,4]) of sum(GRAD_OUT * values)."""
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    crit = SetCriterion(NUM_CLASSES, HungarianMatcher(**COST), {}, LOSSES)
    logits = fam["logits"].to(dtype).clone().requires_grad_(True)
    boxes = fam["boxes"].to(dtype).clone().requires_grad_(True)
    labels = fam["ref_labels"] or [l for l, _ in fam["targets"]]
    targets = [{"labels": l, "boxes": b.to(dtype)} for l, (_, b) in zip(labels, fam["targets"])]
    num_boxes = max(float(sum(len(l) for l in labels)), 1.0)
    values = crit._set_losses(logits, boxes, targets, fam["indices"], num_boxes)
    (GRAD_OUT[0] * values[0] + GRAD_OUT[2] * values[2] + GRAD_OUT[3] * values[3]).backward()
    return tuple(v.detach() for v in values), logits.grad.detach(), boxes.grad.detach()


@functools.lru_cache(maxsize=None)
def family_reference_fp64(builder, *args):
    """shared by the tests, never written"""
    return family_reference(builder(*args))


def row_rel_err(got, ref):
    """per row: largest absolute error of the row over the row's largest reference magnitude (absolute where that is 0)"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err, top = (got - ref).abs().amax(-1), ref.abs().amax(-1)
    return torch.where(top == 0, err, err / top.clamp(min=torch.finfo(torch.float64).tiny))
