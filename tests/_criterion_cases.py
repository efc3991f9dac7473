"""Cases of the training criterion shared by tools/gen_golden_criterion.py (which runs the REFERENCE's SetCriterion +
HungarianMatcher on them, once in fp64 -> ``ref.*`` and once in fp32 -> ``f32.*``, the yardstick) and by
tests/test_criterion_{cpu,gpu}.py (which run this project's).  tests/golden/criterion.npz holds the reference's results
only; inputs are regenerated here from the seed the fixture names.

The smallest shapes that can still go wrong:
  ragged   a wave tail (70 = 64 + 6), an image without targets, more targets than queries in the 5-query set, differing Q
  empty    no target in the whole batch: the num_boxes clamp, class_error = 100, zero box losses and gradients
  enc      enc_outputs against zeroed labels under ``*_enc`` keys next to an aux set
  one      one query, one target

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


def make_inputs(name, seed):
    """fp64 tensors holding fp32-representable values: {set: (logits [B,Q,3], boxes [B,Q,4])}, [(labels int64 [T], boxes [T,4])]"""
    case = CASES[name]
    g = torch.Generator().manual_seed(seed)

    def boxes(*lead):
        centre = 0.2 + 0.6 * torch.rand(*lead, 2, generator=g, dtype=torch.float64)
        size = 0.05 + 0.3 * torch.rand(*lead, 2, generator=g, dtype=torch.float64)
        return _f32(torch.cat([centre, size], dim=-1))

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
