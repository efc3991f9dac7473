"""Generate tests/golden/criterion.npz from the REFERENCE's own SetCriterion + HungarianMatcher.

Build container only (imports the reference through tools/ref_import.py and needs scipy, which the reference's matcher
imports; nothing of either is stored):
    python tools/gen_golden_criterion.py
Runs the reference's ``SetCriterion(3, HungarianMatcher(2, 5, 2), weight_dict, ['labels', 'boxes', 'cardinality'])`` on every
case of tests/_criterion_cases.py, once in fp64 (``ref.*``: the reference) and once in fp32 (``f32.*``: the yardstick), and
stores per case the ordered loss keys, every loss value, the assignment of every set and the gradients of
sum(weight_dict[k] * loss[k]) with respect to every set's logits and boxes, plus the seed used.  Inputs are not stored.

The seed rule (tests/_criterion_cases.py): the first seed from the case's base seed for which the fp64 and fp32 assignments
agree for every set and still agree under 16 seeded relative perturbations of 1e-4 of the fp64 cost matrices.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()
import models.deformable_detr_multi_plusplus as multipp  # noqa: E402
import models.matcher as ref_matcher  # noqa: E402

from tests import _criterion_cases as cc  # noqa: E402
from tests import _golden  # noqa: E402

_solve = ref_matcher.linear_sum_assignment
_seen = []                                     # every cost block the reference's matcher hands to scipy, in call order


def _recording_solve(block):
    _seen.append(torch.as_tensor(block).double().numpy().copy())
    return _solve(block)


ref_matcher.linear_sum_assignment = _recording_solve


def criterion(case):
    return multipp.SetCriterion(cc.NUM_CLASSES, ref_matcher.HungarianMatcher(**cc.COST), cc.weight_dict(case), cc.LOSSES)


def stable(name, seed):
    """-> {tag: (losses, grads, assignments)} when the reference's assignment is stable on this seed, else None"""
    case = cc.CASES[name]
    inputs = cc.make_inputs(name, seed)
    res = {}
    for tag, dtype in (("ref", torch.float64), ("f32", torch.float32)):
        crit = criterion(case)
        del _seen[:]
        assign = cc.assignments(name, inputs, crit.matcher, dtype)
        blocks = list(_seen)
        losses, grads = cc.run(name, inputs, crit, dtype)
        res[tag] = (losses, grads, assign, blocks)
    if any(not np.array_equal(res["ref"][2][n], res["f32"][2][n]) for n in res["ref"][2]):
        return None
    rng = np.random.default_rng(seed)
    for block in res["ref"][3]:
        want = _solve(block)
        for _ in range(cc.N_PERTURB):
            got = _solve(block * (1.0 + cc.PERTURB * rng.uniform(-1.0, 1.0, size=block.shape)))
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                return None
    return res


blobs = {}
for name, case in cc.CASES.items():
    for seed in range(case["base_seed"], case["base_seed"] + cc.MAX_SEEDS):
        res = stable(name, seed)
        if res is not None:
            break
    else:
        raise AssertionError(f"{name}: no seed in {case['base_seed']}..{case['base_seed'] + cc.MAX_SEEDS - 1} has a stable assignment")
    blobs[f"{name}.seed"] = np.asarray(seed, dtype=np.int64)
    for tag, (losses, grads, assign, _) in res.items():
        blobs[f"{tag}.{name}.keys"] = np.asarray(list(losses))
        for k, v in losses.items():
            blobs[f"{tag}.{name}.loss.{k}"] = v.numpy()
        for k, v in grads.items():
            blobs[f"{tag}.{name}.{k}"] = v.numpy()
        for n, a in assign.items():
            blobs[f"{tag}.{name}.assign.{n}"] = a
    print(f"{name}: seed {seed}, keys {list(res['ref'][0])}")
_golden.save(os.path.join(ROOT, "tests", "golden"), "criterion", blobs)
print("wrote tests/golden/criterion.npz:", len(blobs), "arrays,", sum(v.nbytes for v in blobs.values()), "bytes")
