"""Generate tests/golden/dformer_train.npz from the REFERENCE's own DFormerBackbone under one training pass.

Build container only (imports /root/reference through tools/ref_import.py; nothing of it is stored):
    python tools/gen_golden_dformer_train.py
Runs tests/_dformer_train_cases.run_stem on the reference's ``DFormerBackbone(train_backbone=True, freeze_batchnorm=False)`` in
train mode - weights filled by name (tests/_param_fill.py), depth input [2,1,64,96], loss (out * g).sum() with a seeded g -
once in fp64 (``ref.*``: the reference) and once in fp32 (``f32.*``: the yardstick), and stores the output, every parameter
gradient and the running statistics after the pass.  Neither weights nor inputs are stored: the test regenerates both.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()
import models.dformer_backbone as dfb  # noqa: E402
from util.misc import NestedTensor  # noqa: E402

from tests import _golden  # noqa: E402
from tests._dformer_train_cases import run_stem  # noqa: E402
from tests._param_fill import fill_params_by_name  # noqa: E402

blobs = {}
for tag, dtype in (("ref", torch.float64), ("f32", torch.float32)):
    _, res = run_stem(dfb.DFormerBackbone, NestedTensor, fill_params_by_name, dtype)
    blobs.update({f"{tag}.{k}": v.numpy() for k, v in res.items()})
_golden.save(os.path.join(ROOT, "tests", "golden"), "dformer_train", blobs)
print("wrote tests/golden/dformer_train*.npz:", len(blobs), "arrays,", sum(v.nbytes for v in blobs.values()), "bytes")
