"""CPU: the fp64 reference and the fp32 yardstick of tests/_dformer_train_cases.py hold together, the yardstick sits where
fp32 arithmetic puts it, the route's plumbing (ABI, front ends, switch, size rule) exists, and the golden fixture of the whole
stem is what the generator says it is.  No GPU: the operators themselves are checked in tests/test_dformer_train_gpu.py."""
import os

import pytest
import torch

from tests import _dformer_train_cases as dc
from tests import _golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("y", "mean", "rstd", "grad_x", "grad_gamma", "grad_beta", "running_mean", "running_var", "running_mean2", "running_var2")


@pytest.mark.parametrize("gelu", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("name", list(dc.BN_CASES))
def test_closed_form_is_what_autograd_computes_in_fp64(name, gelu):
    case, ref, _ = dc.bn_prepared(name, gelu)
    closed = dc.bn_closed_form(case, gelu)
    for n in NAMES:
        # ("two_values" and "large_mean" cancel in grad_x: eight digits of the fp64 sums are gone there)
        assert dc.rel_err(closed[n], ref[n]) < 1e-9, n


@pytest.mark.parametrize("gelu", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("name", list(dc.BN_CASES))
def test_yardstick_sits_within_fp32_expectations(name, gelu):
    """fp32 autograd against fp64: a few units of 2^-24 times sqrt(values per channel) where nothing cancels; where
    |mean| / std = 1e5 ("large_mean") the centred values carry only 24 - 17 bits, and two values per channel cancel in dx"""
    case, ref, yard = dc.bn_prepared(name, gelu)
    N, C, H, W = case["shape"]
    eps = 2.0 ** -24
    bound = 16 * eps * max(1.0, (N * H * W) ** 0.5)
    if name == "large_mean":
        bound = 16 * eps * 1e5
    for n in NAMES:
        err = dc.rel_err(yard[n], ref[n])
        assert err > 0 or name == "two_values", f"{n}: a yardstick without error bounds nothing"
        if name == "two_values" and n == "grad_x":
            assert err < 0.1
        else:
            assert err < bound, (n, err, bound)


def test_large_mean_case_defeats_the_naive_variance():
    case, ref, yard = dc.bn_prepared("large_mean", False)
    naive = (dc.naive_variance_f32(case).double().clamp_min(0) + dc.BN_EPS).rsqrt()
    assert dc.rel_err(naive, ref["rstd"]) > 100 * dc.YARDSTICK_FACTOR * dc.rel_err(yard["rstd"], ref["rstd"])


def test_cases_cover_the_kernels_paths():
    hw = {n: s[2] * s[3] for n, s in dc.BN_CASES.items()}
    assert any(v % 4 for v in hw.values()) and any(v % 4 == 0 and v % 64 for v in hw.values())          # scalar and 16-byte paths
    assert any(v > dc.CHUNK and v % dc.CHUNK for v in hw.values())                                      # several chunks, ragged
    assert any(v > dc.CHUNK and v % 4 for v in hw.values())                                             # ... on the scalar path
    assert dc.BN_CASES["two_values"][0] * hw["two_values"] == 2
    chunks = {n: s[0] * -(-hw[n] // dc.CHUNK) for n, s in dc.BN_CASES.items()}
    assert any(v > dc.BWD_MAX_GROUPS and v % 2 for v in chunks.values())                               # grouped backward sums, ragged
    assert f"#define DFX_BN_BWD_MAX_GROUPS {dc.BWD_MAX_GROUPS}\n" in open(os.path.join(ROOT, "include", "dfx_fused.h")).read()
    from dfx import ops
    assert ops.BN_CHUNK_PIXELS == dc.CHUNK
    header = open(os.path.join(ROOT, "include", "dfx_fused.h")).read()
    assert f"#define DFX_BN_CHUNK_PIXELS {dc.CHUNK}\n" in header


def test_front_ends_switch_and_size_rule_exist():
    from dfx import _lib, ops
    from models import dformer_backbone, fused
    for name in ("dfx_batch_norm_train_f32", "dfx_batch_norm_backward_f32"):
        assert name in _lib.SIGNATURES
    for name in ("batch_norm_train_forward", "batch_norm_backward", "batch_norm_train", "batch_norm_train_supported"):
        assert callable(getattr(ops, name))
    assert isinstance(fused.DFORMER_TRAIN, bool) and isinstance(fused.DFORMER_TRAIN_MIN_PIXELS, int) and isinstance(fused.DFORMER_TRAIN_MIN_PIXELS_GELU, int)
    assert callable(dformer_backbone._run_stage_train)


def test_cpu_tensors_keep_the_modules_and_the_operator_refuses_them(monkeypatch):
    from torch import nn
    from dfx import ops
    from models import fused
    from models.dformer_backbone import DFormerBackbone
    from util.misc import NestedTensor
    monkeypatch.setattr(fused, "DFORMER_TRAIN", True)            # (the device check is what keeps the modules here)
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS", 0)
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS_GELU", 0)
    bn = nn.BatchNorm2d(4).train()
    with pytest.raises(RuntimeError, match="CPU"):
        ops.batch_norm_train(torch.randn(2, 4, 3, 3), bn)
    net = DFormerBackbone(train_backbone=True, freeze_batchnorm=False).train()
    called = []
    real = ops.batch_norm_train
    ops.batch_norm_train = lambda *a, **k: called.append(1) or real(*a, **k)
    try:
        out = net(NestedTensor(torch.randn(2, 1, 32, 32), torch.zeros(2, 32, 32, dtype=torch.bool)))["0"].tensors
    finally:
        ops.batch_norm_train = real
    assert not called and out.shape == (2, 128, 2, 2) and out.grad_fn is not None


def test_supported_is_a_training_mode_affine_batchnorm_with_a_float_momentum():
    from torch import nn
    from dfx import ops
    assert ops.batch_norm_train_supported(nn.BatchNorm2d(4).train())
    assert ops.batch_norm_train_supported(nn.BatchNorm2d(4, track_running_stats=False).train())
    assert not ops.batch_norm_train_supported(nn.BatchNorm2d(4).eval())
    assert not ops.batch_norm_train_supported(nn.BatchNorm2d(4, affine=False).train())
    assert not ops.batch_norm_train_supported(nn.BatchNorm2d(4, momentum=None).train())
    assert not ops.batch_norm_train_supported(nn.SyncBatchNorm(4).train())
    assert not ops.batch_norm_train_supported(nn.BatchNorm2d(4).double().train())


def test_golden_fixture_holds_the_reference_and_its_fp32_yardstick():
    """tests/golden/dformer_train*.npz (tools/gen_golden_dformer_train.py): the same names under ``ref.`` (fp64) and ``f32.``;
    this repository's module reproduces the fp64 pass on the CPU from the same fill and input"""
    from models.dformer_backbone import DFormerBackbone
    from tests._param_fill import fill_params_by_name
    from util.misc import NestedTensor
    gold = _golden.load(os.path.join(ROOT, "tests", "golden"), "dformer_train")
    ref = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("ref.")}
    f32 = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("f32.")}
    assert set(ref) == set(f32) and "out" in ref and ref["out"].dtype == torch.float64 and f32["out"].dtype == torch.float32
    net, mine = dc.run_stem(DFormerBackbone, NestedTensor, fill_params_by_name, torch.float64)
    assert set(mine) == set(ref), "state_dict keys or trained parameters differ from the reference's"
    assert not any(n.startswith("grad.depth_backbone.downsample_layers_e.3") for n in ref), "the fourth stage is never run"
    for n, want in ref.items():
        if n in dc.STEM_ZERO_GRADS:           # a bias in front of a BatchNorm with batch statistics: rounding noise around zero
            assert want.abs().max() < 1e-12 and f32[n].abs().max() < 1e-3, n
        elif want.is_floating_point():
            assert dc.rel_err(mine[n], want) < 1e-12, n
            assert dc.rel_err(f32[n], want) < (1e-4 if want.abs().max() > 1e-2 else 0.1), n
        else:
            assert torch.equal(mine[n], want), n
