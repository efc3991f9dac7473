"""CPU: the yardstick of the single-level MSDA backward tests checks itself (the builder's fp64 restated grad_value against
fp64 autograd), the host decision ``dfx.ops.level_backward_supported`` and the declaration and binding of the new entry."""
import os
import re

import pytest
import torch

from tests import _msda_fused_cases as fc
from tests import _msda_level_bwd_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_restated_grad_value_equals_autograd_in_fp64(ref_dim):
    case = lc.make_level_case(5, 7, ref_dim, 3, 37)
    assert case["noise"] < fc.MAX_COORD_NOISE and case["value"].shape == (3, 35, 8, 32)
    auto, restated = fc.autograd_backward(case, torch.float64)["value"], fc.restated_backward(case)["value"]
    assert auto.abs().max() > 0
    err = fc.rel_err(restated, auto)
    print(f"  dvalue: restated against autograd {err:.3e} (coordinate noise of the case {case['noise']:.2e})")
    assert err < 1e-12
    want, _ = lc.references(5, 7, ref_dim, 3, 37)
    assert torch.equal(want, restated)


def test_colliding_case_gives_every_query_the_same_samples():
    case = lc.make_level_case(20, 31, 2, 1, 1100, True)
    assert (case["ref"] == case["ref"][:, :1]).all() and (case["offsets"] == case["offsets"][:, :1]).all()
    assert not (case["grad_out"] == case["grad_out"][:, :1]).all()


def test_level_backward_supported_is_a_host_decision(monkeypatch):
    from dfx import ops
    assert ops.USE_LEVEL_BWD == (os.environ.get("DFX_MSDA_LEVEL_BWD", "1") != "0")
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", True)
    assert ops.level_backward_supported(1, 50, 84, 4, 4200)
    assert not ops.level_backward_supported(2, 50, 84, 4, 4200)              # two levels
    assert not ops.level_backward_supported(1, 60, 100, 4, 4200)             # does not fit the LDS image
    assert ops.LEVEL_BWD_MIN_QUERIES > 1
    assert not ops.level_backward_supported(1, 50, 84, 1, ops.LEVEL_BWD_MIN_QUERIES - 1)      # below the threshold
    assert ops.level_backward_supported(1, 50, 84, 1, ops.LEVEL_BWD_MIN_QUERIES)
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", False)
    assert not ops.level_backward_supported(1, 50, 84, 4, 4200)              # the switch


def test_header_declares_and_the_binding_covers_the_entry():
    from dfx import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_msda.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dfx_msda_level_grad_value_f32\s*\(", text)
    sig = _lib.SIGNATURES["dfx_msda_level_grad_value_f32"]
    decl = re.search(r"dfx_msda_level_grad_value_f32\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(sig) == len(decl.split(",")) == 13
    assert hasattr(_lib.load(), "dfx_msda_level_grad_value_f32")


def test_front_end_rejects_cpu_tensors_and_malformed_operands():
    from dfx import ops
    case = lc.make_level_case(5, 7, 2, 3, 37)
    go, ref, off, lg = (case[k] for k in ("grad_out", "ref", "offsets", "logits"))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_level_grad_value(go, ref, off, lg, 3, 5, 7)
    with pytest.raises(RuntimeError, match="offsets"):
        ops.msda_level_grad_value(go, ref, off[..., :60], lg, 3, 5, 7)
    with pytest.raises(RuntimeError, match="float32"):
        ops.msda_level_grad_value(go.double(), ref, off, lg, 3, 5, 7)
    with pytest.raises(RuntimeError, match="reference_points"):
        ops.msda_level_grad_value(go, ref[:, :, 0], off, lg, 3, 5, 7)
