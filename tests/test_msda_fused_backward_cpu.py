"""CPU: the yardstick of the fused MSDA backward tests checks itself (the closed-form restatement against autograd through
the reference statement, fp64), the new entry point is declared and bound, and nothing of the new route runs on CPU tensors."""
import os
import re

import pytest
import torch

from tests import _msda_fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("levels,ref_dim,N,Lq", sorted({c[:4] for c in fc.OPERATOR_CASES}, key=str))
def test_restatement_equals_autograd_in_fp64(levels, ref_dim, N, Lq):
    """The formulas of csrc/msda_fused_backward.hip, written out, against autograd through softmax + the module's
    location arithmetic + ms_deform_attn_core_pytorch.  Also the builder's own assertions: every sample clear of a kink.
    (The strided operator cases are the same CPU tensors as a contiguous one: strides exist on the GPU side only.)"""
    case = fc.make_case(levels, ref_dim, N, Lq)
    assert case["noise"] < fc.MAX_COORD_NOISE
    auto, restated = fc.autograd_backward(case, torch.float64), fc.restated_backward(case)
    for k in fc.GRADS:
        assert restated[k].shape == auto[k].shape
        assert auto[k].abs().max() > 0, k
        err = fc.rel_err(restated[k], auto[k])
        print(f"  d{k}: restated against autograd {err:.3e} (coordinate noise of the case {case['noise']:.2e})")
        assert torch.allclose(restated[k], auto[k], rtol=1e-10, atol=1e-10 * auto[k].abs().max().item()), (k, err)


def test_cases_cover_inside_border_and_outside_samples():
    case = fc.make_case(4, 2, 2, 300)
    pix = fc.pixel_coordinates(case["ref"].double(), case["offsets"].double().view(2, 300, fc.M, 4, fc.P, 2), case["sizes"])
    for l, (H, W) in enumerate(case["sizes"]):
        x = pix[:, :, :, l, :, 0]
        assert ((x > 0) & (x < W - 1)).any() and ((x > -1) & (x < 0)).any() and ((x > W - 1) & (x < W)).any()
        assert (x < -1).any() and (x > W).any()


def test_header_declares_and_the_binding_covers_the_backward_entry():
    from dfx import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_msda.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dfx_msda_fused_backward_f32\s*\(", text)
    sig = _lib.SIGNATURES["dfx_msda_fused_backward_f32"]
    decl = re.search(r"dfx_msda_fused_backward_f32\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(sig) == len(decl.split(",")) == 24
    assert hasattr(_lib.load(), "dfx_msda_fused_backward_f32")


def test_ops_reject_cpu_tensors_like_the_reference():
    from dfx import ops
    case = fc.make_case(2, 2, 3, 37)
    args = (case["value"], case["shapes"], case["lsi"], case["ref"], case["offsets"], case["logits"])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_fused(*args, 2, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_fused(case["value"].requires_grad_(False), *args[1:4], case["offsets"].clone().requires_grad_(), case["logits"], 2, 4)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.msda_fused_backward(case["grad_out"], *args)


def test_module_on_the_cpu_never_takes_the_fused_training_branch(cpu_msda, monkeypatch):
    """Grad mode on CPU tensors: the reference's op sequence with MSDeformAttnFunction (here the CPU oracle), as before."""
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    from models.ops.modules import ms_deform_attn as mod

    def never(*a, **k):
        raise AssertionError("dfx.ops.msda_fused called on CPU tensors")

    calls = [0]
    real = f.MSDeformAttnFunction

    class Counting(real):
        @staticmethod
        def forward(ctx, *a):
            calls[0] += 1
            return real.forward(ctx, *a)

    monkeypatch.setattr(ops, "msda_fused", never)
    monkeypatch.setattr(f, "MSDeformAttnFunction", Counting)
    assert mod.MSDA_TRAIN
    torch.manual_seed(0)
    m = mod.MSDeformAttn(256, 2, 8, 4).train()
    shapes, lsi = fc.level_tensors(fc.LEVELS[2])
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    query = torch.randn(2, 5, 256, requires_grad=True)
    out = m(query, torch.rand(2, 5, 2, 2), torch.randn(2, S, 256), shapes, lsi)
    out.sum().backward()
    assert calls[0] == 1 and query.grad is not None


@pytest.mark.parametrize("what,text", [("level_start_index length", "level_start_index"), ("fp64 value", "float32"),
                                       ("int32 spatial_shapes", "int64"), ("3-d reference_points", "reference_points")])
def test_joint_and_split_form_reject_the_same_operands(what, text):
    """The operand contract is checked before placement, so CPU tensors reach it: each malformed operand is named by the
    forward on the joint row, the trainable form and the backward alike (well-formed CPU operands: the test above)."""
    from dfx import ops
    case = fc.make_case(2, 2, 3, 37)
    value, shapes, lsi, ref, offsets, logits = (case[k] for k in ("value", "shapes", "lsi", "ref", "offsets", "logits"))
    value, shapes, lsi, ref = {
        "level_start_index length": (value, shapes, torch.cat([lsi, lsi[-1:]]), ref),
        "fp64 value": (value.double(), shapes, lsi, ref),
        "int32 spatial_shapes": (value, shapes.int(), lsi, ref),
        "3-d reference_points": (value, shapes, lsi, ref[:, :, 0]),
    }[what]
    with pytest.raises(RuntimeError, match=text):
        ops.msda_fused(value, shapes, lsi, ref, offsets, logits, 2, 4)
    with pytest.raises(RuntimeError, match=text):
        ops.msda_fused_forward(value, shapes, lsi, ref, torch.cat([offsets, logits], -1), 2, 4)
    with pytest.raises(RuntimeError, match=text):
        ops.msda_fused_backward(case["grad_out"], value, shapes, lsi, ref, offsets, logits)
