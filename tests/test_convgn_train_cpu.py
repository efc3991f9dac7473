"""CPU: what the grad-mode route of the input projections and the frozen-part routing rest on without a GPU - the fp64
reference of tests/_convgn_cases.py against its closed form, the host's range rule, the truth table of
``models.fused.needs_grad``, the module's CPU behaviour and the binding of the two new entries."""
import os
import re

import pytest
import torch
from torch import nn

from tests import _convgn_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", [(1, 4, 4, 2, 2), (3, 8, 12, 3, 4), (2, 16, 8, 5, 4)])
def test_conv_reference_is_the_closed_form(shape):
    case = cc.make_conv_case(*shape)
    ref, closed = cc.conv_reference(case), cc.conv_closed_form(case)
    for n in cc.CONV_OUTPUTS:
        assert ref[n].dtype == torch.float64 and ref[n].shape == closed[n].shape, n
        assert cc.rel_err(closed[n], ref[n]) < 1e-13, n
    for n in ("x", "grad_out", "weight", "bias"):
        assert torch.equal(case[n], case[n].float().double()), n          # fp32 numbers: the fp32 runs get the reference's inputs


@pytest.mark.parametrize("shape", cc.GN_SHAPES[:3], ids=lambda s: "x".join(str(v) for v in s))
def test_group_norm_reference_is_the_closed_form_of_the_header(shape):
    case = cc.make_gn_case(*shape)
    ref, closed = cc.gn_reference(case), cc.gn_closed_form(case)
    for n in cc.GN_OUTPUTS + ("y",):
        assert ref[n].dtype == torch.float64 and ref[n].shape == closed[n].shape, n
        assert cc.rel_err(closed[n], ref[n]) < 1e-12, n
    yard = cc.gn_yardstick(case)
    for n in cc.GN_OUTPUTS:
        assert yard[n].dtype == torch.float32 and 0 < cc.rel_err(yard[n], ref[n]) < 1e-5, n


def test_sequential_conv_yardstick_is_the_reference_up_to_fp32_rounding():
    case = cc.make_conv_case(3, 16, 8, 13, 20)
    ref = cc.conv_reference(case)
    one, seven = cc.conv_yardstick(case, 1), cc.conv_yardstick(case, 7)
    for n in cc.CONV_OUTPUTS:
        assert one[n].shape == ref[n].shape
        assert 0 < cc.rel_err(one[n], ref[n]) < 1e-5 and cc.rel_err(seven[n], ref[n]) < 1e-5, n
    assert torch.equal(one["grad_x"], seven["grad_x"]) and not torch.equal(one["grad_w"], seven["grad_w"])


def test_range_rule_gives_whole_steps_no_empty_range_and_stays_within_its_limits():
    from dfx import ops
    for batch in (1, 2, 3, 4, 32, 300):
        for HW in (4, 16, 20, 260, 1024, 4200, 16800, 1_000_000):
            for Co in (4, 64, 256):
                for Ci in (4, 128, 256, 2048):
                    splits = ops._conv1x1_wgrad_splits(Co, Ci, HW, batch)
                    per, n = cc.ranges(HW, splits)
                    assert splits >= 1 and n == splits, (Co, Ci, HW, batch, splits)                  # what the library will run
                    assert per % 16 == 0 and (splits - 1) * per < HW <= splits * per, (Co, Ci, HW, batch, splits, per)
                    if splits > 1:
                        tiles = -(-Ci // 128) * (1 if Co <= 64 else -(-Co // 128))
                        assert per >= 16 * ops._WGRAD_MIN_STEPS                                      # the minimum range length
                        assert batch * splits <= ops._WGRAD_MAX_RANGES                               # the range limit
                        assert tiles * batch * splits <= (1024 if Co <= 64 else 768)                 # one resident round
    # the two projections at 4 frames of 50 x 84: 32 tiles x 4 images leave 6 ranges; 2 tiles: at least 16 steps per range
    assert ops._conv1x1_wgrad_splits(256, 2048, 4200, 4) == 6 and ops._conv1x1_wgrad_splits(256, 128, 4200, 4) == 16
    assert ops._conv1x1_wgrad_splits(4, 4, 4, 1) == 1 and ops._conv1x1_wgrad_splits(256, 128, 260, 3) == 1
    assert ops._conv1x1_wgrad_splits(256, 128, 0, 2) == 1 and ops._conv1x1_wgrad_splits(256, 128, 4200, 0) == 1


def test_needs_grad_truth_table():
    from models.fused import needs_grad
    m = nn.Sequential(nn.Conv2d(4, 4, 1), nn.GroupNorm(2, 4))
    x, xg = torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2, requires_grad=True)
    assert needs_grad(m) and needs_grad(m, x) and needs_grad(m.parameters(), x)
    with torch.no_grad():
        assert not needs_grad(m, xg)
    for p in m.parameters():
        p.requires_grad_(False)
    assert not needs_grad(m) and not needs_grad(m, x) and not needs_grad(m, x, None) and not needs_grad([], x)
    assert needs_grad(m, xg) and needs_grad(m, x, xg) and needs_grad([], xg)
    m[1].bias.requires_grad_(True)
    assert needs_grad(m, x) and needs_grad([m[1].bias]) and not needs_grad(m[0], x) and not needs_grad(list(m[0].parameters()))
    with torch.no_grad():
        assert not needs_grad(m, x)
    derived = xg * 2                                   # a tensor with a grad_fn asks as a leaf does
    assert needs_grad(m[0], derived) and not needs_grad(m[0], derived.detach())


def test_cpu_convgn_in_grad_mode_is_still_nn_sequential():
    from models.detector_common import _conv_gn
    torch.manual_seed(2)
    mine = _conv_gn(8, 32)
    plain = nn.Sequential(nn.Conv2d(8, 32, 1), nn.GroupNorm(32, 32))
    plain.load_state_dict(mine.state_dict())
    x, g = torch.randn(2, 8, 3, 4), torch.randn(2, 32, 3, 4)
    outs = []
    for m in (mine, plain):
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.backward(g)
        outs.append([y.detach(), xi.grad] + [p.grad for p in m.parameters()])
    assert "GroupNormFunction" not in type(y.grad_fn).__name__ and len(outs[0]) == 6
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for p in mine.parameters():
        p.requires_grad_(False)
    assert torch.equal(mine(x), outs[1][0]) and mine(x).grad_fn is None        # frozen on the CPU: the modules all the same


def test_new_entries_are_declared_in_their_headers_and_bound():
    from dfx import _lib
    for header, name, nargs in (("dfx_gemm.h", "dfx_conv1x1_wgrad_f32", 12), ("dfx_fused.h", "dfx_group_norm_backward_f32", 14)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl is not None, f"{name} is not declared in include/{header}"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name)
    from dfx import ops
    assert re.search(r"#define\s+DFX_GN_BWD_CHUNKS\s+%d\b" % ops.GN_BWD_CHUNKS, open(os.path.join(ROOT, "include", "dfx_fused.h")).read())
    from models import fused
    assert fused.CONVGN_TRAIN is True
