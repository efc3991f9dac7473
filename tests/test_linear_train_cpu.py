"""CPU: what the grad-mode Linear route rests on without a GPU - the fp64 reference of tests/_linear_train_cases.py against
autograd, the host's split rule, the module's CPU behaviour and the binding of the new entry."""
import pytest
import torch
from torch import nn

from tests import _linear_train_cases as lc


@pytest.mark.parametrize("shape", [(1, 4, 4), (33, 64, 36), (300, 132, 200)])
def test_reference_is_what_autograd_computes_through_f_linear(shape):
    case = lc.make_case(*shape)
    ref, auto = lc.reference(case), lc.autograd(case)
    for n in lc.OUTPUTS:
        assert ref[n].dtype == torch.float64 and ref[n].shape == auto[n].shape
        assert lc.rel_err(ref[n], auto[n]) < 1e-13, n
    for n in ("x", "grad_out", "weight", "bias"):
        assert torch.equal(case[n], case[n].float().double()), n          # fp32 numbers: the fp32 runs get the reference's inputs


def test_sequential_yardstick_is_the_reference_up_to_fp32_rounding():
    case = lc.make_case(300, 132, 200)
    ref = lc.reference(case)
    one, seven = lc.yardstick(case, 1), lc.yardstick(case, 7)
    for n in lc.OUTPUTS:
        assert 0 < lc.rel_err(one[n], ref[n]) < 1e-5 and lc.rel_err(seven[n], ref[n]) < 1e-5, n
    assert torch.equal(one["grad_x"], seven["grad_x"]) and not torch.equal(one["grad_w"], seven["grad_w"])


def test_split_rule_gives_whole_steps_and_no_empty_range():
    from dfx import ops
    rows = [1, 15, 16, 17, 300, 1200, 4200, 9600, 16800, 134400, 1_000_000, 40_000_000]
    for M in rows:
        for N in (4, 32, 64, 68, 128, 256, 1024):
            for K in (4, 128, 256, 1024, 4096):
                splits = ops._wgrad_splits(M, N, K)
                per, n = lc.ranges(M, splits)
                assert 1 <= splits <= 65535 and n == splits, (M, N, K, splits)      # what the library will run
                assert per % 16 == 0 and (splits - 1) * per < M <= splits * per, (M, N, K, splits, per)
                assert ops._wgrad_ranges(M, splits) == (per, n)
    # one resident round: 16 tiles of 128 x 128 leave 48 ranges; at least 16 steps each; at most 256 ranges
    assert ops._wgrad_splits(134400, 1024, 256) == 48 and ops._wgrad_splits(134400, 32, 256) == 255      # (256 asked for: ranges of 33 whole steps)
    assert ops._wgrad_splits(4200, 1024, 256) == 16 and ops._wgrad_splits(300, 256, 256) == 1
    assert ops._wgrad_splits(0, 256, 256) == 1
    # the clamp of a request: 63 steps cannot make 100 ranges
    assert lc.ranges(1000, 100) == (16, 63) and lc.ranges(1000, 7)[0] == 144


def test_cpu_linear_in_grad_mode_has_nn_linears_bits():
    from models.fused import Linear
    torch.manual_seed(3)
    mine = Linear(256, 64)
    plain = nn.Linear(256, 64)
    plain.load_state_dict(mine.state_dict())
    x = torch.randn(2, 45, 256)
    g = torch.randn(2, 45, 64)
    outs = []
    for m in (mine, plain):
        xi = x.clone().requires_grad_()
        y = m(xi)
        y.backward(g)
        outs.append((y.detach(), xi.grad, m.weight.grad, m.bias.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_new_entry_is_bound_with_its_13_arguments():
    from dfx import _lib
    assert len(_lib.SIGNATURES["dfx_gemm_wgrad_f32"]) == 13
    lib = _lib.load()
    assert hasattr(lib, "dfx_gemm_wgrad_f32") and lib.dfx_abi_version() == 5
