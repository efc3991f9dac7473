"""CPU: what the fused attention backward's GPU tests stand on (tests/_mha_cases.py) and the host logic of the grad-mode
route of models/fused_mha.py that needs no GPU."""
import copy

import pytest
import torch
from torch import nn

from tests import _mha_cases as mc


@pytest.mark.parametrize("shape,p", [((2, 8, 33, 31), 0.0), ((1, 2, 65, 97), mc.DROP_P), ((2, 8, 1, 1), mc.DROP_P)])
def test_restated_backward_equals_fp64_autograd(shape, p):
    """delta, dP, dS, dV, dQ, dK as the kernel computes them against autograd through softmax(...) * drop @ v, in fp64."""
    case = mc.make_case(*shape, p=p)
    want, got = mc.autograd(case), mc.restated(case)
    for name in mc.OUTPUTS:
        err = mc.rel_err(got[name], want[name])
        print(f"  {name}: {err:.3e}")
        assert err < 1e-13, name


def test_restated_lse_is_the_natural_log_sum_exp():
    case = mc.make_case(1, 2, 5, 7)
    q, k = case["q"].view(1, 5, 2, 32), case["k"].view(1, 7, 2, 32)
    s = case["scale"] * torch.einsum("bihd,bjhd->bhij", q, k)
    assert torch.allclose(mc.restated(case)["lse"], s.exp().sum(-1).log(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("self_attention", [True, False])
def test_mask_helper_reproduces_the_module_in_train_mode(self_attention):
    """nn.MultiheadAttention(dropout=0.2).train() under a fixed seed against the restatement with the mask that
    ``attention_dropout_mask`` draws under the same seed: the helper's draw is the module's own."""
    from models import fused_mha
    torch.manual_seed(5)
    mha = nn.MultiheadAttention(256, 8, dropout=0.2).train()
    B, Lq, Lk = 2, 30, 30 if self_attention else 45
    q_in = torch.randn(B, Lq, 256)
    k_in = q_in if self_attention else torch.randn(B, Lk, 256)
    v_in = torch.randn(B, Lk, 256)
    torch.manual_seed(11)
    want = mha(q_in.transpose(0, 1), k_in.transpose(0, 1), v_in.transpose(0, 1))[0].transpose(0, 1)
    torch.manual_seed(11)
    mask = fused_mha.attention_dropout_mask(mha, B, Lq, Lk, q_in.device)
    assert mask.shape == (B * 8, Lq, Lk) and set(mask.unique().tolist()) == {0.0, 1.25}
    got = mc.module_reference(mha, q_in, k_in, v_in, mask, torch.float32)
    err = (got - want).abs().max().item()
    print(f"  module against the restatement with the helper's mask: {err:.3e}")
    assert err <= 2e-7                  # two fp32 evaluations of the same sums on outputs of order 0.1: a few ulps
    # another seed is another mask: the agreement above is not an accident of a mask that does nothing
    torch.manual_seed(12)
    other = mc.module_reference(mha, q_in, k_in, v_in, fused_mha.attention_dropout_mask(mha, B, Lq, Lk, q_in.device), torch.float32)
    assert (other - want).abs().max().item() > 1e-3


def test_no_mask_without_dropout_or_in_eval_mode():
    from models import fused_mha
    plain, evaluating = nn.MultiheadAttention(256, 8, dropout=0.0).train(), nn.MultiheadAttention(256, 8, dropout=0.2).eval()
    state = torch.random.get_rng_state()
    assert fused_mha.attention_dropout_mask(plain, 2, 3, 4, "cpu") is None
    assert fused_mha.attention_dropout_mask(evaluating, 2, 3, 4, "cpu") is None
    assert torch.equal(torch.random.get_rng_state(), state), "a module that does not drop must not draw"


def test_usable_is_false_for_cpu_tensors_in_grad_mode():
    from models import fused_mha
    mha = nn.MultiheadAttention(256, 8)
    x = torch.randn(2, 5, 256)
    assert torch.is_grad_enabled() and fused_mha.MHA_TRAIN
    assert not fused_mha.usable(mha, x, x, x)
    with torch.no_grad():
        assert not fused_mha.usable(mha, x, x, x)


def test_cpu_modules_keep_the_module_route_in_grad_mode():
    """_mha on CPU tensors in grad mode is the module call: same bits, gradients flow."""
    from models.transformer_layers import _mha
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(256, 8, dropout=0.0).train()
    x = torch.randn(2, 6, 256, requires_grad=True)
    got = _mha(mha, x, x, x)
    want = copy.deepcopy(mha)(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1))[0].transpose(0, 1)
    assert torch.equal(got, want) and got.grad_fn is not None


def test_ops_mha_rejects_cpu_tensors():
    from dfx import ops
    x = torch.randn(1, 4, 256)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.mha(x, x, x, 8, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.mha_backward(x, x, x, x, x, torch.zeros(1, 8, 4), 8, 1.0)
