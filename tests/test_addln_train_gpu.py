"""GPU: dfx.ops.add_layernorm_train - norm(residual + dropout(x)) forward and backward on csrc/layernorm_train.hip - against
the inference entry (bit for bit), the fp64 CPU autograd of tests/_addln_cases.py (within the project's yardstick rule) and
the module chain nn.Dropout + add + nn.LayerNorm (the same dropout draw)."""
import itertools

import pytest
import torch
from torch import nn

from tests import _addln_cases as ac

pytestmark = pytest.mark.gpu

GRADS = ac.OUTPUTS[1:]


def _norm(case):
    C = case["gamma"].numel()
    norm = nn.LayerNorm(C, eps=ac.EPS).cuda()
    with torch.no_grad():
        norm.weight.copy_(case["gamma"])
        norm.bias.copy_(case["beta"])
    return norm


def _gpu(case):
    return {k: None if v is None else v.cuda() for k, v in case.items()}


def _run(case, **need):
    """(out, keep, {gradient name: tensor | None}) of the forward entry and the backward entry"""
    from dfx import ops
    t = _gpu(case)
    out, s, mean, rstd, keep = ops.add_layernorm_train_forward(t["x"], t["residual"], t["gamma"], t["beta"], ac.EPS, t["mask"])
    need.setdefault("need_residual", case["residual"] is not None)
    got = ops.add_layernorm_backward(t["grad_out"], s, mean, rstd, t["gamma"], keep, 1 / (1 - ac.P), **need)
    torch.cuda.synchronize()
    return out, keep, dict(zip(GRADS, got))


def _compare(ref, yard, got, what):
    worst = []
    for n in ref:
        y, err = ac.rel_err(yard[n], ref[n]), ac.rel_err(got[n].cpu(), ref[n])
        print(f"  {what} {n}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}, "
              f"max |ref| {ref[n].abs().max().item():.3e}")
        assert got[n].shape == ref[n].shape and torch.isfinite(got[n]).all(), n
        if not err <= ac.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {ac.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


@pytest.mark.parametrize("C", ac.COLS)
@pytest.mark.parametrize("rows", ac.ROWS)
def test_forward_bits_backward_accuracy_and_switched_off_gradients(rows, C):
    from dfx import ops
    for residual, mask in itertools.product((True, False), (True, False)):
        case, ref, yard = ac.prepared(rows, C, residual, mask)
        what = f"rows {rows} C {C} residual {int(residual)} mask {int(mask)}"
        t, norm = _gpu(case), _norm(case)
        out, keep, got = _run(case)
        # forward: the inference entry's bits, on x * mask with a mask; the keep bytes are the mask's non-zeros
        want = ops.add_layernorm(t["x"] if not mask else t["x"] * t["mask"], t["residual"], norm)
        assert torch.equal(out, want), what
        if mask:
            assert keep.dtype == torch.uint8 and torch.equal(keep != 0, t["mask"] != 0), what
        else:
            assert keep is None
            if residual:
                assert got["grad_x"] is got["grad_residual"], what
        if not residual:
            assert got.pop("grad_residual") is None
        _compare(ref, yard, dict(got, out=out), what)
        # a second call gives the same bits
        again = _run(case)[2]
        for n in got:
            assert torch.equal(again[n], got[n]), (what, n)
        # every gradient switched off in turn: None, and the others keep their bits
        for off in got:
            part = _run(case, **{"need_" + off[5:]: False})[2]
            assert part[off] is None, (what, off)
            for n in got:
                if n != off:
                    assert torch.equal(part[n], got[n]), (what, off, n)
        # dy = 0: exact zeros everywhere
        zero = _run(dict(case, grad_out=torch.zeros_like(case["grad_out"])))[2]
        for n in got:
            assert not zero[n].any(), (what, n)


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
def test_permuting_the_rows_permutes_the_row_gradients_bit_for_bit(mask):
    case = ac.make_case(67, 260, True, mask)
    perm = torch.randperm(67, generator=torch.Generator().manual_seed(3))
    moved = {k: v[perm] if v is not None and v.dim() == 2 else v for k, v in case.items()}
    got, got_moved = _run(case)[2], _run(moved)[2]
    for n in ("grad_x", "grad_residual"):
        assert torch.equal(got[n][perm.cuda()], got_moved[n]), n


def test_zero_gamma_column_and_constant_row_stay_finite_and_accurate():
    """gamma[c] = 0 for two columns; row 2 constant (variance 0 - the values and their sum are exact in fp32, so every
    arithmetic sees the same zero variance) with and without a mask."""
    for mask in (False, True):
        case = ac.make_case(5, 260, True, mask, seed=7)
        case["gamma"][3] = 0
        case["gamma"][257] = 0
        case["x"][2] = 0.25
        case["residual"][2] = 0.25
        if mask:
            case["mask"][2] = 1 / (1 - ac.P)
            case["x"][2] = 0.375                  # x * mask = 0.5 exactly
        out, _, got = _run(case)
        _compare(ac.autograd(case, torch.float64), ac.autograd(case, torch.float32), dict(got, out=out), f"edge mask {int(mask)}")


def test_non_contiguous_operands_are_accepted():
    from dfx import ops
    case = ac.make_case(17, 64)
    t, norm = _gpu(case), _norm(case)
    x = t["x"].t().contiguous().t().requires_grad_()               # column-major
    r = torch.cat([t["residual"], t["residual"]], 1)[:, ::2].requires_grad_()     # every second column of a wider tensor
    assert not x.is_contiguous() and not r.is_contiguous()
    xc, rc = x.detach().contiguous().requires_grad_(), r.detach().contiguous().requires_grad_()
    go = t["grad_out"].t().contiguous().t()
    got = torch.autograd.grad(ops.add_layernorm_train(x, r, norm), [x, r, norm.weight], go)
    want = torch.autograd.grad(ops.add_layernorm_train(xc, rc, norm), [xc, rc, norm.weight], go.contiguous())
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from dfx import ops
    launches = []
    monkeypatch.setattr(ops, "_call", lambda *a: launches.append(a))
    norm = nn.LayerNorm(64).cuda()
    x = torch.randn(5, 64, device="cuda")
    bad = [(x.cpu(), None, norm), (x.double(), None, norm), (x, x[:4], norm), (x, x.cpu(), norm), (x[:, :60], None, norm),
           (torch.randn(5, 6, device="cuda"), None, nn.LayerNorm(6).cuda()),
           (torch.randn(2, 1028, device="cuda"), None, nn.LayerNorm(1028).cuda()),
           (x, None, nn.LayerNorm(64, elementwise_affine=False).cuda()), (x, None, nn.LayerNorm(64).double().cuda())]
    for xx, rr, nn_ in bad:
        with pytest.raises(RuntimeError):
            ops.add_layernorm_train(xx, rr, nn_)
    s, mean, keep = torch.empty_like(x), torch.empty(5, device="cuda"), torch.empty(5, 64, dtype=torch.uint8, device="cuda")
    for args in ((x[:4], s, mean, mean, norm.weight), (x, s, mean[:4], mean, norm.weight), (x, s, mean, mean, norm.weight, keep.float()),
                 (x, s, mean, mean, norm.weight, keep[:4]), (x, s.cpu(), mean, mean, norm.weight)):
        with pytest.raises(RuntimeError):
            ops.add_layernorm_backward(*args)
    assert not launches


def test_no_node_without_something_to_differentiate():
    from dfx import ops
    norm = nn.LayerNorm(64).cuda().requires_grad_(False)
    x, r = torch.randn(5, 64, device="cuda"), torch.randn(5, 64, device="cuda")
    out = ops.add_layernorm_train(x, r, norm)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, ops.add_layernorm(x, r, norm))
    with torch.no_grad():
        assert ops.add_layernorm_train(x.requires_grad_(), r, norm).grad_fn is None
    tracked = ops.add_layernorm_train(x, r, norm)
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), out)
    gx, = torch.autograd.grad(tracked.sum(), [x])        # frozen norm, residual without a gradient: only grad_x is made
    assert gx.shape == x.shape


def test_dropout_draw_is_the_modules_own():
    """Under one seed the fused entry and norm(r + drop(x)) drop the same elements (2e-5; another mask differs at order 1)
    and leave the generator in the same state."""
    from dfx import ops
    case = ac.make_case(67, 256)
    t, norm = _gpu(case), _norm(case)
    drop = nn.Dropout(0.2).train()
    x = t["x"].reshape(1, 67, 256)
    r = t["residual"].reshape(1, 67, 256)
    torch.manual_seed(11)
    got = ops.add_layernorm_train(x, r, norm, drop)
    state_fused = torch.cuda.get_rng_state()
    torch.manual_seed(11)
    want = norm(r + drop(x))
    state_module = torch.cuda.get_rng_state()
    assert (got - want).abs().max().item() <= 2e-5
    assert torch.equal(state_fused, state_module)
    # an identity dropout (eval mode, p = 0) draws nothing
    for idle in (nn.Dropout(0.2).eval(), nn.Dropout(0.0).train()):
        assert torch.equal(ops.add_layernorm_train(x, r, norm, idle), ops.add_layernorm(x, r, norm))
        assert torch.equal(torch.cuda.get_rng_state(), state_module)
    # gradients through the drawn mask against the module chain under the same seed
    leaves = [x.clone().requires_grad_(), r.clone().requires_grad_()]
    torch.manual_seed(12)
    g1 = torch.autograd.grad(ops.add_layernorm_train(leaves[0], leaves[1], norm, drop), leaves + list(norm.parameters()), t["grad_out"].reshape(1, 67, 256))
    torch.manual_seed(12)
    g2 = torch.autograd.grad(norm(leaves[1] + drop(leaves[0])), leaves + list(norm.parameters()), t["grad_out"].reshape(1, 67, 256))
    for a, b in zip(g1, g2):
        assert ac.rel_err(a, b) <= 2e-5


def test_no_rows():
    from dfx import ops
    norm = nn.LayerNorm(64).cuda()
    x = torch.randn(0, 64, device="cuda", requires_grad=True)
    out = ops.add_layernorm_train(x, None, norm)
    gx, gw, gb = torch.autograd.grad(out.sum(), [x, norm.weight, norm.bias])
    assert out.shape == (0, 64) and gx.shape == (0, 64) and not gw.any() and not gb.any()
