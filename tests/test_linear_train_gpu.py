"""GPU: Linear in grad mode - dfx_gemm_wgrad_f32 (csrc/gemm_wgrad.hip) and the input gradient on dfx_gemm_f32 against the fp64
reference of tests/_linear_train_cases.py, the autograd surface of ``dfx.ops.linear_train`` and the grad-mode route of
``models.fused.Linear``."""
import copy

import pytest
import torch
from torch import nn

from tests import _linear_train_cases as lc

pytestmark = pytest.mark.gpu


def _gpu(case, requires=()):
    t = {n: case[n].float().cuda() for n in ("x", "weight", "bias", "grad_out")}
    for n in requires:
        t[n].requires_grad_()
    return t


def _backward(case, bias=True, splits=None, **need):
    from dfx import ops
    t = _gpu(case)
    got = ops.linear_backward(t["grad_out"], t["x"], t["weight"], need_b=bias, splits=splits, **need)
    torch.cuda.synchronize()
    return dict(zip(lc.OUTPUTS, got))


def _compare(ref, yard, got, names):
    """Per output: error relative to the reference's largest magnitude, at most 4x the sequential CPU fp32 figure"""
    worst = []
    for n in names:
        y, err = lc.rel_err(yard[n], ref[n]), lc.rel_err(got[n].cpu(), ref[n])
        print(f"  {n}: cpu fp32 sequential {y:.3e}, gpu {err:.3e}, max |ref| {ref[n].abs().max().item():.3e}")
        if not err <= lc.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {lc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


# ---- operator against fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", lc.OPERATOR_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_operator_matches_fp64_within_the_sequential_yardstick(shape, bias):
    M, N, K, splits = shape
    case, ref, yard = lc.prepared(M, N, K, lc.host_splits(M, N, K, splits))
    got = _backward(case, bias=bias, splits=splits)
    assert got["grad_x"].shape == (M, K) and got["grad_w"].shape == (N, K)
    assert (got["grad_b"] is None) == (not bias)
    _compare(ref, yard, got, lc.OUTPUTS if bias else lc.OUTPUTS[:2])


def test_padded_rows_and_columns_contribute_nothing():
    """33 rows (15 padded rows in the third 16-row step), 64 x 36 outputs on the 64 x 128 tile: with grad_out of order 1000
    a tail row or column that is not exactly zero adds terms of the size of the result, far beyond the yardstick."""
    case, ref, yard = lc.prepared(33, 64, 36, 1, 1024.0)
    _compare(ref, yard, _backward(case), lc.OUTPUTS)


@pytest.mark.parametrize("splits", [1, 7])
def test_two_calls_give_the_same_bits(splits):
    """No atomics, the ranges are added in ascending order; the outputs and the workspace are allocated with ``empty``."""
    case, _, _ = lc.prepared(1000, 256, 256, splits)
    a = _backward(case, splits=splits)
    junk = torch.full((splits * (256 * 256 + 256) + 1000 * 256,), float("nan"), device="cuda")     # what the next ``empty`` may hand out
    del junk
    b = _backward(case, splits=splits)
    for n in lc.OUTPUTS:
        assert torch.equal(a[n], b[n]), n
        assert torch.isfinite(b[n]).all(), n


def test_grad_x_in_row_ranges_has_the_bits_of_one_call(monkeypatch):
    from dfx import ops
    case, _, _ = lc.prepared(1000, 256, 256, 1)
    whole = _backward(case, need_w=False, bias=False)
    assert whole["grad_w"] is None and whole["grad_b"] is None
    calls, real = [0], ops._call

    def counting(what, name, *a):
        calls[0] += name == "dfx_gemm_f32"
        return real(what, name, *a)

    monkeypatch.setattr(ops, "_call", counting)
    monkeypatch.setattr(ops, "_GEMM_MAX_BYTES", 256 * 256 * 4)          # 255 rows fit: ranges of 128 rows
    parts = _backward(case, need_w=False, bias=False)
    assert calls[0] == 8
    assert torch.equal(parts["grad_x"], whole["grad_x"])


# ---- autograd bookkeeping --------------------------------------------------------------------------------------
def _train(case, requires, bias=True):
    from dfx import ops
    t = _gpu(case, requires)
    y = ops.linear_train(t["x"], t["weight"], t["bias"] if bias else None)
    assert y.grad_fn is not None
    y.backward(t["grad_out"])
    torch.cuda.synchronize()
    return {"y": y.detach(), "grad_x": t["x"].grad, "grad_w": t["weight"].grad, "grad_b": t["bias"].grad}


def test_unrequested_gradients_are_skipped_and_the_others_unchanged(monkeypatch):
    from dfx import ops
    case, _, _ = lc.prepared(300, 132, 200, 1)
    asked, real = [], ops.linear_backward

    def spy(*a, need_x=True, need_w=True, need_b=True, **k):
        asked.append((need_x, need_w, need_b))
        res = real(*a, need_x=need_x, need_w=need_w, need_b=need_b, **k)
        assert [r is not None for r in res] == [need_x, need_w, need_b]
        return res

    monkeypatch.setattr(ops, "linear_backward", spy)
    full = _train(case, ("x", "weight", "bias"))
    only_x, only_w, only_b = _train(case, ("x",)), _train(case, ("weight",)), _train(case, ("bias",))
    no_bias = _train(case, ("x", "weight"), bias=False)
    assert asked == [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, True, False)]
    direct = _backward(case)
    for n in lc.OUTPUTS:
        assert torch.equal(full[n], direct[n]), n
    assert only_x["grad_w"] is None and only_x["grad_b"] is None and torch.equal(only_x["grad_x"], full["grad_x"])
    assert only_w["grad_x"] is None and only_w["grad_b"] is None and torch.equal(only_w["grad_w"], full["grad_w"])
    assert only_b["grad_x"] is None and only_b["grad_w"] is None
    assert lc.rel_err(only_b["grad_b"], full["grad_b"]) < 1e-5          # (the library's sum: another order)
    assert no_bias["grad_b"] is None and torch.equal(no_bias["grad_w"], full["grad_w"])


def test_no_node_without_a_gradient_to_carry_and_the_forward_keeps_its_bits():
    from dfx import ops
    case, _, _ = lc.prepared(300, 132, 200, 1)
    t = _gpu(case)
    raw = ops.linear(t["x"], t["weight"], t["bias"])
    plain = ops.linear_train(t["x"], t["weight"], t["bias"])
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, raw)
    tg = _gpu(case, ("x", "weight", "bias"))
    with torch.no_grad():
        quiet = ops.linear_train(tg["x"], tg["weight"], tg["bias"])
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, raw)
    tracked = ops.linear_train(tg["x"], tg["weight"], tg["bias"])
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), raw)
    shaped = ops.linear_train(tg["x"].view(3, 100, 200), tg["weight"], None)
    assert shaped.shape == (3, 100, 132) and torch.equal(shaped.detach().view(300, 132), ops.linear(t["x"], t["weight"]))


# ---- the entry checks its arguments ----------------------------------------------------------------------------
def test_entry_checks_its_arguments():
    from dfx import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    M, N, K = 33, 8, 12
    dy, x = torch.randn(M, N, device="cuda"), torch.randn(M, K, device="cuda")
    dw, db = torch.full((N * K + 4,), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
    fn = lib.dfx_gemm_wgrad_f32
    assert fn(dy.data_ptr(), 6, x.data_ptr(), K, dw.data_ptr(), K, None, M, 6, K, 1, None, st) != 0
    assert b"multiples of 4" in lib.dfx_last_error()
    assert fn(dy.data_ptr(), N, x.data_ptr(), K, dw.data_ptr() + 4, K, None, M, N, K, 1, None, st) != 0
    assert b"aligned" in lib.dfx_last_error()
    assert fn(dy.data_ptr(), N, x.data_ptr(), K, dw.data_ptr(), K, None, M, N, K, 2, None, st) != 0
    assert b"workspace" in lib.dfx_last_error()
    assert fn(dy.data_ptr(), N, x.data_ptr(), K, dw.data_ptr(), K, None, M, 0, K, 2, None, st) == 0
    torch.cuda.synchronize()
    assert (dw == 7).all(), "a refused or empty call wrote to dW"
    assert fn(None, N, None, K, dw.data_ptr(), K, db.data_ptr(), 0, N, K, 1, None, st) == 0
    torch.cuda.synchronize()
    assert (dw[:N * K] == 0).all() and (dw[N * K:] == 7).all() and (db == 0).all()


# ---- the module ------------------------------------------------------------------------------------------------
def _ffn(seed=5):
    from models.fused import Linear
    torch.manual_seed(seed)
    return nn.Sequential(Linear(256, 1024), nn.ReLU(), Linear(1024, 256))


def _ffn_inputs(seed=6):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(2, 45, 256, generator=g), "weight": torch.randn(2, 45, 256, generator=g)}


def _call_module(m, inputs, device, dtype):
    """(output, {name: gradient}) of loss = sum(out * weight)"""
    m = copy.deepcopy(m).to(device=device, dtype=dtype)
    x = inputs["x"].to(device=device, dtype=dtype).requires_grad_()
    out = m(x)
    leaves = {"x": x, **dict(m.named_parameters())}
    grads = torch.autograd.grad((out * inputs["weight"].to(device=device, dtype=dtype)).sum(), list(leaves.values()))
    return out.detach().cpu().double(), {n: g.detach().cpu().double() for n, g in zip(leaves, grads)}


def _seq(a, b):
    """a [I,J] @ b [J,L] in fp32, one j at a time"""
    out = torch.zeros(a.shape[0], b.shape[1])
    for j in range(a.shape[1]):
        out += torch.outer(a[:, j], b[j])
    return out


def _sequential_module(m, inputs):
    """The same output and gradients in fp32 on the CPU with every product summed sequentially (the yardstick)"""
    x, g = inputs["x"].reshape(-1, 256), inputs["weight"].reshape(-1, 256)
    w1, b1, w2, b2 = (p.detach() for p in (m[0].weight, m[0].bias, m[2].weight, m[2].bias))
    y1 = _seq(x, w1.t()) + b1
    h = y1.clamp_min(0)
    y2 = _seq(h, w2.t()) + b2
    dh = _seq(g, w2) * (y1 > 0)
    ones = torch.ones(1, x.shape[0])
    grads = {"x": _seq(dh, w1).view_as(inputs["x"]), "0.weight": _seq(dh.t(), x), "0.bias": _seq(ones, dh)[0],
             "2.weight": _seq(g.t(), h), "2.bias": _seq(ones, g)[0]}
    return y2.view_as(inputs["x"]), grads


class _LinearSpy:
    def __init__(self, monkeypatch):
        self.calls = 0
        real = torch.nn.functional.linear

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)

        monkeypatch.setattr(torch.nn.functional, "linear", spy)


def test_module_trains_on_the_mfma_route(monkeypatch):
    """Linear(256, 1024), ReLU, Linear(1024, 256) on [2, 45, 256]: the output and every gradient against the fp64 CPU module,
    each within 4x the error of the sequential fp32 restatement; torch.nn.functional.linear is not called on the route and is
    with LINEAR_TRAIN off."""
    from models import fused
    m, inputs = _ffn(), _ffn_inputs()
    ref = _call_module(m, inputs, "cpu", torch.float64)
    # (a hidden unit whose pre-activation rounds across zero would flip its ReLU between two fp32 evaluations: none comes near)
    pre = torch.nn.functional.linear(inputs["x"].double(), m[0].weight.double(), m[0].bias.double())
    assert pre.abs().min().item() > 2e-6
    yard = _sequential_module(m, inputs)
    spy = _LinearSpy(monkeypatch)
    assert fused.LINEAR_TRAIN
    got = _call_module(m, inputs, "cuda", torch.float32)
    assert spy.calls == 0, "grad mode still ran the library route"
    assert set(got[1]) == set(ref[1]) == set(yard[1]) and len(ref[1]) == 5
    bad = []
    for n, r, y, g in [("out", ref[0], yard[0], got[0])] + [(n, ref[1][n], yard[1][n], got[1][n]) for n in ref[1]]:
        ey, eg = lc.rel_err(y, r), lc.rel_err(g, r)
        print(f"  {n}: cpu fp32 sequential {ey:.3e}, gpu {eg:.3e}")
        if not eg <= lc.YARDSTICK_FACTOR * ey:
            bad.append(f"{n}: gpu {eg:.3e} against {lc.YARDSTICK_FACTOR} x {ey:.3e}")
    assert not bad, "; ".join(bad)
    monkeypatch.setattr(fused, "LINEAR_TRAIN", False)
    library = _call_module(m, inputs, "cuda", torch.float32)
    assert spy.calls == 2
    assert torch.allclose(got[0], library[0], rtol=1e-4, atol=2e-5)


def test_other_widths_and_frozen_layers_stay_on_nn_linear(monkeypatch):
    from models.fused import Linear
    spy = _LinearSpy(monkeypatch)
    x = torch.randn(2, 45, 256, device="cuda", requires_grad=True)
    narrow = Linear(256, 31).cuda()
    y = narrow(x)
    assert spy.calls == 1 and y.shape == (2, 45, 31) and "LinearFunction" not in type(y.grad_fn).__name__
    wide = Linear(256, 32).cuda()
    assert "LinearFunction" in type(wide(x).grad_fn).__name__ and spy.calls == 1
    for p in wide.parameters():
        p.requires_grad_(False)
    frozen = wide(x.detach())                 # grad mode with nothing to differentiate
    assert spy.calls == 2 and frozen.grad_fn is None
    from models import fused
    assert fused.LINEAR_TRAIN_MAX_OUT_FEATURES == 1024
    widest, beyond = Linear(256, 1024).cuda(), Linear(256, 1028).cuda()
    assert "LinearFunction" in type(widest(x).grad_fn).__name__ and spy.calls == 2
    assert "LinearFunction" not in type(beyond(x).grad_fn).__name__ and spy.calls == 3
