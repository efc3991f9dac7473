"""GPU: the input projections in grad mode - dfx_group_norm_backward_f32 (csrc/groupnorm_backward.hip), dfx_conv1x1_wgrad_f32 and
the input gradient on dfx_gemm_f32 against the fp64 reference of tests/_convgn_cases.py, and the grad-mode route of
``models.detector_common._ConvGN``."""
import copy

import pytest
import torch
from torch import nn

from tests import _convgn_cases as cc

pytestmark = pytest.mark.gpu


def _compare(ref, yard, got, names, what):
    """Per output: error relative to the reference's largest magnitude, at most YARDSTICK_FACTOR x the CPU fp32 figure"""
    worst = []
    for n in names:
        y, err = cc.rel_err(yard[n], ref[n]), cc.rel_err(got[n].cpu(), ref[n])
        print(f"  {what} {n}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}, "
              f"max |ref| {ref[n].abs().max().item():.3e}")
        assert got[n].shape == ref[n].shape, n
        if not err <= cc.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {cc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


# ---- GroupNorm backward ----------------------------------------------------------------------------------------
def _gn_backward(case, tokens, **need):
    """(forward result as NCHW, {output: gradient}) of the GPU forward + backward; ``tokens``: both in the token-major layout"""
    from dfx import ops
    x, gamma, beta = (case[n].float().cuda() for n in ("x", "gamma", "beta"))
    N, C, H, W = x.shape
    y, stats = ops._group_norm_forward(x, gamma, beta, case["groups"], cc.GN_EPS, tokens)
    go = case["grad_out"].float().cuda()
    if tokens:
        go = go.flatten(2).transpose(1, 2).contiguous()
        y = y.transpose(1, 2).unflatten(2, (H, W))
    got = ops.group_norm_backward(go, x, stats, gamma, case["groups"], tokens=tokens, **need)
    torch.cuda.synchronize()
    return y, dict(zip(cc.GN_OUTPUTS, got))


@pytest.mark.parametrize("tokens", [False, True], ids=["nchw", "tokens"])
@pytest.mark.parametrize("shape", cc.GN_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_group_norm_backward_matches_fp64_within_the_yardstick(shape, tokens):
    case, ref, yard = cc.gn_prepared(*shape)
    y, got = _gn_backward(case, tokens)
    _compare(ref, yard, {**got, "y": y}, cc.GN_OUTPUTS + ("y",), "group_norm")
    # NULL outputs: dx only, the parameter gradients only, each of them alone - what is computed keeps its bits
    only_x = _gn_backward(case, tokens, need_gamma=False, need_beta=False)[1]
    params = _gn_backward(case, tokens, need_x=False)[1]
    only_g = _gn_backward(case, tokens, need_x=False, need_beta=False)[1]
    only_b = _gn_backward(case, tokens, need_x=False, need_gamma=False)[1]
    assert only_x["grad_gamma"] is None and only_x["grad_beta"] is None and torch.equal(only_x["grad_x"], got["grad_x"])
    assert params["grad_x"] is None and only_g["grad_x"] is None and only_g["grad_beta"] is None
    assert only_b["grad_x"] is None and only_b["grad_gamma"] is None
    for n in ("grad_gamma", "grad_beta"):
        assert torch.equal(params[n], got[n]), n
    assert torch.equal(only_g["grad_gamma"], got["grad_gamma"]) and torch.equal(only_b["grad_beta"], got["grad_beta"])


@pytest.mark.parametrize("tokens", [False, True], ids=["nchw", "tokens"])
def test_group_norm_backward_twice_gives_the_same_bits_in_either_layout(tokens):
    case, _, _ = cc.gn_prepared(*cc.GN_SHAPES[2])
    a = _gn_backward(case, tokens)[1]
    junk = torch.full((3 * 256 * 13 * 21 + 3 * 256 * 32,), float("nan"), device="cuda")        # what the next ``empty`` may hand out
    del junk
    b = _gn_backward(case, tokens)[1]
    other = _gn_backward(case, not tokens)[1]
    for n in cc.GN_OUTPUTS:
        assert torch.equal(a[n], b[n]) and torch.isfinite(b[n]).all(), n
        assert torch.equal(a[n], other[n]), n         # the layout of dy changes how it is read, not what is added in which order


def test_group_norm_backward_entry_checks_its_arguments():
    from dfx import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    N, C, HW, G = 2, 8, 6, 4
    t = lambda n: torch.full((n,), 7.0, device="cuda")       # noqa: E731
    dy, x, stats, gamma, dx, dg, db, ws = t(N * C * HW), t(N * C * HW), t(N * G * 2), t(C), t(N * C * HW), t(C), t(C), t(N * C * 32)
    fn = lib.dfx_group_norm_backward_f32
    p = lambda v: v.data_ptr()                               # noqa: E731
    assert fn(p(dy), p(x), p(stats), p(gamma), p(dx), p(dg), p(db), p(ws), N, C, HW, 3, 0, st) != 0
    assert b"bad dimension" in lib.dfx_last_error()
    assert fn(p(dy), p(x), p(stats), p(gamma), p(dx), p(dg), p(db), None, N, C, HW, G, 0, st) != 0
    assert b"null pointer" in lib.dfx_last_error()
    assert fn(p(dy), p(x), p(stats), p(gamma), p(dx), p(dg), p(db), p(ws), 70000, C, HW, G, 0, st) != 0
    assert b"too large" in lib.dfx_last_error()
    assert fn(None, None, None, None, p(dx), p(dg), p(db), None, 0, C, HW, G, 0, st) == 0
    assert fn(None, None, None, None, p(dx), p(dg), p(db), None, N, C, 0, G, 1, st) == 0
    torch.cuda.synchronize()
    assert all((v == 7).all() for v in (dx, dg, db)), "a refused or empty call wrote to an output"


# ---- conv1x1_backward ------------------------------------------------------------------------------------------
def _conv_backward(case, splits=None, **need):
    from dfx import ops
    t = {n: case[n].float().cuda() for n in ("x", "weight", "grad_out")}
    got = ops.conv1x1_backward(t["grad_out"], t["x"], t["weight"], splits=splits, **need)
    torch.cuda.synchronize()
    return dict(zip(cc.CONV_OUTPUTS, got))


@pytest.mark.parametrize("shape", cc.CONV_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv1x1_backward_matches_fp64_within_the_sequential_yardstick(shape):
    N, Co, Ci, H, W, splits = shape
    case, ref, yard = cc.conv_prepared(N, Co, Ci, H, W, cc.host_splits(Co, Ci, H * W, N, splits))
    got = _conv_backward(case, splits=splits)
    _compare(ref, yard, got, cc.CONV_OUTPUTS, "conv1x1")


@pytest.mark.parametrize("shape", cc.CONV_SHAPES[:2], ids=lambda s: "x".join(str(v) for v in s))
def test_conv1x1_backward_computes_what_is_asked_for(shape):
    N, Co, Ci, H, W, splits = shape
    case, _, _ = cc.conv_prepared(N, Co, Ci, H, W, cc.host_splits(Co, Ci, H * W, N, splits))
    full = _conv_backward(case)
    for need in [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]:
        got = _conv_backward(case, need_x=need[0], need_w=need[1], need_b=need[2])
        for n, asked in zip(cc.CONV_OUTPUTS, need):
            assert (got[n] is not None) == asked, (need, n)
            assert not asked or torch.equal(got[n], full[n]), (need, n)


@pytest.mark.parametrize("splits", [1, 7])
def test_conv1x1_backward_twice_gives_the_same_bits(splits):
    """No atomics, the slabs are added in ascending (image, range) order; the outputs and the workspace come from ``empty``."""
    case, _, _ = cc.conv_prepared(2, 256, 128, 50, 84, splits)
    a = _conv_backward(case, splits=splits)
    junk = torch.full((2 * splits * 256 * 128 + 2 * 128 * 4200,), float("nan"), device="cuda")
    del junk
    b = _conv_backward(case, splits=splits)
    for n in cc.CONV_OUTPUTS:
        assert torch.equal(a[n], b[n]) and torch.isfinite(b[n]).all(), n


def test_conv1x1_wgrad_entry_checks_its_arguments():
    from dfx import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    N, Co, Ci, HW = 2, 8, 12, 20
    dz, x = torch.randn(N, Co, HW, device="cuda"), torch.randn(N, Ci, HW, device="cuda")
    dw, ws = torch.full((Co * Ci + 4,), 7.0, device="cuda"), torch.empty(N * 2 * Co * Ci, device="cuda")
    fn = lib.dfx_conv1x1_wgrad_f32
    assert fn(dz.data_ptr(), Co * HW, x.data_ptr(), Ci * HW, dw.data_ptr(), 6, Ci, HW, N, 1, ws.data_ptr(), st) != 0
    assert b"multiples of 4" in lib.dfx_last_error()
    assert fn(dz.data_ptr(), Co * HW, x.data_ptr(), Ci * HW, dw.data_ptr(), Co, Ci, 18, N, 1, ws.data_ptr(), st) != 0
    assert b"multiples of 4" in lib.dfx_last_error()
    assert fn(dz.data_ptr(), Co * HW, x.data_ptr(), Ci * HW, dw.data_ptr() + 4, Co, Ci, HW, N, 1, ws.data_ptr(), st) != 0
    assert b"aligned" in lib.dfx_last_error()
    assert fn(dz.data_ptr(), Co * HW, x.data_ptr(), Ci * HW, dw.data_ptr(), Co, Ci, HW, N, 1, None, st) != 0
    assert b"workspace" in lib.dfx_last_error()
    assert fn(dz.data_ptr(), Co * (1 << 28), x.data_ptr(), Ci * HW, dw.data_ptr(), Co, Ci, 1 << 28, 1, 1, ws.data_ptr(), st) != 0
    assert b"2 GiB" in lib.dfx_last_error()
    assert fn(dz.data_ptr(), Co * HW, x.data_ptr(), Ci * HW, dw.data_ptr(), 0, Ci, HW, N, 1, ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (dw == 7).all(), "a refused or empty call wrote to dW"
    assert fn(None, 0, None, 0, dw.data_ptr(), Co, Ci, HW, 0, 1, None, st) == 0
    torch.cuda.synchronize()
    assert (dw[:Co * Ci] == 0).all() and (dw[Co * Ci:] == 7).all()


# ---- autograd bookkeeping --------------------------------------------------------------------------------------
def test_conv1x1_train_makes_a_node_only_for_a_gradient_and_keeps_the_forward_bits(monkeypatch):
    from dfx import ops
    N, Co, Ci, H, W, _ = cc.CONV_SHAPES[1]
    case, _, _ = cc.conv_prepared(N, Co, Ci, H, W, 1)
    t = {n: case[n].float().cuda() for n in ("x", "weight", "bias", "grad_out")}
    raw = ops.conv1x1(t["x"], t["weight"], t["bias"])
    plain = ops.conv1x1_train(t["x"], t["weight"], t["bias"])
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, raw)
    direct = _conv_backward(case)
    asked, real = [], ops.conv1x1_backward

    def spy(*a, need_x=True, need_w=True, need_b=True, **k):
        asked.append((need_x, need_w, need_b))
        return real(*a, need_x=need_x, need_w=need_w, need_b=need_b, **k)

    monkeypatch.setattr(ops, "conv1x1_backward", spy)
    for requires in (("x", "weight", "bias"), ("x",), ("weight",), ("bias",)):
        leaves = {n: t[n].clone().requires_grad_(n in requires) for n in ("x", "weight", "bias")}
        with torch.no_grad():
            quiet = ops.conv1x1_train(*leaves.values())
        assert quiet.grad_fn is None and torch.equal(quiet, raw)
        y = ops.conv1x1_train(*leaves.values())
        assert y.grad_fn is not None and torch.equal(y.detach(), raw)
        y.backward(t["grad_out"])
        for n, out in zip(("x", "weight", "bias"), cc.CONV_OUTPUTS):
            assert (leaves[n].grad is not None) == (n in requires), (requires, n)
            if n in requires:
                assert leaves[n].grad.shape == leaves[n].shape and torch.equal(leaves[n].grad, direct[out]), (requires, n)
    assert asked == [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]


# ---- the module ------------------------------------------------------------------------------------------------
def _projection(cin=128, cout=256, seed=5, **kw):
    from models.detector_common import _conv_gn
    torch.manual_seed(seed)
    m = _conv_gn(cin, cout, **kw)
    with torch.no_grad():                                     # (the detector zeroes the bias and leaves the norm at 1 / 0)
        m[0].bias.normal_()
        m[1].weight.normal_(1.0, 0.3)
        m[1].bias.normal_()
    return m


def _inputs(N, cin, cout, H, W, Ho=None, Wo=None, seed=6):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(N, cin, H, W, generator=g), "weight": torch.randn(N, cout, Ho or H, Wo or W, generator=g)}


def _call_module(m, inputs, device, dtype):
    """(output, {name: gradient}, grad_fn name) of loss = sum(out * weight)"""
    m = copy.deepcopy(m).to(device=device, dtype=dtype)
    x = inputs["x"].to(device=device, dtype=dtype).requires_grad_()
    out = m(x)
    leaves = {"x": x, **dict(m.named_parameters())}
    grads = torch.autograd.grad((out * inputs["weight"].to(device=device, dtype=dtype)).sum(), list(leaves.values()))
    return out.detach().cpu(), {n: g.detach().cpu() for n, g in zip(leaves, grads)}, type(out.grad_fn).__name__


def _module_yardstick(m, inputs):
    """The module in fp32 on the CPU with the convolution's sums restated sequentially (tests/_convgn_cases.conv_yardstick:
    the weight gradient in the host rule's ranges) and the GroupNorm through fp32 CPU autograd of F.group_norm."""
    import torch.nn.functional as F
    conv, norm = m[0], m[1]
    x, g = inputs["x"], inputs["weight"]
    N, Ci, H, W = x.shape
    Co = conv.out_channels
    w = conv.weight.detach().reshape(Co, Ci)
    z = torch.zeros(N, Co, H * W)
    for i in range(Ci):
        z += w[:, i][None, :, None] * x[:, i].reshape(N, 1, H * W)
    z = (z + conv.bias.detach()[None, :, None]).reshape(N, Co, H, W).requires_grad_()
    gamma, beta = norm.weight.detach().clone().requires_grad_(), norm.bias.detach().clone().requires_grad_()
    y = F.group_norm(z, norm.num_groups, gamma, beta, norm.eps)
    dz, dgamma, dbeta = torch.autograd.grad(y, [z, gamma, beta], g)
    case = {"x": x.double(), "grad_out": dz.double(), "weight": conv.weight.detach().double(), "shape": (N, Co, Ci, H, W)}
    back = cc.conv_yardstick(case, cc.host_splits(Co, Ci, H * W, N, None))
    return y.detach(), {"x": back["grad_x"], "0.weight": back["grad_w"], "0.bias": back["grad_b"], "1.weight": dgamma, "1.bias": dbeta}


class _ModuleSpy:
    """counts nn.Conv2d.forward and nn.GroupNorm.forward"""

    def __init__(self, monkeypatch):
        self.conv = self.norm = 0
        conv, norm = nn.Conv2d.forward, nn.GroupNorm.forward

        def conv_spy(mod, x):
            self.conv += 1
            return conv(mod, x)

        def norm_spy(mod, x):
            self.norm += 1
            return norm(mod, x)

        monkeypatch.setattr(nn.Conv2d, "forward", conv_spy)
        monkeypatch.setattr(nn.GroupNorm, "forward", norm_spy)


def test_module_trains_on_the_projects_kernels(monkeypatch):
    """The depth projection Conv2d(128, 256, 1) + GroupNorm(32, 256) on a 2 x 13 x 20 map: the output and all five gradients
    against the fp64 CPU module within the bound, the forward bit-equal to the no_grad route, no nn.Conv2d / nn.GroupNorm
    forward on the route - and both with CONVGN_TRAIN off."""
    from models import fused
    m, inputs = _projection(), _inputs(2, 128, 256, 13, 20)
    ref = _call_module(m, inputs, "cpu", torch.float64)
    yard = _module_yardstick(m, inputs)
    spy = _ModuleSpy(monkeypatch)
    assert fused.CONVGN_TRAIN
    monkeypatch.setattr(fused, "CONVGN_TRAIN_MIN_PIXELS", 0)       # (the size rule is a speed matter: its own test is below)
    got = _call_module(m, inputs, "cuda", torch.float32)
    assert (spy.conv, spy.norm) == (0, 0), "grad mode still ran the library route"
    assert set(got[1]) == set(ref[1]) == set(yard[1]) and len(ref[1]) == 5
    named = [("out", ref[0], yard[0], got[0])] + [(n, ref[1][n], yard[1][n], got[1][n]) for n in ref[1]]
    _compare({n: r for n, r, _, _ in named}, {n: y for n, _, y, _ in named}, {n: g for n, _, _, g in named}, [n for n, *_ in named], "module")
    with torch.no_grad():
        quiet = copy.deepcopy(m).cuda()(inputs["x"].cuda())
    assert quiet.grad_fn is None and torch.equal(quiet.cpu(), got[0])
    assert quiet.shape == (2, 256, 13, 20) and quiet.flatten(2).transpose(1, 2).is_contiguous()      # token-major memory
    monkeypatch.setattr(fused, "CONVGN_TRAIN", False)
    library = _call_module(m, inputs, "cuda", torch.float32)
    assert (spy.conv, spy.norm) == (1, 1)
    assert torch.allclose(got[0], library[0], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("geometry", ["hw_not_a_multiple_of_4", "3x3_stride_2"])
def test_other_convolutions_keep_nn_conv2d_and_take_the_norms_node(monkeypatch, geometry):
    if geometry == "3x3_stride_2":
        m, inputs = _projection(128, 256, kernel_size=3, stride=2, padding=1), _inputs(2, 128, 256, 13, 20, 7, 10)
    else:
        m, inputs = _projection(), _inputs(2, 128, 256, 13, 21)
    from models import fused
    ref = _call_module(m, inputs, "cpu", torch.float64)
    # the yardstick is nn.Sequential on the same GPU (the switch off): the convolution is the library's on both sides, what
    # differs is the GroupNorm and its backward
    monkeypatch.setattr(fused, "CONVGN_TRAIN", False)
    yard = _call_module(m, inputs, "cuda", torch.float32)
    monkeypatch.setattr(fused, "CONVGN_TRAIN", True)
    monkeypatch.setattr(fused, "CONVGN_TRAIN_MIN_PIXELS", 0)
    spy = _ModuleSpy(monkeypatch)
    got = _call_module(m, inputs, "cuda", torch.float32)
    assert (spy.conv, spy.norm) == (1, 0)
    named = [("out", ref[0], yard[0], got[0])] + [(n, ref[1][n], yard[1][n], got[1][n]) for n in ref[1]]
    _compare({n: r for n, r, _, _ in named}, {n: y for n, _, y, _ in named}, {n: g for n, _, _, g in named}, [n for n, *_ in named], "module")


def test_maps_below_the_measured_size_keep_nn_sequential(monkeypatch):
    """models.fused.CONVGN_TRAIN_MIN_PIXELS: the smallest map measured faster on the kernels (12 frames of 50 x 84); one pixel
    row fewer runs the library's modules, the threshold itself the kernels - with the same results up to fp32 rounding."""
    from models import fused
    assert fused.CONVGN_TRAIN_MIN_PIXELS == 12 * 50 * 84
    m = _projection(128, 256).cuda()
    spy = _ModuleSpy(monkeypatch)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(12, 128, 50, 84, generator=g).cuda().requires_grad_()
    below = m(x[:, :, :49])
    assert (spy.conv, spy.norm) == (1, 1)
    at = m(x)
    assert (spy.conv, spy.norm) == (1, 1) and at.requires_grad
    monkeypatch.setattr(fused, "CONVGN_TRAIN", False)
    library = m(x)
    assert (spy.conv, spy.norm) == (2, 2)
    assert torch.allclose(at, library, rtol=1e-4, atol=2e-5) and torch.allclose(below, m(x[:, :, :49]), rtol=1e-4, atol=2e-5)
