"""GPU: BatchNorm2d with batch statistics (+ GELU), forward and backward - dfx_batch_norm_train_f32 and
dfx_batch_norm_backward_f32 (csrc/batchnorm_train.hip) - against the fp64 reference of tests/_dformer_train_cases.py within
the project's yardstick rule, at the smallest shapes that can still go wrong (tests/_dformer_train_cases.BN_CASES)."""
import pytest
import torch

from tests import _dformer_train_cases as dc

pytestmark = pytest.mark.gpu

FORWARD = ("y", "mean", "rstd", "running_mean", "running_var", "running_mean2", "running_var2")
GRADS = ("grad_x", "grad_gamma", "grad_beta")
ACTS = [None, "gelu"]


def _compare(ref, yard, got, names, what):
    """Per output: error relative to the reference's largest magnitude, at most YARDSTICK_FACTOR x the CPU fp32 figure"""
    worst = []
    for n in names:
        y, err = dc.rel_err(yard[n], ref[n]), dc.rel_err(got[n].cpu(), ref[n])
        print(f"  {what} {n}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}, "
              f"max |ref| {ref[n].abs().max().item():.3e}")
        assert got[n].shape == ref[n].shape, n
        if not err <= dc.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {dc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


def _forward(case, act):
    """the forward twice on the same running buffers -> {y, mean, rstd, running_* after one call, running_*2 after two}, stats"""
    from dfx import ops
    x, gamma, beta, rm, rv = (case[n].float().cuda() for n in ("x", "gamma", "beta", "running_mean", "running_var"))
    C = x.shape[1]
    versions = (rm._version, rv._version)
    y, stats = ops.batch_norm_train_forward(x, gamma, beta, rm, rv, dc.BN_MOMENTUM, dc.BN_EPS, act)
    assert rm._version > versions[0] and rv._version > versions[1], "the in-place update must move the version counters"
    out = {"y": y, "mean": stats[:C].clone(), "rstd": stats[C:].clone(), "running_mean": rm.clone(), "running_var": rv.clone()}
    y2, stats2 = ops.batch_norm_train_forward(x, gamma, beta, rm, rv, dc.BN_MOMENTUM, dc.BN_EPS, act)
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.equal(stats2, stats)
    out.update(running_mean2=rm, running_var2=rv)
    return out, stats


def _backward(case, act, stats, **need):
    from dfx import ops
    x, gamma, beta, go = (case[n].float().cuda() for n in ("x", "gamma", "beta", "grad_out"))
    got = ops.batch_norm_backward(go, x, stats, gamma, beta, dc.BN_EPS, act, **need)
    torch.cuda.synchronize()
    return dict(zip(GRADS, got))


@pytest.mark.parametrize("act", ACTS, ids=["plain", "gelu"])
@pytest.mark.parametrize("name", list(dc.BN_CASES))
def test_batch_norm_forward_and_backward_match_fp64_within_the_yardstick(name, act):
    case, ref, yard = dc.bn_prepared(name, act == "gelu")
    fwd, stats = _forward(case, act)
    full = _backward(case, act, stats)
    _compare(ref, yard, {**fwd, **full}, FORWARD + GRADS, f"batch_norm[{name}]")
    assert all(torch.isfinite(v).all() for v in full.values())
    # every NULL-output combination: what is computed keeps its bits
    for need in [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]:
        got = _backward(case, act, stats, need_x=need[0], need_gamma=need[1], need_beta=need[2])
        for n, asked in zip(GRADS, need):
            assert (got[n] is not None) == asked, (need, n)
            assert not asked or torch.equal(got[n], full[n]), (need, n)


@pytest.mark.parametrize("act", ACTS, ids=["plain", "gelu"])
@pytest.mark.parametrize("name", ["chunks_ragged", "stem_32"])
def test_batch_norm_twice_gives_the_same_bits(name, act):
    """No atomics, every sum in an order fixed by the shape; outputs and workspaces come from ``empty``."""
    case, _, _ = dc.bn_prepared(name, act == "gelu")
    fa, stats = _forward(case, act)
    a = _backward(case, act, stats)
    junk = torch.full((4 * case["x"].numel() + 4096,), float("nan"), device="cuda")      # what the next ``empty`` may hand out
    del junk
    fb, stats_b = _forward(case, act)
    b = _backward(case, act, stats_b)
    for n in FORWARD:
        assert torch.equal(fa[n], fb[n]) and torch.isfinite(fb[n]).all(), n
    for n in GRADS:
        assert torch.equal(a[n], b[n]) and torch.isfinite(b[n]).all(), n


def test_batch_norm_without_running_buffers_and_statistics_only():
    from dfx import _lib, ops
    case, _, _ = dc.bn_prepared("stem_32", False)
    x, gamma, beta = (case[n].float().cuda() for n in ("x", "gamma", "beta"))
    N, C, H, W = x.shape
    y, stats = ops.batch_norm_train_forward(x, gamma, beta, None, None, dc.BN_MOMENTUM, dc.BN_EPS)
    with_buffers, stats2 = _forward(case, None)
    assert torch.equal(y, with_buffers["y"]) and torch.equal(stats, stats2)
    only = torch.full((2 * C,), 7.0, device="cuda")
    ws = torch.empty(6 * C * N, device="cuda")
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    assert lib.dfx_batch_norm_train_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, None, only.data_ptr(),
                                        ws.data_ptr(), N, C, H * W, dc.BN_EPS, dc.BN_MOMENTUM, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(only, stats)


def test_batch_norm_entries_check_their_arguments():
    from dfx import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    N, C, HW = 2, 8, 6
    t = lambda n: torch.full((n,), 7.0, device="cuda")       # noqa: E731
    x, dy, gamma, beta, rm, rv, y, stats, ws = t(N * C * HW), t(N * C * HW), t(C), t(C), t(C), t(C), t(N * C * HW), t(2 * C), t(8 * C * N)
    dx, dg, db = t(N * C * HW), t(C), t(C)
    p = lambda v: v.data_ptr()                               # noqa: E731
    fwd, bwd = lib.dfx_batch_norm_train_f32, lib.dfx_batch_norm_backward_f32
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), N, 0, HW, 1e-5, 0.1, 0, st) != 0
    assert b"bad dimension" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), 1, C, 1, 1e-5, 0.1, 0, st) != 0
    assert b"more than one value" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), N, C, HW, 1e-5, 0.1, 1, st) != 0
    assert b"activation" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), None, N, C, HW, 1e-5, 0.1, 0, st) != 0
    assert b"null pointer" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), N, C, HW, 1e-5, 1.5, 0, st) != 0
    assert b"momentum" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), 70000, C, HW, 1e-5, 0.1, 0, st) != 0
    assert b"too large" in lib.dfx_last_error()
    assert fwd(p(x), p(gamma), p(beta), p(rm), p(rv), p(y), p(stats), p(ws), N, C, 1 << 31, 1e-5, 0.1, 0, st) != 0
    assert b"too large" in lib.dfx_last_error()
    assert bwd(p(dy), p(x), p(stats), p(gamma), p(beta), p(dx), p(dg), p(db), p(ws), N, C, -1, 1e-5, 0, st) != 0
    assert b"bad dimension" in lib.dfx_last_error()
    assert bwd(p(dy), p(x), p(stats), p(gamma), None, p(dx), p(dg), p(db), p(ws), N, C, HW, 1e-5, 2, st) != 0
    assert b"null pointer" in lib.dfx_last_error()
    assert bwd(p(dy), p(x), p(stats), p(gamma), p(beta), p(dx), p(dg), p(db), p(ws), N, C, HW, 1e-5, 3, st) != 0
    assert b"activation" in lib.dfx_last_error()
    assert bwd(p(dy), p(x), p(stats), p(gamma), p(beta), p(dx), p(dg), p(db), p(ws), N, 70000, HW, 1e-5, 0, st) != 0
    assert b"too large" in lib.dfx_last_error()
    assert bwd(None, None, None, None, None, None, None, None, None, N, C, HW, 1e-5, 0, st) == 0       # nothing asked for
    torch.cuda.synchronize()
    assert all((v == 7).all() for v in (rm, rv, y, stats, dx, dg, db)), "a refused or empty call wrote to an output"


@pytest.mark.parametrize("act", ACTS, ids=["plain", "gelu"])
def test_batch_norm_train_node_moves_the_module_as_nn_batchnorm_does(act):
    """dfx.ops.batch_norm_train on an nn.BatchNorm2d: running statistics and num_batches_tracked move as the module's own
    forward moves them, the node is made only for a gradient and computes only what is asked for."""
    import copy
    from torch import nn
    from dfx import ops
    case, ref, yard = dc.bn_prepared("stem_16", act == "gelu")
    N, C, H, W = case["shape"]
    bn = nn.BatchNorm2d(C, eps=dc.BN_EPS, momentum=dc.BN_MOMENTUM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(case["gamma"]), bn.bias.copy_(case["beta"])
        bn.running_mean.copy_(case["running_mean"]), bn.running_var.copy_(case["running_var"])
    lib = copy.deepcopy(bn)
    x = case["x"].float().cuda().requires_grad_()
    y = ops.batch_norm_train(x, bn, act)
    assert y.grad_fn is not None and int(bn.num_batches_tracked) == 1
    y.backward(case["grad_out"].float().cuda())
    got = {"y": y.detach(), "grad_x": x.grad, "grad_gamma": bn.weight.grad, "grad_beta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    _compare(ref, yard, got, tuple(got), "batch_norm_train")
    yl = lib(x.detach())
    assert torch.allclose(bn.running_mean, lib.running_mean, rtol=1e-6, atol=1e-7)      # (both within the yardstick of fp64 above)
    assert torch.allclose(bn.running_var, lib.running_var, rtol=1e-6, atol=1e-7)
    assert int(lib.num_batches_tracked) == 1 and yl.shape == y.shape
    # nothing to differentiate: no node; frozen affine parameters: only the input gradient is computed
    bn.requires_grad_(False)
    assert ops.batch_norm_train(x.detach(), bn, act).grad_fn is None and int(bn.num_batches_tracked) == 2
    asked = []
    real = ops.batch_norm_backward
    ops.batch_norm_backward = lambda *a, **k: (asked.append(k), real(*a, **k))[1]
    try:
        ops.batch_norm_train(x, bn, act).sum().backward()
    finally:
        ops.batch_norm_backward = real
    assert asked == [{"need_x": True, "need_gamma": False, "need_beta": False}]
    bn.eval()
    with pytest.raises(RuntimeError, match="training mode"):
        ops.batch_norm_train(x, bn, act)
