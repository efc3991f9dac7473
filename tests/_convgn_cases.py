"""Cases, the fp64 reference and the fp32 yardsticks shared by tests/test_convgn_train_cpu.py and tests/test_convgn_train_gpu.py.

The operators (dfx.ops.conv1x1_backward, dfx.ops.group_norm_backward; include/dfx_gemm.h dfx_conv1x1_wgrad_f32,
include/dfx_fused.h dfx_group_norm_backward_f32) are the backward of the input projections, Conv2d(Ci, Co, 1) + GroupNorm.

``*_reference`` is torch autograd through F.conv2d / F.group_norm in fp64 on the CPU, from fp32-representable inputs;
``*_closed_form`` writes the same sums down (the CPU test holds the two together).  The bound is the project's: ``rel_err``
of the GPU result may be at most YARDSTICK_FACTOR times the ``rel_err`` of the yardstick, the same quantity in fp32 on the CPU:
  grad_w / grad_b  sequentially in the kernel's order - the pixels one at a time inside a range, the ranges of an image in
                   ascending order, then the images in ascending order (as tests/_linear_train_cases.yardstick does for rows)
  grad_x           one output channel at a time
  GroupNorm        fp32 CPU autograd of F.group_norm
"""
import functools

import torch
import torch.nn.functional as F

from tests._linear_train_cases import YARDSTICK_FACTOR, ranges, rel_err  # noqa: F401  (the project's factor and error measure)

CONV_OUTPUTS = ("grad_x", "grad_w", "grad_b")
GN_OUTPUTS = ("grad_x", "grad_gamma", "grad_beta")

# (N, Co, Ci, H, W, splits): the smallest problem; H*W = 260, no whole number of 16-deep steps, three images; the depth
# projection on the production map in one and in seven ranges; the RGB projection's width on a small map
CONV_SHAPES = [(1, 4, 4, 2, 2, None), (3, 256, 128, 13, 20, None), (2, 256, 128, 50, 84, 1), (2, 256, 128, 50, 84, 7),
               (2, 256, 2048, 10, 12, None)]
# (N, C, H, W, groups): 2 channels per group, H*W = 35 (no multiple of 4, one partial pixel tile); 3 channels per group and
# a partial 64-channel tile (a group straddles the tile edge); odd H*W with three images in the channel sums; the production map
GN_SHAPES = [(1, 64, 7, 5, 32), (2, 96, 4, 4, 32), (3, 256, 13, 21, 32), (2, 256, 50, 84, 32)]
GN_EPS = 1e-5


def _f32(t):
    return t.float().double()


# ---- 1x1 convolution -------------------------------------------------------------------------------------------------
def make_conv_case(N, Co, Ci, H, W, seed=0):
    """fp64 CPU tensors of fp32-representable values: x and grad_out standard normal, weight / sqrt(Ci), bias"""
    g = torch.Generator().manual_seed(1000 * seed + 3 * N + 7 * Co + 13 * Ci + 17 * H + W)
    case = {"x": torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64),
            "grad_out": torch.randn(N, Co, H, W, generator=g, dtype=torch.float64),
            "weight": torch.randn(Co, Ci, 1, 1, generator=g, dtype=torch.float64) / Ci ** 0.5,
            "bias": torch.randn(Co, generator=g, dtype=torch.float64)}
    case = {n: _f32(t) for n, t in case.items()}
    case["shape"] = (N, Co, Ci, H, W)
    return case


def conv_reference(case):
    leaves = [case[n].detach().clone().requires_grad_() for n in ("x", "weight", "bias")]
    y = F.conv2d(*leaves)
    return dict(zip(CONV_OUTPUTS, torch.autograd.grad(y, leaves, case["grad_out"])))


def conv_closed_form(case):
    go, x, w = case["grad_out"], case["x"], case["weight"]
    return {"grad_x": torch.einsum("nohw,oi->nihw", go, w[:, :, 0, 0]),
            "grad_w": torch.einsum("nohw,nihw->oi", go, x)[:, :, None, None], "grad_b": go.sum((0, 2, 3))}


def conv_yardstick(case, splits):
    """The three sums in fp32, sequentially in the kernel's order (see the module docstring)."""
    N, Co, Ci, H, W = case["shape"]
    HW = H * W
    go, x = case["grad_out"].float().reshape(N, Co, HW), case["x"].float().reshape(N, Ci, HW)
    w = case["weight"].float().reshape(Co, Ci)
    per, n_ranges = ranges(HW, splits)
    grad_w, grad_b = None, None
    for n in range(N):
        got, xt = go[n].t().contiguous(), x[n].t().contiguous()            # [HW, Co], [HW, Ci]
        for s in range(n_ranges):
            pw, pb = torch.zeros(Co, Ci), torch.zeros(Co)
            for p in range(s * per, min(HW, (s + 1) * per)):
                pw += torch.outer(got[p], xt[p])
                pb += got[p]
            grad_w, grad_b = (pw, pb) if grad_w is None else (grad_w + pw, grad_b + pb)
    grad_x = torch.zeros(N, Ci, HW)
    for o in range(Co):
        grad_x += w[o][None, :, None] * go[:, o][:, None, :]
    return {"grad_x": grad_x.reshape(N, Ci, H, W), "grad_w": grad_w.reshape(Co, Ci, 1, 1), "grad_b": grad_b}


def host_splits(Co, Ci, HW, N, splits):
    """the number of ranges per image a case runs with: its own, or (None) the host rule's"""
    if splits is not None:
        return splits
    from dfx import ops
    return ops._conv1x1_wgrad_splits(Co, Ci, HW, N)


@functools.lru_cache(maxsize=None)
def conv_prepared(N, Co, Ci, H, W, splits):
    """(case, fp64 reference, fp32 yardstick for ``splits`` ranges per image), computed once per case and never modified"""
    case = make_conv_case(N, Co, Ci, H, W)
    return case, conv_reference(case), conv_yardstick(case, splits)


# ---- GroupNorm -------------------------------------------------------------------------------------------------------
def make_gn_case(N, C, H, W, groups, seed=0):
    """x with a per-channel offset (means that are not zero), grad_out standard normal, gamma around 1, beta"""
    g = torch.Generator().manual_seed(1000 * seed + 3 * N + 7 * C + 13 * H + W)
    case = {"x": torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 1.5 + torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64),
            "grad_out": torch.randn(N, C, H, W, generator=g, dtype=torch.float64),
            "gamma": 1.0 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64),
            "beta": torch.randn(C, generator=g, dtype=torch.float64)}
    case = {n: _f32(t) for n, t in case.items()}
    case["shape"], case["groups"] = (N, C, H, W), groups
    return case


def _gn_autograd(case, dtype):
    leaves = [case[n].to(dtype).detach().clone().requires_grad_() for n in ("x", "gamma", "beta")]
    y = F.group_norm(leaves[0], case["groups"], leaves[1], leaves[2], GN_EPS)
    out = dict(zip(GN_OUTPUTS, torch.autograd.grad(y, leaves, case["grad_out"].to(dtype))))
    out["y"] = y.detach()
    return out


def gn_reference(case):
    return _gn_autograd(case, torch.float64)


def gn_yardstick(case):
    return _gn_autograd(case, torch.float32)


def gn_closed_form(case):
    """include/dfx_fused.h: dx = rstd (gamma dy - a_g / m - xh b_g / m), dgamma = sum dy xh, dbeta = sum dy"""
    (N, C, H, W), G = case["shape"], case["groups"]
    x, dy, gamma = case["x"], case["grad_out"], case["gamma"]
    xg = x.reshape(N, G, -1)
    mean, var = xg.mean(2, keepdim=True), xg.var(2, unbiased=False, keepdim=True)
    rstd = (var + GN_EPS).rsqrt()
    xh = ((xg - mean) * rstd).reshape(N, C, H, W)
    gdy = (gamma.view(1, C, 1, 1) * dy).reshape(N, G, -1)
    m = xg.shape[2]
    a, b = gdy.sum(2, keepdim=True), (gdy * xh.reshape(N, G, -1)).sum(2, keepdim=True)
    dx = (rstd * (gdy - a / m - xh.reshape(N, G, -1) * b / m)).reshape(N, C, H, W)
    return {"grad_x": dx, "grad_gamma": (dy * xh).sum((0, 2, 3)), "grad_beta": dy.sum((0, 2, 3)),
            "y": xh * gamma.view(1, C, 1, 1) + case["beta"].view(1, C, 1, 1)}


@functools.lru_cache(maxsize=None)
def gn_prepared(N, C, H, W, groups):
    """(case, fp64 reference, fp32 yardstick), computed once per case and never modified"""
    case = make_gn_case(N, C, H, W, groups)
    return case, gn_reference(case), gn_yardstick(case)
