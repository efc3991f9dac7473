"""Cases, the fp64 reference and the fp32 yardstick shared by tests/test_dformer_train_cpu.py, tests/test_dformer_train_gpu.py,
tests/test_dformer_train_routes_gpu.py and tools/gen_golden_dformer_train.py.

The operators (dfx.ops.batch_norm_train_forward / batch_norm_backward; include/dfx_fused.h dfx_batch_norm_train_f32,
dfx_batch_norm_backward_f32) are nn.BatchNorm2d with batch statistics, optionally followed by the exact GELU, of the DFormer
depth stem when it trains.

``bn_reference`` is torch autograd through F.batch_norm(training=True) (+ F.gelu) in fp64 on the CPU, from fp32-representable
inputs; ``bn_closed_form`` writes the same sums down (the CPU test holds the two together).  The bound is the project's:
``rel_err`` of the GPU result may be at most YARDSTICK_FACTOR times the ``rel_err`` of the yardstick, the same computation
through fp32 CPU autograd.
"""
import functools

import torch
import torch.nn.functional as F

from tests._linear_train_cases import YARDSTICK_FACTOR, rel_err  # noqa: F401  (the project's factor and error measure)

BN_OUTPUTS = ("y", "mean", "rstd", "grad_x", "grad_gamma", "grad_beta")
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
CHUNK = 8192          # DFX_BN_CHUNK_PIXELS of include/dfx_fused.h
BWD_MAX_GROUPS = 128  # DFX_BN_BWD_MAX_GROUPS

# name -> (N, C, H, W, kind).  two values per channel; H*W = 680, no multiple of 64 ... and 170, no multiple of 4 (the scalar
# path); 45 pixels, odd; H*W = 9000 = one whole chunk and a ragged one of 808 pixels, three images (six chunks per channel);
# the same with H*W = 9001 on the scalar path; 131 images = 131 chunks per channel, more than DFX_BN_BWD_MAX_GROUPS = 128, so
# the backward's sums run over groups of two chunks with a single one left over; |mean| >> std, where E[x^2] - E[x]^2 in
# fp32 has no correct digit; a zero and a negative gamma
BN_CASES = {
    "two_values": (2, 1, 1, 1, "plain"),
    "stem_16": (3, 16, 20, 34, "plain"),
    "stem_32": (2, 32, 10, 17, "plain"),
    "stem_64": (1, 64, 5, 9, "plain"),
    "chunks_ragged": (3, 2, 90, 100, "plain"),
    "chunks_ragged_scalar": (2, 2, 1, 9001, "plain"),
    "many_images": (131, 2, 3, 5, "plain"),
    "large_mean": (2, 4, 12, 20, "large_mean"),
    "gamma_zero_negative": (2, 4, 6, 10, "gamma"),
}


def _f32(t):
    return t.float().double()


def make_bn_case(name, seed=0):
    """fp64 CPU tensors of fp32-representable values: x with a per-channel offset and scale, grad_out standard normal,
    gamma around 1, beta, running statistics that are not the initial ones"""
    N, C, H, W, kind = BN_CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + 3 * N + 7 * C + 13 * H + W)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rnd(N, C, H, W) * (0.5 + rnd(1, C, 1, 1).abs()) + rnd(1, C, 1, 1)
    if kind == "large_mean":
        x = 1000.0 + 0.01 * rnd(N, C, H, W)
    gamma = 1.0 + 0.5 * rnd(C)
    if kind == "gamma":
        gamma[0], gamma[1] = 0.0, -1.25
    case = {"x": x, "grad_out": rnd(N, C, H, W), "gamma": gamma, "beta": 0.5 * rnd(C),
            "running_mean": 0.1 * rnd(C), "running_var": 0.75 + 0.5 * rnd(C).abs()}
    case = {n: _f32(t) for n, t in case.items()}
    case["shape"], case["name"] = (N, C, H, W), name
    return case


def _bn_autograd(case, gelu, dtype):
    leaves = [case[n].to(dtype).detach().clone().requires_grad_() for n in ("x", "gamma", "beta")]
    rm, rv = case["running_mean"].to(dtype).clone(), case["running_var"].to(dtype).clone()
    y = F.batch_norm(leaves[0], rm, rv, leaves[1], leaves[2], True, BN_MOMENTUM, BN_EPS)
    if gelu:
        y = F.gelu(y)
    out = dict(zip(("grad_x", "grad_gamma", "grad_beta"), torch.autograd.grad(y, leaves, case["grad_out"].to(dtype))))
    x = leaves[0].detach()
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)       # (in ``dtype``: the yardstick's are fp32 sums)
    out.update(y=y.detach(), mean=mean, rstd=(var + BN_EPS).rsqrt(), running_mean=rm, running_var=rv)
    rm2, rv2 = rm.clone(), rv.clone()                                     # the running statistics after a second call
    F.batch_norm(x, rm2, rv2, leaves[1].detach(), leaves[2].detach(), True, BN_MOMENTUM, BN_EPS)
    out.update(running_mean2=rm2, running_var2=rv2)
    return out


def bn_reference(case, gelu):
    return _bn_autograd(case, gelu, torch.float64)


def bn_yardstick(case, gelu):
    return _bn_autograd(case, gelu, torch.float32)


def bn_closed_form(case, gelu):
    """include/dfx_fused.h: z = gamma xh + beta, g = dy (* gelu'(z)), dx = gamma rstd (g - mean g - xh mean(g xh)),
    dgamma = sum g xh, dbeta = sum g; running = (1 - m) running + m stat with the unbiased variance"""
    N, C, H, W = case["shape"]
    x, dy = case["x"], case["grad_out"]
    v = lambda t: t.view(1, C, 1, 1)          # noqa: E731
    m = N * H * W
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    rstd = (var + BN_EPS).rsqrt()
    xh = (x - v(mean)) * v(rstd)
    z = v(case["gamma"]) * xh + v(case["beta"])
    if gelu:
        g = dy * (0.5 * (1 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5)
        y = 0.5 * z * (1 + torch.erf(z / 2 ** 0.5))
    else:
        g, y = dy, z
    s1, s2 = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    dx = v(case["gamma"] * rstd) * (g - v(s1) / m - xh * v(s2) / m)
    rm = (1 - BN_MOMENTUM) * case["running_mean"] + BN_MOMENTUM * mean
    rv = (1 - BN_MOMENTUM) * case["running_var"] + BN_MOMENTUM * var * m / (m - 1)
    return {"y": y, "mean": mean, "rstd": rstd, "grad_x": dx, "grad_gamma": s2, "grad_beta": s1,
            "running_mean": rm, "running_var": rv,
            "running_mean2": (1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean,
            "running_var2": (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var * m / (m - 1)}


def naive_variance_f32(case):
    """E[x^2] - E[x]^2 with fp32 sums: what the kernel must NOT do (the "large_mean" case shows why)"""
    x = case["x"].float()
    return (x * x).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2


@functools.lru_cache(maxsize=None)
def bn_prepared(name, gelu):
    """(case, fp64 reference, fp32 yardstick), computed once per case and never modified"""
    case = make_bn_case(name)
    return case, bn_reference(case, gelu), bn_yardstick(case, gelu)


# ---- the whole stem ---------------------------------------------------------------------------------------------------
STEM_INPUT = (2, 1, 64, 96)
STEM_SEED = 5
# the biases whose output goes straight into a BatchNorm in training mode - stage 0's two convolutions, stage 1's convolution
# (stage 2's leading BatchNorm normalises it) and the BatchNorm that ends stage 0 (stage 1 begins with another): the batch mean
# removes them, their gradient is mathematically zero.  (The weight of that BatchNorm, 0.4, is left a gradient of 4e-4 by
# eps alone; fp32 autograd has two digits of it, and the yardstick rule carries that.)
STEM_ZERO_GRADS = tuple(f"grad.depth_backbone.downsample_layers_e.{s}.bias" for s in ("0.0", "0.3", "0.4", "1.1"))


def stem_inputs():
    """the depth input [2,1,64,96] and the output gradient g [2,128,4,6] of the loss (out * g).sum(), fp32-representable fp64"""
    gen = torch.Generator().manual_seed(STEM_SEED)
    depth = _f32(torch.randn(*STEM_INPUT, generator=gen, dtype=torch.float64) * 0.5 + 0.3)
    g = _f32(torch.randn(STEM_INPUT[0], 128, STEM_INPUT[2] // 16, STEM_INPUT[3] // 16, generator=gen, dtype=torch.float64))
    return depth, g


def run_stem(backbone_cls, nested_tensor_cls, fill, dtype, device="cpu"):
    """One training pass of ``backbone_cls(train_backbone=True, freeze_batchnorm=False)`` in train mode with weights filled by
    name: -> (module, {"out", "grad.<parameter>", "buffer.<running statistic>"}) as CPU tensors of ``dtype``"""
    torch.manual_seed(0)
    net = backbone_cls(train_backbone=True, freeze_batchnorm=False)
    fill(net, seed=STEM_SEED)
    net = net.to(device=device, dtype=dtype).train()
    depth, g = stem_inputs()
    depth, g = depth.to(device=device, dtype=dtype), g.to(device=device, dtype=dtype)
    mask = torch.zeros(depth.shape[0], depth.shape[2], depth.shape[3], dtype=torch.bool, device=device)
    out = net(nested_tensor_cls(depth, mask))["0"].tensors
    (out * g).sum().backward()
    res = {"out": out.detach()}
    for n, p in net.named_parameters():
        if p.grad is not None:
            res["grad." + n] = p.grad
    for n, b in net.named_buffers():
        res["buffer." + n] = b
    return net, {k: v.detach().cpu().clone() for k, v in res.items()}
