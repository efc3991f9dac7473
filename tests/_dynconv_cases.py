"""Shared builders of the DynamicConv backward tests: seeded cases whose gradients do not depend on a ReLU unit that fp32
evaluations may disagree about, the module formulation (bmm + layer_norm + relu) under autograd, and a restatement of
the backward in plain tensor arithmetic (the yardstick the GPU tests compare with).

ReLU kinks.  The gradient is discontinuous where a pre-activation changes sign, and two fp32 evaluations disagree about
the sign of a pre-activation within their rounding error of zero; one flipped unit changes dZ of its whole row and
dK1, dK2 of its whole RoI.  ``make_case`` therefore works per row: ``noise`` = the largest difference of any
pre-activation (P1, P2) between a CPU fp64 and a CPU fp32 forward; a row (RoI r, row i) is *unclear* when any of its
320 pre-activations is within ``KINK_FACTOR * noise`` of zero in fp64; ``grad_out`` is zeroed on unclear rows.  A zero dY
row gives zero dZ2, dA1, dZ1 rows whatever the masks are, so every output of the backward is compared in full.  At most
``MAX_UNCLEAR`` of the rows of a case may be zeroed (asserted).
"""
import functools

import torch
import torch.nn.functional as F

C, DD, EPS = 256, 64, 1e-5
KINK_FACTOR, MAX_UNCLEAR = 8, 0.03
# (K, R, extra params columns): the operator cases of the GPU file; (37, 49) has strided params rows
OPERATOR_CASES = [(600, 49, 0), (37, 49, 64), (1, 49, 0), (300, 64, 0), (5, 7, 0), (1200, 49, 0)]
PADDING_CASES = [(40, 7, 0), (40, 49, 0)]          # LayerNorm biases = +2: padded rows would pass the ReLUs
OUTPUTS = ("feats", "params", "g1", "b1", "g2", "b2")


def split_params(params, K):
    return params[:, : C * DD].reshape(K, C, DD), params[:, C * DD: 2 * C * DD].reshape(K, DD, C)


def forward_stages(feats, params, g1, b1, g2, b2):
    """(P1, P2, Y) of the module formulation in the dtype of the arguments."""
    k1, k2 = split_params(params, feats.shape[0])
    p1 = F.layer_norm(torch.bmm(feats, k1), (DD,), g1, b1, EPS)
    p2 = F.layer_norm(torch.bmm(torch.relu(p1), k2), (C,), g2, b2, EPS)
    return p1, p2, torch.relu(p2)


def autograd_backward(case, dtype):
    """{output name: gradient} through autograd of the module formulation, on the CPU in ``dtype``."""
    t = {k: case[k].detach().to(dtype).clone().requires_grad_() for k in OUTPUTS}      # clone: the cached case stays as built
    y = forward_stages(*(t[k] for k in OUTPUTS))[2]
    grads = torch.autograd.grad(y, [t[k] for k in OUTPUTS], case["grad_out"].to(dtype))
    return dict(zip(OUTPUTS, grads))


def _ln_backward(G, z, g, n):
    """dZ, dg, db of LayerNorm over the last n entries (biased variance, eps inside the root) given G = dL/dP."""
    mean = z.mean(-1, keepdim=True)
    rstd = ((z - mean).pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    zh = (z - mean) * rstd
    h = G * g
    dz = rstd * (h - h.mean(-1, keepdim=True) - zh * (h * zh).mean(-1, keepdim=True))
    return dz, (G * zh).sum((0, 1)), G.sum((0, 1))


def restated_backward(case, dtype=torch.float64):
    """The backward the kernel implements, line by line (csrc/dynconv_backward.hip), in plain tensor arithmetic."""
    x, params, g1, b1, g2, b2 = (case[k].to(dtype) for k in OUTPUTS)
    dy = case["grad_out"].to(dtype)
    K = x.shape[0]
    k1, k2 = split_params(params, K)
    z1 = torch.bmm(x, k1)
    p1 = F.layer_norm(z1, (DD,), g1, b1, EPS)
    a1 = torch.relu(p1)
    z2 = torch.bmm(a1, k2)
    p2 = F.layer_norm(z2, (C,), g2, b2, EPS)
    dz2, dg2, db2 = _ln_backward(dy * (p2 > 0), z2, g2, C)
    dk2 = torch.bmm(a1.transpose(1, 2), dz2)
    da1 = torch.bmm(dz2, k2.transpose(1, 2))
    dz1, dg1, db1 = _ln_backward(da1 * (p1 > 0), z1, g1, DD)
    dk1 = torch.bmm(x.transpose(1, 2), dz1)
    dx = torch.bmm(dz1, k1.transpose(1, 2))
    dparams = torch.zeros_like(params)
    dparams[:, : C * DD] = dk1.reshape(K, -1)
    dparams[:, C * DD: 2 * C * DD] = dk2.reshape(K, -1)
    return {"feats": dx, "params": dparams, "g1": dg1, "b1": db1, "g2": dg2, "b2": db2}


@functools.lru_cache(maxsize=None)
def make_case(K, R, extra=0, bias=None, seed=None):
    """feats N(0,1), params N(0,1)/8, LayerNorm weights N(1,0.3), biases N(0,0.3) (or the constant ``bias``), grad_out
    N(0,1) with the unclear rows zeroed; fp32 CPU tensors plus the bookkeeping of the kink rule."""
    g = torch.Generator().manual_seed(1000 * K + R if seed is None else seed)
    case = {"feats": torch.randn(K, R, C, generator=g), "params": torch.randn(K, 2 * C * DD + extra, generator=g) / 8}
    for n, width in (("1", DD), ("2", C)):
        case["g" + n] = 1 + 0.3 * torch.randn(width, generator=g)
        case["b" + n] = 0.3 * torch.randn(width, generator=g) if bias is None else torch.full((width,), float(bias))
    grad_out = torch.randn(K, R, C, generator=g)
    p64 = forward_stages(*(case[k].double() for k in OUTPUTS))
    p32 = forward_stages(*(case[k] for k in OUTPUTS))
    noise = max((p32[i].double() - p64[i]).abs().max().item() for i in (0, 1))
    margin = KINK_FACTOR * noise
    unclear = (p64[0].abs().min(-1).values < margin) | (p64[1].abs().min(-1).values < margin)      # [K,R]
    fraction = unclear.float().mean().item()
    assert fraction <= MAX_UNCLEAR, f"({K},{R}): {fraction:.2%} of the rows are within {margin:.2e} of a ReLU kink"
    case["grad_out"] = grad_out * (~unclear)[..., None]
    case.update(noise=noise, unclear=unclear, fraction=fraction, p2_positive=p64[1] > 0)
    return case


def rel_err(got, ref):
    """max |got - ref| relative to the gradient's largest magnitude."""
    return ((got.double() - ref.double()).abs().max() / ref.abs().max().clamp(min=1e-300)).item()


class Norm:
    """The attributes dfx.ops reads of an nn.LayerNorm."""

    def __init__(self, weight, bias):
        self.weight, self.bias, self.eps, self.normalized_shape = weight, bias, EPS, tuple(weight.shape)
