"""CPU references of the residual + dropout + LayerNorm tail (dfx.ops.add_layernorm_train):
out = F.layer_norm(residual + x * mask) and its four gradients by CPU autograd, in fp64 (the reference) and in fp32 (the
yardstick: the project's rule, tests/_linear_train_cases.py, allows the GPU YARDSTICK_FACTOR times the fp32 CPU's own error).
Computed once per case and shared; callers do not modify what they get."""
import functools

import torch
import torch.nn.functional as F

from tests._linear_train_cases import YARDSTICK_FACTOR, rel_err  # noqa: F401

EPS = 1e-5
P = 0.25
OUTPUTS = ("out", "grad_x", "grad_residual", "grad_gamma", "grad_beta")
# 1, 5: fewer rows than the four waves of a workgroup and a partial second forward workgroup; 67: a partial last workgroup
# of both launches (forward 17 x 4, backward grid 5 = 20 waves: 7 waves walk four rows, 13 walk three);
# 17: backward grid 2 = 8 waves, wave 0 walks rows 0, 8, 16 and the seven others two rows each
ROWS = (1, 5, 67, 17)
# 4: one lane of 64; 64: 16 lanes; 256: one whole chunk; 260: a second chunk with one lane; 1024: all four chunks
COLS = (4, 64, 256, 260, 1024)


def make_case(rows, C, residual=True, mask=True, seed=0):
    g = torch.Generator().manual_seed(1000 * rows + C + seed)
    case = {"x": torch.randn(rows, C, generator=g), "gamma": 1 + 0.5 * torch.randn(C, generator=g),
            "beta": torch.randn(C, generator=g), "grad_out": torch.randn(rows, C, generator=g),
            "residual": torch.randn(rows, C, generator=g) if residual else None, "mask": None}
    if mask:        # 0 or the fp32 value of 1 / (1 - P), as F.dropout leaves it
        case["mask"] = (torch.rand(rows, C, generator=g) >= P).float() / (1 - P)
    return case


def autograd(case, dtype):
    """{output: tensor} of F.layer_norm(residual + x * mask) and its gradients in ``dtype`` on the CPU"""
    t = {k: None if v is None else v.detach().clone().to(dtype) for k, v in case.items()}       # (never the case's own tensors)
    leaves = {"grad_x": t["x"].requires_grad_(), "grad_gamma": t["gamma"].requires_grad_(), "grad_beta": t["beta"].requires_grad_()}
    if t["residual"] is not None:
        leaves["grad_residual"] = t["residual"].requires_grad_()
    s = t["x"] if t["mask"] is None else t["x"] * t["mask"]
    if t["residual"] is not None:
        s = t["residual"] + s
    out = F.layer_norm(s, (s.shape[-1],), t["gamma"], t["beta"], EPS)
    grads = torch.autograd.grad(out, list(leaves.values()), t["grad_out"])
    return dict(zip(leaves, (g.detach() for g in grads)), out=out.detach())


@functools.lru_cache(maxsize=None)
def prepared(rows, C, residual=True, mask=True):
    """(case, fp64 reference, fp32 CPU yardstick)"""
    case = make_case(rows, C, residual, mask)
    return case, autograd(case, torch.float64), autograd(case, torch.float32)
