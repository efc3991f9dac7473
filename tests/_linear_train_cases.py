"""Cases, the fp64 reference and the fp32 yardstick shared by tests/test_linear_train_cpu.py and tests/test_linear_train_gpu.py.

The operator (dfx.ops.linear_backward; include/dfx_gemm.h, dfx_gemm_wgrad_f32): for y = x W^T + b and a given dY
  grad_x = dY W,   grad_w = dY^T x,   grad_b = sum_m dY[m].
``reference`` writes this down in fp64.  ``yardstick`` computes the same three sums in fp32 on the CPU in the kernel's order:
the rows of the summed dimension one at a time inside each range of the split, the ranges in ascending order; for grad_x one
n at a time.  (A library fp32 matmul on the CPU is no fair yardstick: it blocks its sums and shows a third of the error of a
sequential sum at (1000, 256, 256) - the MFMA adds two rows per instruction and lies in between.)
"""
import functools

import torch

OUTPUTS = ("grad_x", "grad_w", "grad_b")
YARDSTICK_FACTOR = 4      # the GPU may be this many times the CPU's own fp32 error (the project's factor: test_roi_backward_gpu)

# (M, N, K, splits): the smallest problem; one whole 16-row step on exact tiles; a tail of the summed dimension with partial
# tiles on the 64-row tile; N <= 64 with two tile columns; a partial second tile on both axes; 63 steps in 1, 2, 7 and (asked
# for 100) 63 ranges; the encoder FFN's two Linears with the host's own choice (None)
OPERATOR_SHAPES = [(1, 4, 4, None), (16, 128, 128, None), (33, 64, 36, None), (300, 32, 256, None), (300, 132, 200, None),
                   (1000, 256, 256, 1), (1000, 256, 256, 2), (1000, 256, 256, 7), (1000, 256, 256, 100),
                   (4200, 1024, 256, None), (4200, 256, 1024, None)]


def ranges(M, splits):
    """(rows per range, number of ranges) of a request for ``splits`` ranges: the arithmetic of dfx_gemm_splitk_f32 - whole
    16-row steps per range, and as many ranges as are not empty."""
    per = ((M + splits - 1) // splits + 15) // 16 * 16
    return per, (M + per - 1) // per


def make_case(M, N, K, seed=0, grad_scale=1.0):
    """fp64 CPU tensors of fp32-representable values: x [M,K] and grad_out [M,N] standard normal (grad_out times grad_scale),
    weight [N,K] standard normal / sqrt(K), bias [N]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * M + 13 * N + K)
    case = {"x": torch.randn(M, K, generator=g, dtype=torch.float64),
            "grad_out": torch.randn(M, N, generator=g, dtype=torch.float64) * grad_scale,
            "weight": torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5,
            "bias": torch.randn(N, generator=g, dtype=torch.float64)}
    case = {n: t.float().double() for n, t in case.items()}
    case["shape"] = (M, N, K)
    return case


def reference(case):
    go, x, w = case["grad_out"], case["x"], case["weight"]
    return {"grad_x": go @ w, "grad_w": go.t() @ x, "grad_b": go.sum(0)}


def autograd(case):
    """The same three from torch's autograd through F.linear, in fp64."""
    leaves = [case[n].detach().clone().requires_grad_() for n in ("x", "weight", "bias")]
    y = torch.nn.functional.linear(*leaves)
    return dict(zip(OUTPUTS, torch.autograd.grad(y, leaves, case["grad_out"])))


def yardstick(case, splits):
    """The three sums in fp32, sequentially in the kernel's order (see the module docstring)."""
    go, x, w = (case[n].float() for n in ("grad_out", "x", "weight"))
    M, N, K = case["shape"]
    per, n_ranges = ranges(M, splits)
    grad_w, grad_b = None, None
    for s in range(n_ranges):
        pw, pb = torch.zeros(N, K), torch.zeros(N)
        for m in range(s * per, min(M, (s + 1) * per)):
            pw += torch.outer(go[m], x[m])
            pb += go[m]
        grad_w, grad_b = (pw, pb) if grad_w is None else (grad_w + pw, grad_b + pb)
    grad_x = torch.zeros(M, K)
    for n in range(N):
        grad_x += torch.outer(go[:, n], w[n])
    return {"grad_x": grad_x, "grad_w": grad_w, "grad_b": grad_b}


@functools.lru_cache(maxsize=None)
def prepared(M, N, K, splits, grad_scale=1.0):
    """(case, fp64 reference, fp32 yardstick for ``splits`` ranges), computed once per case and never modified"""
    case = make_case(M, N, K, grad_scale=grad_scale)
    return case, reference(case), yardstick(case, splits)


def rel_err(got, ref):
    """largest absolute error relative to the reference's largest magnitude (tests/_mha_cases.py)"""
    err, top = (got.double() - ref.double()).abs().max().item(), ref.double().abs().max().item()
    return err if top == 0 else err / top


def host_splits(M, N, K, splits):
    """the number of ranges a case runs with: its own, or (None) the host rule's"""
    if splits is not None:
        return splits
    from dfx import ops
    return ops._wgrad_splits(M, N, K)
