"""Cases and the fp64 restatement shared by tests/test_mha_backward_cpu.py and tests/test_mha_backward_gpu.py.

The operator (include/dfx_mha.h): per head h of width 32, with S = scale * q_h k_h^T [Lq, Lk],
  lse = logsumexp_j S,  P = exp(S - lse),  out_h = (P o drop) v_h
and for a given dO
  delta_i = <dO_i, out_i>,  dP = (dO v^T) o drop,  dS = scale * P o (dP - delta),  dV = (P o drop)^T dO,  dQ = dS k,  dK = dS^T q.
``restated`` writes this down in whatever dtype its inputs have (fp64: the reference; fp32: the yardstick), ``autograd``
gets the same gradients from torch's autograd through softmax(...) * drop @ v.
"""
import torch

D = 32
OUTPUTS = ("out", "lse", "grad_q", "grad_k", "grad_v")
GRADS = ("grad_q", "grad_k", "grad_v")

# (B, heads, Lq, Lk): the smallest problem; exact tiles; one row past / short of a tile on both sides; a partial last query
# wave and a partial last key tile with Lk % 4 != 0; the forward's key-range groups; the layers' own size
OPERATOR_SHAPES = [(2, 8, 1, 1), (1, 8, 64, 32), (2, 8, 33, 31), (1, 2, 65, 97), (1, 8, 70, 130), (2, 8, 300, 300)]
DROP_P = 0.5


def make_case(B, heads, Lq, Lk, p=0.0, seed=0, grad_scale=1.0):
    """fp64 CPU tensors (of fp32-representable values) q [B,Lq,E], k / v [B,Lk,E], grad_out [B,Lq,E], drop [B,heads,Lq,Lk] or None (values 0 or 1/(1-p)).
    q and k are standard normal, so the scores scale * <q,k> at scale = 1/sqrt(32) are of order one, as in the layers."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Lq + 13 * Lk + B + heads)
    E = D * heads
    case = {n: torch.randn(B, L, E, generator=g, dtype=torch.float64) for n, L in (("q", Lq), ("k", Lk), ("v", Lk))}
    case["grad_out"] = torch.randn(B, Lq, E, generator=g, dtype=torch.float64) * grad_scale
    for n in ("q", "k", "v", "grad_out"):                   # fp32 numbers: the fp32 runs get exactly the reference's inputs
        case[n] = case[n].float().double()
    case["drop"] = None
    if p > 0:
        keep = torch.rand(B, heads, Lq, Lk, generator=g, dtype=torch.float64) >= p
        case["drop"] = keep.to(torch.float64) / (1 - p)
    case.update(heads=heads, scale=1.0 / D ** 0.5, shape=(B, heads, Lq, Lk))
    return case


def cast(case, dtype):
    return {n: (t.to(dtype) if torch.is_tensor(t) else t) for n, t in case.items()}


def _split(t, heads):
    B, L, _ = t.shape
    return t.view(B, L, heads, D).permute(0, 2, 1, 3)          # [B,heads,L,32]


def _join(t):
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * D)


def restated(case):
    """{out, lse, grad_q, grad_k, grad_v} by the formulas above, in the dtype of the case's tensors."""
    H, scale, drop = case["heads"], case["scale"], case["drop"]
    q, k, v, go = (_split(case[n], H) for n in ("q", "k", "v", "grad_out"))
    S = scale * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    Pd = P if drop is None else P * drop
    out = Pd @ v
    delta = (go * out).sum(-1, keepdim=True)
    dP = go @ v.transpose(-1, -2)
    if drop is not None:
        dP = dP * drop
    dS = scale * P * (dP - delta)
    return {"out": _join(out), "lse": lse, "grad_q": _join(dS @ k), "grad_k": _join(dS.transpose(-1, -2) @ q),
            "grad_v": _join(Pd.transpose(-1, -2) @ go)}


def autograd(case):
    """The same five through torch's autograd: softmax(scale q k^T) * drop @ v, backward with grad_out."""
    H, scale, drop = case["heads"], case["scale"], case["drop"]
    leaves = {n: case[n].detach().clone().requires_grad_() for n in ("q", "k", "v")}
    q, k, v = (_split(leaves[n], H) for n in ("q", "k", "v"))
    S = scale * q @ k.transpose(-1, -2)
    P = torch.softmax(S, -1)
    out = _join((P if drop is None else P * drop) @ v)
    gq, gk, gv = torch.autograd.grad(out, [leaves["q"], leaves["k"], leaves["v"]], case["grad_out"])
    return {"out": out.detach(), "lse": torch.logsumexp(S.detach(), -1), "grad_q": gq, "grad_k": gk, "grad_v": gv}


def rel_err(got, ref):
    """largest absolute error relative to the reference's largest magnitude (the absolute error itself where the reference
    is identically zero: grad_q and grad_k at Lk = 1, where the softmax is constant)"""
    err, top = (got.double() - ref.double()).abs().max().item(), ref.double().abs().max().item()
    return err if top == 0 else err / top


# ---- the module ------------------------------------------------------------------------------------------------
def module_reference(mha, q_in, k_in, v_in, mask, dtype):
    """nn.MultiheadAttention restated with an explicit dropout mask [B*heads, Lq, Lk] (or None), batch-first inputs
    [B,L,E] -> [B,Lq,E], with the module's own parameters cast to ``dtype``; differentiable."""
    E, H = mha.embed_dim, mha.num_heads
    W, b = mha.in_proj_weight.to(dtype), mha.in_proj_bias.to(dtype)
    B, Lq, _ = q_in.shape
    Lk = k_in.shape[1]
    q = torch.nn.functional.linear(q_in, W[:E], b[:E])
    k = torch.nn.functional.linear(k_in, W[E:2 * E], b[E:2 * E])
    v = torch.nn.functional.linear(v_in, W[2 * E:], b[2 * E:])
    q, k, v = (_split(t, H) for t in (q, k, v))
    P = torch.softmax((q / (E // H) ** 0.5) @ k.transpose(-1, -2), -1)
    if mask is not None:
        P = P * mask.to(dtype).view(B, H, Lq, Lk)
    return torch.nn.functional.linear(_join(P @ v), mha.out_proj.weight.to(dtype), mha.out_proj.bias.to(dtype))
