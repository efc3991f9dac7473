"""nn.MultiheadAttention (no masks) on the hand-written kernels: joint input projections on the MFMA GEMM, one fused
attention launch (dfx_mha.h), output projection on the GEMM.

The library path spends ~12 launches per call on 300 x 300 problems (projection pieces, scaling, two
transposing copies, bmm, softmax, bmm, copy, projection); the 27 calls of a clip step are a fifth of its
launches.  Arithmetic is the module's own: q = (x_q W_q^T + b_q) / sqrt(d), softmax(q k^T) v, out_proj.
Inputs and output are batch-first [B, L, E] (the callers held batch-first tensors and transposed them
only for the module).

In grad mode (``_train_forward``) the projections are F.linear on the module's own parameter slices, under autograd, and
the part in between is dfx.ops.mha with its fused backward (csrc/mha_backward.hip): no [B*heads, Lq, Lk] tensor is kept
for the backward except the dropout mask of a module that drops (train mode, dropout > 0).
"""
import math
import os

import torch
import torch.nn.functional as F

from dfx import ops as _ops

from .fused import apply_post, derived_key, has_hooks, post_is_fusable

# grad mode on the fused attention forward + backward; DFX_MHA_TRAIN=0 keeps nn.MultiheadAttention itself (A/B runs).
# Read once at import.
MHA_TRAIN = os.environ.get("DFX_MHA_TRAIN", "1") != "0"


def usable(mha, *tensors):
    """On the GPU in fp32 with 32-wide heads and a packed in_proj the fused route applies.  It never calls the module or
    its out_proj, so in grad mode a hook on either selects the module route (under no_grad hooks are ignored, as they
    always were), and so does DFX_MHA_TRAIN=0."""
    if not (mha.in_proj_weight is not None and mha.head_dim == 32
            and mha.in_proj_bias is not None and not mha.batch_first and mha.bias_k is None and not mha.add_zero_attn
            and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)):
        return False
    if not torch.is_grad_enabled():
        return True
    return MHA_TRAIN and not (has_hooks(mha) or has_hooks(mha.out_proj))


def attention_dropout_mask(mha, B, Lq, Lk, device):
    """The mask nn.MultiheadAttention would draw in this call, [B*heads, Lq, Lk] with values 0 or 1/(1-p) (row b*heads + h),
    or None when the module does not drop (eval mode or dropout == 0).  The module's only random draw is
    F.dropout(weights [B*heads, Lq, Lk], p): the same call on a tensor of ones of that shape takes the same numbers from
    the generator, so a fixed seed gives both routes the same mask.  Runs on CPU tensors too."""
    if not (mha.training and mha.dropout > 0):
        return None
    return F.dropout(torch.ones(B * mha.num_heads, Lq, Lk, dtype=torch.float32, device=device), mha.dropout, True)


def project_kv(mha, pool):
    """K and V projections of a POOL of key / value rows [rows, E] in one GEMM -> [rows, 2E] ([K | V]); rows gathered from it
    are the projections of the gathered rows (a Linear is row-wise), so a pool shared by many queries' key sets is projected once."""
    E = mha.embed_dim
    return _ops.linear(pool.contiguous(), mha.in_proj_weight[E:], mha.in_proj_bias[E:])


def project_kv_stack(mhas, pool):
    """``project_kv`` of several attention modules over the SAME pool in one launch (weights stacked along N, every result a
    contiguous [rows, 2E] tensor: dfx.ops.linear(col_block=2E)) - the three temporal query encoders of TransVOD++ pick from one
    pool of reference queries.  -> list of [rows, 2E]"""
    E = mhas[0].embed_dim
    key = derived_key(*(t for m in mhas for t in (m.in_proj_weight, m.in_proj_bias)))
    cache = mhas[0].__dict__.get("_kv_stack")
    if cache is None or cache[0] != key:
        cache = (key, torch.cat([m.in_proj_weight[E:] for m in mhas], 0).contiguous(),
                 torch.cat([m.in_proj_bias[E:] for m in mhas], 0).contiguous())
        mhas[0]._kv_stack = cache
    out = _ops.linear(pool.contiguous(), cache[1], cache[2], col_block=2 * E)          # [n, rows, 2E]
    return [out[i] for i in range(len(mhas))]


def forward(mha, q_in, k_in, v_in, post=None, kv=None):
    """mha: nn.MultiheadAttention; q_in [B,Lq,E], k_in / v_in [B,Lk,E] -> [B,Lq,E]
    (= mha(q_in^T, k_in^T, v_in^T)[0]^T of the module; no caller uses the attention weights).
    post = (residual [B,Lq,E], norm[, dropout]): -> norm(residual + dropout(output)): out_proj's GEMM, then the add and the
    LayerNorm in one add_layernorm launch (dfx.ops.linear(norm=...)) when the dropout is the identity (eval mode).
    kv [B,Lk,2E]: already projected keys / values (``project_kv`` rows); k_in / v_in are then ignored."""
    if torch.is_grad_enabled():
        if kv is not None:
            raise RuntimeError("fused_mha.forward: already projected keys / values (kv=) are an inference shortcut; "
                               "in grad mode pass k_in and v_in")
        return _train_forward(mha, q_in, k_in, v_in, post)
    E, H = mha.embed_dim, mha.num_heads
    W, b = mha.in_proj_weight, mha.in_proj_bias
    B, Lq, _ = q_in.shape
    if kv is not None:
        q = _ops.linear(q_in.contiguous(), W[:E], b[:E]).view(B, Lq, E)
        ctx = _ops.mha(q, kv[..., :E], kv[..., E:], H, 1.0 / math.sqrt(E // H))
        if post_is_fusable(post) and E == 256:
            return _ops.linear(ctx, mha.out_proj.weight, mha.out_proj.bias, residual=post[0].contiguous(), norm=post[1])
        out = _ops.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)
        return apply_post(post, out)
    Lk = k_in.shape[1]
    same_qk, same_kv = q_in is k_in, k_in is v_in
    q_in, k_in, v_in = q_in.contiguous(), k_in.contiguous(), v_in.contiguous()
    if same_qk and same_kv:                                 # one projection for q, k, v
        qkv = _ops.linear(q_in, W, b).view(B, Lq, 3 * E)
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    elif same_qk:                                           # self-attention with positional q / k, plain v
        qk = _ops.linear(q_in, W[:2 * E], b[:2 * E]).view(B, Lq, 2 * E)
        q, k = qk[..., :E], qk[..., E:]
        v = _ops.linear(v_in, W[2 * E:], b[2 * E:]).view(B, Lk, E)
    else:
        q = _ops.linear(q_in, W[:E], b[:E]).view(B, Lq, E)
        k = _ops.linear(k_in, W[E:2 * E], b[E:2 * E]).view(B, Lk, E)
        v = _ops.linear(v_in, W[2 * E:], b[2 * E:]).view(B, Lk, E)
    ctx = _ops.mha(q, k, v, H, 1.0 / math.sqrt(E // H))
    if post_is_fusable(post) and E == 256:
        return _ops.linear(ctx, mha.out_proj.weight, mha.out_proj.bias, residual=post[0].contiguous(), norm=post[1])
    out = _ops.linear(ctx, mha.out_proj.weight, mha.out_proj.bias)
    return apply_post(post, out)


def _train_forward(mha, q_in, k_in, v_in, post):
    """``forward`` in grad mode: the projections as F.linear on slices of the module's own parameters (autograd, library
    GEMM), dfx.ops.mha with the module's dropout mask in between, ``post`` unfused."""
    E, H = mha.embed_dim, mha.num_heads
    W, b = mha.in_proj_weight, mha.in_proj_bias
    B, Lq, _ = q_in.shape
    Lk = k_in.shape[1]
    if q_in is k_in and k_in is v_in:                       # one projection; q, k, v are its column blocks (strided views)
        q, k, v = F.linear(q_in, W, b).view(B, Lq, 3, E).unbind(2)
    elif q_in is k_in:
        q, k = F.linear(q_in, W[:2 * E], b[:2 * E]).view(B, Lq, 2, E).unbind(2)
        v = F.linear(v_in, W[2 * E:], b[2 * E:])
    else:
        q = F.linear(q_in, W[:E], b[:E])
        k = F.linear(k_in, W[E:2 * E], b[E:2 * E])
        v = F.linear(v_in, W[2 * E:], b[2 * E:])
    drop = attention_dropout_mask(mha, B, Lq, Lk, q_in.device)
    ctx = _ops.mha(q, k, v, H, 1.0 / math.sqrt(E // H), drop=drop)
    return apply_post(post, F.linear(ctx, mha.out_proj.weight, mha.out_proj.bias))
