"""``MSDeformAttn``: the multi-scale deformable attention module, reference surface
(/root/reference/models/ops/modules/ms_deform_attn.py:30-117) on the gfx950 kernels.

Same constructor, parameter names (``sampling_offsets``, ``attention_weights``,
``value_proj``, ``output_proj`` -> same state_dict keys), initialisation and forward
signature as the reference.  Four execution routes, the first that applies:

* "level": inference on the GPU, fp32, one level that fits a CU's LDS under many queries (encoder, depth fusion) with the
  host sizes riding on the shapes tensor: the level-in-LDS kernel (csrc/msda_level.hip) between projections that exchange
  block-major operands with it (``dfx.ops.level_supported``);
* "fused": inference on the GPU with the production head geometry (8 heads x 32 channels, 4 points,
  <= 4 levels, fp32): ONE GEMM produces [offsets | logits] per query and the fused kernel
  (csrc/msda_fused.hip) does softmax, location arithmetic and sampling in one launch;
* "train": training (grad mode) on the GPU with the same geometry, fp32, no autocast and one reference level
  per value level: the four Linear layers under autograd, and between them the same fused kernel
  with the fused backward (csrc/msda_fused_backward.hip) behind it (``dfx.ops.msda_fused``);
* "operator": anything else (fp64, autocast, odd geometry, the temporal decoder's flat read in grad mode, DFX_MSDA_TRAIN=0):
  the reference's op sequence with the autograd operator ``MSDeformAttnFunction``
  (csrc/msda_forward.hip / msda_backward.hip).

There is no CPU route: like the reference's op (ms_deform_attn.h:38) it raises on CPU tensors.
"""
import math
import os
import warnings

import torch
import torch.nn.functional as F
from torch import nn

from models.fused import Linear, apply_post, derived_key, post_is_fusable

from dfx import ops as _ops
from ..functions import ms_deform_attn_func as _func


# MSDeformAttn in grad mode on the fused forward + fused backward (csrc/msda_fused_backward.hip); DFX_MSDA_TRAIN=0 keeps
# the reference's op sequence with MSDeformAttnFunction (A/B runs).  Read once at import.
MSDA_TRAIN = os.environ.get("DFX_MSDA_TRAIN", "1") != "0"


def _is_power_of_2(n):
    if not isinstance(n, int) or n < 0:
        raise ValueError(f"invalid input for _is_power_of_2: {n} (type: {type(n)})")
    return n != 0 and (n & (n - 1)) == 0


class MSDeformAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model must be divisible by n_heads, but got {d_model} and {n_heads}")
        if not _is_power_of_2(d_model // n_heads):
            warnings.warn("MSDeformAttn: a power-of-2 head dimension maps best onto the kernels "
                          "(32 channels per head takes the wave-per-query fast path).")
        self.im2col_step = 64
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        mlp = n_heads * n_levels * n_points
        self.sampling_offsets = Linear(d_model, mlp * 2)
        self.attention_weights = Linear(d_model, mlp)
        self.value_proj = Linear(d_model, d_model)
        self.output_proj = Linear(d_model, d_model)
        self._reset_parameters()

    def _reset_parameters(self):
        """ref :62-76 - zero offset weights, ring-shaped offset bias (head h points along angle
        2*pi*h/n_heads, point i at radius i+1), zero attention logits, xavier projections."""
        with torch.no_grad():
            self.sampling_offsets.weight.zero_()
            angle = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
            ring = torch.stack([angle.cos(), angle.sin()], -1)
            ring = ring / ring.abs().max(-1, keepdim=True)[0]
            ring = ring.view(self.n_heads, 1, 1, 2).repeat(1, self.n_levels, self.n_points, 1)
            ring = ring * torch.arange(1, self.n_points + 1, dtype=torch.float32).view(1, 1, -1, 1)
            self.sampling_offsets.bias = nn.Parameter(ring.reshape(-1))
            self.attention_weights.weight.zero_()
            self.attention_weights.bias.zero_()
            nn.init.xavier_uniform_(self.value_proj.weight)
            self.value_proj.bias.zero_()
            nn.init.xavier_uniform_(self.output_proj.weight)
            self.output_proj.bias.zero_()

    # -- one GEMM for both query projections (weights concatenated lazily, refreshed when edited) --
    def _qproj_params(self):
        so, aw = self.sampling_offsets, self.attention_weights
        key = derived_key(so.weight, so.bias, aw.weight, aw.bias) + (so.weight.device, so.weight.dtype)
        cache = self.__dict__.get("_qproj_cache")
        if cache is None or cache[0] != key:
            w = torch.cat([so.weight.detach(), aw.weight.detach()], 0).contiguous()
            b = torch.cat([so.bias.detach(), aw.bias.detach()], 0).contiguous()
            self._qproj_cache = (key, w, b)
        return self._qproj_cache[1], self._qproj_cache[2]

    def _qproj_params_by_head(self):
        """The joint projection with its output columns regrouped per head - [8 offsets | 4 logits] x n_heads
        (n_levels == 1) - so that a col_block=12 GEMM writes what one workgroup of the level-in-LDS kernel
        reads as one contiguous slab."""
        w, b = self._qproj_params()
        if self._qproj_cache[0] != self.__dict__.get("_qproj_head_key"):
            M, P = self.n_heads, self.n_points
            so = torch.arange(M * P * 2, device=w.device).view(M, P * 2)
            aw = torch.arange(M * P, device=w.device).view(M, P) + M * P * 2
            order = torch.cat([so, aw], 1).reshape(-1)
            self._qproj_head = (w[order].contiguous(), b[order].contiguous())
            self._qproj_head_key = self._qproj_cache[0]
        return self._qproj_head

    def _route(self, q_parts, reference_points, input_flatten, value, host):
        """Which kernels run this call: "level", "fused", "train" or "operator" (the module docstring, in that order)."""
        M, L, P = self.n_heads, self.n_levels, self.n_points
        D, Lq, Lr = self.d_model // M, q_parts[0].shape[1], reference_points.shape[2]
        no_grad = not torch.is_grad_enabled() or not (any(t.requires_grad for t in q_parts) or input_flatten.requires_grad)
        if no_grad and input_flatten.is_cuda and input_flatten.dtype == torch.float32 \
                and _ops.fused_supported(input_flatten, M, D, L, P, Lr):
            if host is not None and _ops.level_supported(input_flatten, host[0][0], host[0][1], Lq, M, D, L, P, Lr):
                return "level"
            return "fused"
        v = input_flatten if value is None else value          # (value_proj keeps device and, outside autocast, dtype)
        q_dtype = torch.promote_types(q_parts[0].dtype, q_parts[-1].dtype)            # of the summed (src, pos) pair
        if (MSDA_TRAIN and v.is_cuda and not torch.is_autocast_enabled() and Lr == L
                and v.dtype == q_dtype == reference_points.dtype == torch.float32 and _ops.fused_supported(v, M, D, L, P, Lr)):
            return "train"
        return "operator"

    def _project_values(self, input_flatten, input_padding_mask, kernel, col_block=0):
        """value_proj with the padded tokens zeroed: one GEMM launch with the mask in its epilogue (``kernel``), else the
        Linear module and a masked_fill."""
        if kernel:
            return _ops.linear(input_flatten.contiguous(), self.value_proj.weight, self.value_proj.bias,
                               row_mask=input_padding_mask, col_block=col_block)
        value = self.value_proj(input_flatten)
        return value if input_padding_mask is None else value.masked_fill(input_padding_mask[..., None], float(0))

    def _project_output(self, sampled, post, N, Lq, fuse_post=False, blocked=False):
        """output_proj and ``post`` on the sampled values, [N,Lq,C] or (``blocked``) the level kernel's [C/4, N*Lq, 4];
        fuse_post: the add and the LayerNorm of a fusable post ride behind the GEMM (dfx.ops.linear(norm=...))."""
        proj = self.output_proj
        if fuse_post and post_is_fusable(post) and self.d_model == 256:
            out = _ops.linear(sampled, proj.weight, proj.bias, x_blocked=blocked, residual=post[0].contiguous(), norm=post[1])
            return out.view(N, Lq, -1) if blocked else out
        out = _ops.linear(sampled, proj.weight, proj.bias, x_blocked=True).view(N, Lq, -1) if blocked else proj(sampled)
        return apply_post(post, out)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None, post=None, value=None):
        """query [N,Lq,C] (or a (tensor, positional_embedding) pair whose sum is the query: the add is
        then fused into the projection GEMM); reference_points [N,Lq,L,2] (or 4: cx,cy,w,h) in [0,1];
        input_flatten [N,sum(H_l*W_l),C]; input_spatial_shapes i64 [L,2]; input_level_start_index
        i64 [L]; input_padding_mask [N,S] True = padding.  -> [N,Lq,C]   (ref :78-117)
        post = (residual, norm[, dropout]): return ``norm(residual + dropout(output))`` instead - what every caller does
        next; on the fused GPU routes, and when the dropout is the identity (eval mode), the add and the LayerNorm are one
        add_layernorm launch behind output_proj's GEMM (dfx.ops.linear(norm=...)).
        value [N,S,C]: ``value_proj(input_flatten)`` with the padded tokens already zeroed, when the caller projected the
        values of several layers that share ``input_flatten`` in one launch (``project_values``); the single-level
        many-query route (block-major operands) ignores it."""
        q_parts = query if isinstance(query, tuple) else (query,)
        N, Lq, _ = q_parts[0].shape
        _, S, _ = input_flatten.shape
        M, L, P = self.n_heads, self.n_levels, self.n_points
        D = self.d_model // M
        if getattr(input_spatial_shapes, "_dfx_tokens", None) != S:
            # one device read per distinct shapes tensor (the reference asserts on every call, ref :92)
            assert int((input_spatial_shapes[:, 0] * input_spatial_shapes[:, 1]).sum()) == S
            input_spatial_shapes._dfx_tokens = S
        ref_dim = reference_points.shape[-1]
        if ref_dim not in (2, 4):
            raise ValueError(f"Last dim of reference_points must be 2 or 4, but get {ref_dim} instead.")

        host = getattr(input_spatial_shapes, "_dfx_host", None)
        route = self._route(q_parts, reference_points, input_flatten, value, host)
        if route in ("level", "fused"):
            # value_proj (+ masked_fill of padded tokens), [offsets | logits] in one GEMM (+ the caller's ``src + pos`` add
            # when handed over as a (src, pos) pair), fused sampling.  "level": the level lives in LDS and the three
            # projections exchange block-major operands with the kernel (include/dfx_msda.h); a handed-over ``value`` is
            # row-major and not used
            level = route == "level"
            w, b = self._qproj_params_by_head() if level else self._qproj_params()
            if level or value is None:
                value = self._project_values(input_flatten, input_padding_mask, True, col_block=4 if level else 0)
            qproj = _ops.linear(q_parts[0].contiguous(), w, b, add=q_parts[1].contiguous() if len(q_parts) > 1 else None,
                                col_block=12 if level else 0)
            if level:
                sampled = _ops.msda_level_forward(value, reference_points, qproj, N, host[0][0], host[0][1])
            else:
                sampled = _ops.msda_fused_forward(value.view(N, S, M, D), input_spatial_shapes, input_level_start_index,
                                                  reference_points, qproj, L, P)
            return self._project_output(sampled, post, N, Lq, fuse_post=True, blocked=level)

        query = q_parts[0] + q_parts[1] if len(q_parts) > 1 else query
        if value is None:
            value = self._project_values(input_flatten, input_padding_mask, False)
        value = value.view(N, S, M, D)
        if route == "train":
            # grad mode on the fused front end: the four Linear layers stay the modules they are, what lies between
            # them is one launch forwards and one backwards (csrc/msda_fused.hip, csrc/msda_fused_backward.hip);
            # no sampling_locations / attention_weights tensors exist, the node saves the Linear outputs only
            sampled = _ops.msda_fused(value.contiguous(), input_spatial_shapes, input_level_start_index, reference_points,
                                      self.sampling_offsets(query), self.attention_weights(query), L, P)
            return self._project_output(sampled, post, N, Lq)

        offsets = self.sampling_offsets(query).view(N, Lq, M, L, P, 2)
        weights = F.softmax(self.attention_weights(query).view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
        if ref_dim == 2:
            wh = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
            locations = reference_points[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        else:
            locations = reference_points[:, :, None, :, None, :2] \
                + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        locations = locations.contiguous()
        if reference_points.shape[2] != L and N > 1:
            # flat read of an over-long location tensor (TransVOD temporal decoder): the
            # reference only does this with N == 1; each batch element follows that rule on its own
            sampled = torch.cat([_func.MSDeformAttnFunction.apply(
                value[b:b + 1].contiguous(), input_spatial_shapes, input_level_start_index,
                locations[b:b + 1].contiguous(), weights[b:b + 1].contiguous(), self.im2col_step)
                for b in range(N)], 0)
        else:
            sampled = _func.MSDeformAttnFunction.apply(value, input_spatial_shapes, input_level_start_index,
                                                       locations, weights, self.im2col_step)
        return self._project_output(sampled, post, N, Lq)


_STACK_VALUES = os.environ.get("DFX_VALUE_STACK", "1") == "1"          # 0: every layer projects its own values (A/B runs)


def project_values(attns, input_flatten, input_padding_mask=None):
    """``value_proj`` of several MSDeformAttn modules over the SAME ``input_flatten`` [N,S,C] in ONE GEMM launch (weights
    stacked along N, every result a contiguous [N,S,C] tensor of its own: dfx.ops.linear(col_block=C)) with the padded tokens
    zeroed - the six decoder layers of a frame read one memory, the three temporal decoders one current-frame memory
    (/root/reference/models/deformable_transformer_single.py:703-748, deformable_transformer_multi_plusplus.py:560-599 each
    project it on their own: the same products, the input read once instead of once per layer).
    -> list of value tensors for ``MSDeformAttn.forward(value=...)``, or None where the fused GPU route does not apply."""
    first = attns[0]
    C = first.d_model
    if (not _STACK_VALUES or len(attns) < 2 or torch.is_grad_enabled() or not input_flatten.is_cuda or input_flatten.dtype != torch.float32
            or C % 128 != 0 or any(a.d_model != C or a.value_proj.weight.dtype != torch.float32 or a.value_proj.bias is None
                                   or a.value_proj.weight.device != input_flatten.device for a in attns)):
        return None
    key = derived_key(*(t for a in attns for t in (a.value_proj.weight, a.value_proj.bias)))
    cache = first.__dict__.get("_value_stack")
    if cache is None or cache[0] != key:
        cache = (key, torch.cat([a.value_proj.weight for a in attns], 0).contiguous(),
                 torch.cat([a.value_proj.bias for a in attns], 0).contiguous())
        first._value_stack = cache
    N, S, _ = input_flatten.shape
    out = _ops.linear(input_flatten.contiguous(), cache[1], cache[2], row_mask=input_padding_mask, col_block=C)   # [n, N*S, C]
    return [out[i].view(N, S, C) for i in range(len(attns))]
