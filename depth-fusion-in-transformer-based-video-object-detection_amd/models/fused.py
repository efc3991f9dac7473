"""Switch for the GPU-only fused inference routes of the host modules.

Default module behaviour is the reference's op-by-op formulation (works on any device through
PyTorch).  ``enable_fused_inference(model)`` turns on, for every module that has one, the route
that runs on the hand-written gfx950 kernels (dfx.ops): folded frozen-BN + fused epilogues in the
ResNet, ... These routes have no CPU implementation and raise on CPU tensors; the MSDA operator
itself is always on the HIP kernels, fused route or not.
"""


def enable_fused_inference(model, enabled=True):
    n = 0
    for mod in model.modules():
        if hasattr(mod, "fused_inference"):
            mod.fused_inference = enabled
            n += 1
    return n


import os

import torch
from torch import nn

# Linear in grad mode on the MFMA GEMM and its weight-gradient kernel (dfx.ops.linear_train, csrc/gemm_wgrad.hip);
# DFX_LINEAR_TRAIN=0 keeps nn.Linear there (A/B measurements).  Read once at import.
LINEAR_TRAIN = os.environ.get("DFX_LINEAR_TRAIN", "1") != "0"
# The widest layer the route takes: out_features up to 1024 (the FFN) is what was measured and what the operator tests cover.
# The input gradient adds its out_features terms one after the other in one MFMA chain; at RCNNHead's dynamic_layer
# (256 -> 32768) that sum is 5.0e-6 from fp64 against the 2.3e-6 tests/test_dynconv_backward_gpu.py allows (4 x the CPU's
# blocked fp32 sum), so wider layers stay on nn.Linear (profiles/r14_linear_train.txt).
LINEAR_TRAIN_MAX_OUT_FEATURES = 1024
# The input projections (models.detector_common._ConvGN) in grad mode on dfx.ops.conv1x1_train and the GroupNorm backward
# kernels (csrc/groupnorm_backward.hip); DFX_CONVGN_TRAIN=0 keeps nn.Sequential there (A/B measurements).  Read once at import.
CONVGN_TRAIN = os.environ.get("DFX_CONVGN_TRAIN", "1") != "0"
# The smallest map (images x H x W pixels) at which that route MEASURED faster than nn.Sequential beyond the repetition spread:
# 12 frames of 50 x 84 (1.05x at 2048 -> 256, 1.15x at 128 -> 256; 32 frames 1.04x / 1.10x).  8 frames tie and 4 frames are
# 8-15 % slower - a handful of short launches issued from Python against the library's C++ nodes - so smaller maps keep
# nn.Sequential (tools/bench_convgn_train.py, profiles/r15_convgn_train.txt).
CONVGN_TRAIN_MIN_PIXELS = 12 * 50 * 84
# The tail of every sub-layer, norm(residual + dropout(y)), in grad mode on dfx.ops.add_layernorm_train (csrc/layernorm_train.hip: one
# forward launch, two backward launches, the module's own dropout draw) instead of nn.Dropout + add + nn.LayerNorm under autograd;
# DFX_ADDLN_TRAIN=0 keeps the modules (A/B measurements).  Read once at import.  Taken by apply_post, transformer_layers._norm_add and
# the norm(residual + dropout(.)) form of transformer_layers._linear_norm_add for fp32 GPU tensors outside autocast with C % 4 == 0,
# C <= 1024, something to differentiate (needs_grad) and no hooks on the norm or the dropout.
ADDLN_TRAIN = os.environ.get("DFX_ADDLN_TRAIN", "1") != "0"
# The smallest row count at which one tail MEASURED faster than the parent commit's modules beyond the repetition spread: 32 frames of
# 4200 tokens (1.84x with a live dropout, 2.60x without).  12 x 4200 rows tie (1.02x, and 1.26x inside a spread that reaches the parent's
# figure); 4 x 4200 rows and fewer are 20-23 % slower - one tail there is host time, ~0.2 ms whatever the row count, and this route's
# Python node costs more of it than the library's C++ nodes - so fewer rows keep the modules (tools/bench_addln_train.py,
# profiles/r17_addln_train.txt).
ADDLN_TRAIN_MIN_ROWS = 32 * 4200
# The BatchNorms of the DFormer depth stem (models.dformer_backbone.DFormerBackbone) in grad mode on dfx.ops.batch_norm_train
# (csrc/batchnorm_train.hip: batch statistics, the GELU of stage 0 inside the same call, three forward and two backward launches)
# instead of nn.BatchNorm2d + nn.GELU under autograd; DFX_DFORMER_TRAIN=0 keeps the modules everywhere (A/B measurements).  Read
# once at import.  Taken per layer for fp32 GPU tensors outside autocast when something needs a gradient, the BatchNorm is in
# training mode, affine, with a float momentum and without hooks.  The stem's convolutions stay nn.Conv2d.
DFORMER_TRAIN = os.environ.get("DFX_DFORMER_TRAIN", "1") != "0"
# The smallest BatchNorm input (images x H x W pixels) at which one layer, forward + backward, MEASURED faster than the parent
# commit's modules beyond the repetition spread (tools/bench_dformer_train.py, profiles/r18_dformer_train.txt).
# A call costs 0.115 ms whatever its size - five short launches issued from Python - and the library's nodes cost 0.07-0.09 ms:
#   BatchNorm alone: 534400 pixels (8 x 200 x 334 at 32 channels 1.83x, 32 x 100 x 167 at 64 channels 1.97x); 267200 pixels tie
#     (1.07x inside the spread) and 133600 and fewer are 17-45 % SLOWER, so they keep the module;
#   BatchNorm + GELU in one call (stage 0, 16 channels): 533600 pixels = two 400 x 667 maps (alone 2.91x, 32 maps 6.97x; the stem
#     with this layer routed 1.28x at 2 frames).  One map wins alone (1.44x) but LOSES inside the stem (0.77x): a one-frame
#     step is host-bound, and the node's host time shows there in full.  So one map keeps the modules.
DFORMER_TRAIN_MIN_PIXELS = 8 * 200 * 334
DFORMER_TRAIN_MIN_PIXELS_GELU = 2 * 400 * 667

# The FFNs of the transformer layers in GPU inference on the bf16 MFMA GEMM (dfx.ops.linear_bf16, csrc/gemm_bf16.hip): bf16 products,
# fp32 accumulation, the 1024-wide hidden tensor kept in bf16, the residual add and the LayerNorm in fp32.  OFF by default: it
# changes the results (every FFN input and weight is rounded to 8 significant bits; DESIGN.md 4k has the bounds and the
# measured deviation).  DFX_LINEAR_BF16=1 turns it on.  Read once at import; the call sites (transformer_layers._ffn_bf16) read
# this global at call time.  Taken where the fp32 fused FFN is taken today - fp32 GPU activations under no_grad, fp32 weights on
# the same device, identity dropouts, a LayerNorm over 256 columns - when every in_features is a multiple of 8.  A
# ClipRunner(graph=True) has captured the launches of one mode: call refresh() after toggling.
LINEAR_BF16 = os.environ.get("DFX_LINEAR_BF16", "0") == "1"
# No size rule: one FFN (two GEMMs + add_layernorm) MEASURED faster than the fp32 route beyond the repetition spread at every row
# count tried - 1200 -> 413 us at 32 x 4200 rows (2.91x), 480 -> 139 us at 12 x 4200 (3.45x), 185 -> 57 us at 4 x 4200 (3.23x),
# 112 -> 42.5 us at 9600 (2.64x), 50.2 -> 41.6 us at 300 (1.21x: host time there) - and so did the single-Linear GELU FFN of the
# fusion layers (262 -> 157 us at 32 x 4200, 44 -> 28 us at 4 x 4200) (tools/bench_ffn_bf16.py, profiles/r21_ffn_bf16.txt).

# Linear in grad mode on bf16 products with fp32 accumulation (dfx.ops.linear_bf16_train: the forward and the input gradient on
# csrc/gemm_bf16.hip, the weight and bias gradients on csrc/gemm_bf16_wgrad.hip), fp32 tensors in and out of every layer.  OFF by
# default: it changes the results (x, the weight and the incoming gradient are rounded to 8 significant bits inside the three
# products; DESIGN.md 4l has the bounds).  DFX_LINEAR_BF16_TRAIN=1 turns it on.  Read once at import, consulted by
# Linear.forward at call time; independent of LINEAR_BF16 (which is for no_grad).  Taken where ops.linear_train is taken today
# when in_features and out_features are multiples of 8, out_features <= LINEAR_TRAIN_MAX_OUT_FEATURES and the call is large
# enough (below).
LINEAR_BF16_TRAIN = os.environ.get("DFX_LINEAR_BF16_TRAIN", "0") == "1"
# The smallest call the route takes, in elements of the layer's input and output together, rows x (in_features + out_features):
# the fp32 traffic that each of the three memory-bound products moves.  It is the smallest call that MEASURED faster than the
# fp32 route beyond the repetition spread in both runs of tools/bench_linear_bf16_train.py (profiles/r22_linear_bf16_train.txt;
# forward + backward of one layer, run A / run B): 12 x 4200 rows of 256 -> 64, 144 -> 97 us (1.48x) / 144 -> 100 us (1.44x).
# Every larger call won in both runs: 32 x 4200 rows 1722 -> 632 us (2.72x / 2.71x) at 256 -> 1024, 541 -> 241 us (2.25x / 2.21x)
# at 256 -> 256, 208 -> 127 us (1.64x / 1.63x) at 256 -> 32; 12 x 4200 rows 705 -> 272 us (2.59x / 2.56x) at 256 -> 1024,
# 258 -> 102 us (2.54x / 2.46x) at 256 -> 256; 4 x 4200 rows of 256 -> 1024 285 -> 226 us (1.26x) / 278 -> 98 us (2.82x).
# Below it a pass is host time - 90 us on a quiet host, 200 - 230 us on a busy one, whatever the route - and this route's Python
# node costs ~5 us more of it: 0.91x - 0.98x, inside the spread, at 300 and 9600 rows at every width and at 4 x 4200 rows of
# 256 -> 64 / 32; 12 x 4200 rows of 256 -> 32 0.94x / 1.24x and 4 x 4200 rows of 256 -> 256 0.94x / 1.54x, inside the spread both
# times.  Those keep the fp32 route.
LINEAR_BF16_TRAIN_MIN_ELEMENTS = 12 * 4200 * (256 + 64)


def derived_key(*sources):
    """The "have the sources changed" key of every tensor kept by an inference route that was DERIVED from weights (folded BN,
    transformed / re-ordered filters, stacked projection matrices, captured graphs): a tuple of ``(data_ptr, _version)``, one
    entry per source tensor.  A module stands for its own parameters and buffers (``recurse=False``), in definition order; a
    ``None`` (a missing bias) stays ``None``.  The version counter moves under every in-place write that autograd sees
    (``optimizer.step()``, ``load_state_dict``, ``with no_grad(): p.mul_()``), the pointer under every rebinding
    (``p.data = new``, ``load_state_dict(assign=True)``, ``setattr`` of a buffer) - which leaves the counter where it was.
    In-place writes through ``.data`` (``p.data.mul_()``) move neither: ``drop_derived`` is for those."""
    out = []
    for s in sources:
        if s is None:
            out.append(None)
        elif isinstance(s, nn.Module):
            out.extend(None if t is None else (t.data_ptr(), t._version) for t in (*s._parameters.values(), *s._buffers.values()))
        else:
            out.append((s.data_ptr(), s._version))
    return tuple(out)


# every attribute a fused inference route keeps derived tensors in, by the module that holds it
DERIVED_ATTRIBUTES = ("_folded", "_plans1x1", "_chain_carry", "_stem_folded",                   # models/resnet.py, models/dformer_backbone.py
                      "_plan",                                                                   # models/detector_common.py
                      "_qproj_cache", "_qproj_head", "_qproj_head_key", "_value_stack",          # models/ops/modules/ms_deform_attn.py
                      "_kv_stack")                                                               # models/fused_mha.py


# ... and the one the opt-in bf16 FFN route keeps (bf16_weight below).  A tuple of its own: tests/test_weight_updates_cpu.py plants
# exactly the names above and pins their number; drop_derived walks both.
DERIVED_ATTRIBUTES_BF16 = ("_weight_bf16", "_weight_bf16_pair")      # bf16_weight, bf16_weight_pair


def drop_derived(model):
    """Forget every tensor the fused inference routes of ``model`` derived from its weights: the DERIVED_ATTRIBUTES (and
    DERIVED_ATTRIBUTES_BF16) of every submodule and the whole of ``util.memo``.  The next call rebuilds them, exactly as a module
    that has never run would.
    For edits no key can see (``derived_key``), and for whoever wants the memory back.  -> the number of entries dropped.
    (A ``ClipRunner(graph=True)`` keeps captured launches of its own: ``ClipRunner.refresh()``.)"""
    from util import memo
    n = 0
    for mod in model.modules():
        for name in DERIVED_ATTRIBUTES + DERIVED_ATTRIBUTES_BF16:
            if mod.__dict__.pop(name, None) is not None:
                n += 1
    n += len(memo._MEMO)
    memo.clear()
    return n


def bf16_weight(linear):
    """The bf16 copy of a Linear's weight for the LINEAR_BF16 route, [out_features, in_features] contiguous, rounded to nearest
    even (``weight.to(torch.bfloat16)``).  Kept on the module (DERIVED_ATTRIBUTES_BF16) under ``derived_key(weight)`` plus the
    device and rebuilt when that key changes; ``drop_derived`` forgets it."""
    w = linear.weight
    key = (derived_key(w), w.device)
    kept = linear.__dict__.get("_weight_bf16")
    if kept is None or kept[0] != key:
        kept = (key, w.detach().to(torch.bfloat16).contiguous())
        linear._weight_bf16 = kept
    return kept[1]


def bf16_weight_pair(linear):
    """The two bf16 copies of a Linear's weight for the LINEAR_BF16_TRAIN route, made together: ([out_features, in_features],
    [in_features, out_features]), both contiguous - the forward's operand and, transposed, the input gradient's.  One rounding
    (``weight.to(torch.bfloat16)``), so the two hold the same values.  Kept on the module (DERIVED_ATTRIBUTES_BF16, a name of
    its own: ``_weight_bf16`` belongs to the no_grad route) under ``derived_key(weight)`` plus the device and rebuilt when
    that key changes - after every optimizer step; ``drop_derived`` forgets them."""
    w = linear.weight
    key = (derived_key(w), w.device)
    kept = linear.__dict__.get("_weight_bf16_pair")
    if kept is None or kept[0] != key:
        wb = w.detach().to(torch.bfloat16).contiguous()
        kept = (key, wb, wb.t().contiguous())
        linear._weight_bf16_pair = kept
    return kept[1], kept[2]


def linear_bf16_usable(x, *linears):
    """May the FFN whose Linears are ``linears`` run on dfx.ops.linear_bf16 for the input ``x``?  Only as the LINEAR_BF16 comment
    says.  (The switch is read here, at call time, from this module's globals.)"""
    if not (LINEAR_BF16 and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.numel() > 0):
        return False
    return all(l.in_features % 8 == 0 and l.weight.dtype == torch.float32 and l.weight.device == x.device
               and (l.bias is None or (l.bias.dtype == torch.float32 and l.bias.device == x.device)) for l in linears)


def needs_grad(part, *tensors):
    """Does running ``part`` (a module, or an iterable of parameters) on ``tensors`` have anything to differentiate?  True only
    when grad mode is on and one of the tensors or one of the part's parameters requires a gradient.  The front of the detector
    routes on this, not on grad mode alone: a frozen backbone under a training step keeps its fused inference route, and its
    outputs carry no grad_fn (``MSDeformAttn._route`` decides the same way)."""
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    params = part.parameters() if isinstance(part, nn.Module) else part
    return any(p.requires_grad for p in params)


class Linear(nn.Linear):
    """nn.Linear (same parameters, same state_dict keys) whose fp32 forward on the GPU is the hand-written MFMA GEMM with the
    bias in its epilogue (dfx.ops.linear, csrc/gemm_f32.hip).  In grad mode, when the input or a parameter asks for a
    gradient and out_features is a multiple of 4 (up to LINEAR_TRAIN_MAX_OUT_FEATURES) as well, the same forward carries an autograd node whose backward is the
    GEMM again (input gradient) and csrc/gemm_wgrad.hip (weight and bias gradients): dfx.ops.linear_train - or, with
    LINEAR_BF16_TRAIN on, both feature counts multiples of 8 and LINEAR_BF16_TRAIN_MIN_ELEMENTS met, the same three products on bf16 operands:
    dfx.ops.linear_bf16_train.  Anything else is nn.Linear."""

    def forward(self, x):
        # (under autocast, or with parameters in another dtype / on another device, this is plain nn.Linear)
        if (x.is_cuda and x.dtype == torch.float32 and self.in_features % 4 == 0
                and x.numel() > 0 and self.weight.dtype == torch.float32 and self.weight.device == x.device
                and not torch.is_autocast_enabled()):
            if not torch.is_grad_enabled():
                from dfx import ops
                return ops.linear(x.contiguous(), self.weight, self.bias)
            if (LINEAR_TRAIN and self.out_features % 4 == 0 and self.out_features <= LINEAR_TRAIN_MAX_OUT_FEATURES
                    and (x.requires_grad or self.weight.requires_grad or (self.bias is not None and self.bias.requires_grad))):
                from dfx import ops
                if (LINEAR_BF16_TRAIN and self.in_features % 8 == 0 and self.out_features % 8 == 0
                        and x.numel() // self.in_features * (self.in_features + self.out_features) >= LINEAR_BF16_TRAIN_MIN_ELEMENTS
                        and (self.bias is None or (self.bias.dtype == torch.float32 and self.bias.device == x.device))):
                    return ops.linear_bf16_train(x, self.weight, self.bias, *bf16_weight_pair(self))
                return ops.linear_train(x, self.weight, self.bias)
        return super().forward(x)


def post_is_fusable(post):
    """post = (residual, norm[, dropout]): may the add + LayerNorm go through dfx.ops.linear(norm=...)?  Only when the sub-layer's
    Dropout is the identity (eval mode or p = 0) - the reference applies ``norm(residual + dropout(out))``
    (/root/reference/models/deformable_transformer_single.py:635-643) also under no_grad in train mode."""
    if post is None:
        return False
    drop = post[2] if len(post) > 2 else None
    return drop is None or not drop.training or drop.p == 0


def addln_train_usable(norm, dropout, x, residual):
    """May ``norm(residual + dropout(x))`` run on dfx.ops.add_layernorm_train?  Only as the ADDLN_TRAIN comment says; anything
    else keeps the modules.  (The switch and the size rule are read here, at call time, from this module's globals.)"""
    if not (ADDLN_TRAIN and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()):
        return False
    C = x.shape[-1] if x.dim() else 0
    if not (type(norm) is nn.LayerNorm and tuple(norm.normalized_shape) == (C,) and norm.elementwise_affine and norm.bias is not None
            and C % 4 == 0 and 0 < C <= 1024 and x.numel() > 0 and x.numel() // C >= ADDLN_TRAIN_MIN_ROWS
            and norm.weight.dtype == torch.float32 and norm.weight.device == x.device):
        return False
    if residual is not None and not (residual.shape == x.shape and residual.dtype == torch.float32 and residual.device == x.device):
        return False
    if dropout is not None and (type(dropout) is not nn.Dropout or dropout.inplace or has_hooks(dropout)):
        return False
    return not has_hooks(norm) and needs_grad(norm, x, residual)


def apply_post(post, out):
    """norm(residual + dropout(out)) for post = (residual, norm[, dropout]); ``out`` itself when post is None."""
    if post is None:
        return out
    drop = post[2] if len(post) > 2 else None
    if addln_train_usable(post[1], drop, out, post[0]):
        from dfx import ops
        return ops.add_layernorm_train(out, post[0], post[1], drop)
    if drop is not None:
        out = drop(out)
    return post[1](post[0] + out)


def has_hooks(module):
    """True when calling ``module`` would run a forward, forward-pre or backward hook: one registered on the module or a
    global one (torch.nn.modules.module.register_module_*_hook), which runs for every module."""
    from torch.nn.modules import module as _m
    own = (module._forward_hooks, module._forward_pre_hooks, module._backward_hooks, getattr(module, "_backward_pre_hooks", None))
    shared = (getattr(_m, name, None) for name in ("_global_forward_hooks", "_global_forward_pre_hooks", "_global_backward_hooks",
                                                   "_global_backward_pre_hooks"))
    return any(bool(h) for h in own) or any(bool(h) for h in shared)
