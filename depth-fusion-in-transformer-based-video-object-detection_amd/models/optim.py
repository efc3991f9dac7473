"""The reference's optimizer construction: name-keyed parameter groups and the optimizer over them.

``build_param_groups`` restates ref main.py:308-421 (four ``depth_type`` branches, each with its ``requires_grad`` side
effects) and main_multi.py:282-293 (two groups) with the reference's own keyword tests, and makes the reference's check that
every trainable parameter landed in a group (main.py:515-520).  It reads the reference's namespace fields ``lr``,
``lr_linear_proj_names``, ``lr_linear_proj_mult``, ``lr_backbone_names``, ``depth_type`` (``build_optimizer`` also
``weight_decay`` and ``sgd``).  The rules are kept literally: where they put one parameter into two groups, the
optimizer's constructor raises as it does under the reference.

``build_optimizer`` is main.py:423-428 / main_multi.py:295-302: SGD with momentum 0.9 under ``args.sgd``, else AdamW - the
fused ``dfx.optim.AdamW`` (HIP kernels over all parameters, csrc/optim.hip) or ``torch.optim.AdamW``, see ``use_fused``.
"""
import os

import torch

# Does dfx.optim.AdamW.step(max_norm) beat the faster torch route (clip_grad_norm_ + AdamW, foreach or fused=True) in wall
# time on BOTH measured parameter sets by more than the observed min-max spread?  Measured (tools/bench_optim_step.py,
# profiles/r20_optim_step.txt; median (min .. max) ms of 30 steps, the faster torch route is foreach on both):
#   single-frame Late Fusion, 328 tensors, 1.2e7 elements   1.143 (1.112 .. 1.230)  against  2.593 (2.564 .. 2.782)   2.27x
#   TransVOD++ with depth, 607 tensors, 8.1e7 elements      2.565 (2.377 .. 3.690)  against  4.930 (4.760 .. 6.674)   1.92x
# Its slowest step is faster than torch's fastest on both, so it is the default for fp32 parameters on a GPU.
FUSED_WINS = True


def match_name_keywords(n, name_keywords):
    """ref main.py:275-286, main_multi.py:249-260"""
    return any(b in n for b in name_keywords)


def is_depthencoder(param_name, include_keywords=("transformer.depth_encoder_layer",)):
    """ref main.py:292-305 (its exclude_keywords argument is never used)"""
    return any(keyword in param_name for keyword in include_keywords)


def _five_groups(args, named, first_rule, backbone_keywords, depth_keywords):
    """the group list the three depth branches of main.py share: other layers, the (depth) backbone, the linear projections at
    lr * lr_linear_proj_mult, the depth encoder at lr * 10, and the depth encoder's linear projections at lr"""
    proj = args.lr_linear_proj_names

    def de(n):
        return is_depthencoder(n) if depth_keywords is None else is_depthencoder(n, depth_keywords)

    return [
        {"params": [p for n, p in named if first_rule(n) and not match_name_keywords(n, proj) and p.requires_grad and not de(n)],
         "lr": args.lr},
        {"params": [p for n, p in named if match_name_keywords(n, backbone_keywords) and p.requires_grad and not de(n)],
         "lr": args.lr},
        {"params": [p for n, p in named if match_name_keywords(n, proj) and p.requires_grad and not de(n)],
         "lr": args.lr * args.lr_linear_proj_mult},
        {"params": [p for n, p in named if p.requires_grad and de(n) and not match_name_keywords(n, proj)],
         "lr": args.lr * 10},
        {"params": [p for n, p in named if p.requires_grad and de(n) and match_name_keywords(n, proj)],
         "lr": args.lr},
    ]


def build_param_groups(args, model, script="main.py"):
    """-> the ``param_dicts`` of the reference's ``script`` for ``model`` (without any DDP wrapper).  As in the reference, the
    three depth branches of main.py SET ``requires_grad`` on every parameter first.  Raises ValueError when the groups,
    free of duplicates, do not hold exactly the trainable parameters' element count (main.py:515-520)."""
    if script not in ("main.py", "main_multi.py"):
        raise ValueError(f"build_param_groups: script is 'main.py' or 'main_multi.py', not {script!r}")
    named = list(model.named_parameters())
    proj = args.lr_linear_proj_names
    if script == "main_multi.py":                                            # main_multi.py:282-293
        groups = [
            {"params": [p for n, p in named if p.requires_grad and not match_name_keywords(n, proj)], "lr": args.lr},
            {"params": [p for n, p in named if p.requires_grad and match_name_keywords(n, proj)],
             "lr": args.lr * args.lr_linear_proj_mult},
        ]
    elif "latefusion" in args.depth_type:                                    # main.py:311-341
        for n, p in named:
            p.requires_grad = not ("backbone.0.body" in n and "depth" not in n)
        groups = _five_groups(args, named, lambda n: not match_name_keywords(n, ["backbone"]), ["depth_backbone"], None)
    elif "crossfusion" in args.depth_type:                                   # main.py:342-372
        for n, p in named:
            p.requires_grad = True
        groups = _five_groups(args, named, lambda n: match_name_keywords(n, ["transformer", "class_embed", "query_embed", "input_proj"]),
                              ["backbone"], ["d2r_fusion", "r2d_fusion", "rgb_proj", "d_proj"])
    elif "encoder_cf" in args.depth_type:                                    # main.py:373-403
        for n, p in named:
            p.requires_grad = "backbone.0.body" not in n
        groups = _five_groups(args, named, lambda n: not match_name_keywords(n, ["backbone"]), ["depth_backbone"],
                              ["encoder.fusion_layers"])
    else:                                                                    # main.py:404-421
        bb = args.lr_backbone_names
        groups = [
            {"params": [p for n, p in named if not match_name_keywords(n, bb) and not match_name_keywords(n, proj) and p.requires_grad],
             "lr": args.lr},
            {"params": [p for n, p in named if match_name_keywords(n, bb) and p.requires_grad], "lr": args.lr * 0.1},
            {"params": [p for n, p in named if match_name_keywords(n, proj) and p.requires_grad],
             "lr": args.lr * args.lr_linear_proj_mult},
        ]
    in_model = sum(p.numel() for p in model.parameters() if p.requires_grad)
    in_groups = sum(p.numel() for g in groups for p in g["params"])
    ids = [id(p) for g in groups for p in g["params"]]
    # a parameter in two groups is the optimizer constructor's to refuse: the reference builds the optimizer first
    # (main.py:423-428) and never reaches its own check then
    if len(set(ids)) == len(ids) and in_model != in_groups:
        raise ValueError("Some parameters are not included in param_dicts.")
    return groups


def use_fused(groups):
    """Does ``build_optimizer`` take ``dfx.optim.AdamW``?  ``DFX_OPTIM=0``: never.  ``DFX_OPTIM=1``: always (it raises on
    parameters it cannot take).  Otherwise: when every parameter is fp32 on a GPU and the measurement says it wins."""
    env = os.environ.get("DFX_OPTIM")
    if env == "0":
        return False
    if env == "1":
        return True
    params = [p for g in groups for p in g["params"]]
    return FUSED_WINS and len(params) > 0 and all(p.is_cuda and p.dtype == torch.float32 for p in params)


def build_optimizer(args, model, script="main.py"):
    """The optimizer of the reference's ``script`` over ``build_param_groups(args, model, script)``."""
    groups = build_param_groups(args, model, script)
    if args.sgd:
        return torch.optim.SGD(groups, lr=args.lr, momentum=0.9, weight_decay=args.weight_decay)
    if use_fused(groups):
        from dfx.optim import AdamW
        return AdamW(groups, lr=args.lr, weight_decay=args.weight_decay)
    return torch.optim.AdamW(groups, lr=args.lr, weight_decay=args.weight_decay)
