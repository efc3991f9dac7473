"""CPU: the reference's parameter groups and optimizer choice (models/optim.py) on the six shipped namespaces, and the argument
checks of the optimizer entries of the C ABI (include/dfx_optim.h) - nothing here launches a kernel."""
import json
import os
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["Baseline.sh", "LateFusion.sh", "Encoder_CrossFusion.sh", "Backbone_CrossFusion.sh", "TransVOD++.sh",
           "TransVOD++_withdepth.sh"]
# what the literal rules of the reference give per shipped configuration: every one of the six puts each trainable parameter
# into exactly one group, so none of them makes torch's constructor raise ("some parameters appear in more than one parameter
# group"); the branch is the one main.py:311-421 / main_multi.py:282-293 takes for the depth_type that build_model sets
BRANCH = {"Baseline.sh": "plain", "LateFusion.sh": "latefusion", "Encoder_CrossFusion.sh": "encoder_cf",
          "Backbone_CrossFusion.sh": "crossfusion", "TransVOD++.sh": "multi", "TransVOD++_withdepth.sh": "multi"}
DEPTH_KEYS = {"latefusion": ["transformer.depth_encoder_layer"], "encoder_cf": ["encoder.fusion_layers"],
              "crossfusion": ["d2r_fusion", "r2d_fusion", "rgb_proj", "d_proj"]}


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "args.json")))


def _built(fixture, script, **override):
    from models import build_model
    ns = dict(fixture["configs"][script]["namespace"])
    ns.update(device="cpu", dformer_weights=None)
    ns.update(override)
    args = SimpleNamespace(**ns)
    model, _, _ = build_model(args)               # sets args.depth_type from --fusion_type, as the reference's build() does
    return args, model, fixture["configs"][script]["script"]


def _frozen_by_the_branch(branch, name):
    if branch == "latefusion":
        return "backbone.0.body" in name and "depth" not in name
    if branch == "encoder_cf":
        return "backbone.0.body" in name
    return False


def _multiplier(branch, args, name):
    """the lr multiplier of the cited reference lines, decided per NAME (the reference decides per group)"""
    proj = any(k in name for k in args.lr_linear_proj_names)
    if branch == "multi":                                     # main_multi.py:282-293
        return args.lr_linear_proj_mult if proj else 1.0
    if branch == "plain":                                     # main.py:404-421
        backbone = any(k in name for k in args.lr_backbone_names)
        assert not (backbone and proj), name
        return 0.1 if backbone else args.lr_linear_proj_mult if proj else 1.0
    depth = any(k in name for k in DEPTH_KEYS[branch])       # main.py:317-341, 348-372, 379-403
    if depth:
        return 1.0 if proj else 10.0
    return args.lr_linear_proj_mult if proj else 1.0


@pytest.mark.parametrize("script", SCRIPTS)
def test_groups_hold_every_trainable_parameter_once_with_the_reference_multipliers(fixture, script):
    from models.optim import build_param_groups
    args, model, main = _built(fixture, script)
    branch = BRANCH[script]
    assert (main == "main_multi.py") == (branch == "multi")
    if branch in DEPTH_KEYS:
        assert branch in args.depth_type
    groups = build_param_groups(args, model, main)
    assert len(groups) == {"multi": 2, "plain": 3}.get(branch, 5)
    names = {id(p): n for n, p in model.named_parameters()}
    seen = Counter(id(p) for g in groups for p in g["params"])
    assert set(seen.values()) == {1}
    assert set(seen) == {id(p) for p in model.parameters() if p.requires_grad}
    for n, p in model.named_parameters():
        assert p.requires_grad == (not _frozen_by_the_branch(branch, n)), n
    assert any(not p.requires_grad for p in model.parameters()) == (branch in ("latefusion", "encoder_cf"))
    used = set()
    for g in groups:
        for p in g["params"]:
            m = _multiplier(branch, args, names[id(p)])
            assert g["lr"] == args.lr * m, (names[id(p)], g["lr"], m)
            used.add(m)
    assert used == {"multi": {1.0, 0.1}, "plain": {1.0, 0.1}}.get(branch, {1.0, 0.1, 10.0})
    torch.optim.AdamW(groups, lr=args.lr, weight_decay=args.weight_decay)          # and torch's constructor takes them


def test_latefusion_depth_type_freezes_the_rgb_body(fixture):
    from models.optim import build_param_groups
    args, model, main = _built(fixture, "LateFusion.sh")
    for p in model.parameters():
        p.requires_grad = True
    build_param_groups(args, model, main)
    body = [(n, p) for n, p in model.named_parameters() if "backbone.0.body" in n]
    assert len(body) > 50
    for n, p in body:
        assert p.requires_grad == ("depth" in n), n
    assert all(p.requires_grad for n, p in model.named_parameters() if "backbone.0.body" not in n)


def test_a_parameter_no_rule_names_is_reported(fixture):
    from models.optim import build_param_groups
    args, model, main = _built(fixture, "Backbone_CrossFusion.sh")
    model.extra_scale = torch.nn.Parameter(torch.ones(3))          # no keyword of the crossfusion rules matches
    with pytest.raises(ValueError, match="not included in param_dicts"):
        build_param_groups(args, model, main)
    with pytest.raises(ValueError, match="script"):
        build_param_groups(args, model, "train.py")


def test_build_optimizer_on_cpu_is_torch_adamw_over_the_groups(fixture, monkeypatch):
    from models.optim import build_optimizer, build_param_groups
    monkeypatch.delenv("DFX_OPTIM", raising=False)
    args, model, main = _built(fixture, "LateFusion.sh")
    opt = build_optimizer(args, model, main)
    assert type(opt) is torch.optim.AdamW
    groups = build_param_groups(args, model, main)
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in groups]
    assert [[id(p) for p in g["params"]] for g in opt.param_groups] == [[id(p) for p in g["params"]] for g in groups]
    assert all(g["weight_decay"] == args.weight_decay and g["betas"] == (0.9, 0.999) for g in opt.param_groups)
    monkeypatch.setenv("DFX_OPTIM", "1")                           # forced: the fused class refuses CPU parameters, no fall-back
    with pytest.raises(ValueError, match="CPU"):
        build_optimizer(args, model, main)
    monkeypatch.setenv("DFX_OPTIM", "0")
    assert type(build_optimizer(args, model, main)) is torch.optim.AdamW


def test_build_optimizer_with_sgd(fixture):
    from models.optim import build_optimizer
    args, model, main = _built(fixture, "TransVOD++.sh", sgd=True)
    opt = build_optimizer(args, model, main)
    assert type(opt) is torch.optim.SGD
    assert all(g["momentum"] == 0.9 and g["weight_decay"] == args.weight_decay for g in opt.param_groups)
    assert [g["lr"] for g in opt.param_groups] == [args.lr, args.lr * args.lr_linear_proj_mult]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
OPTIM_SYMBOLS = ("dfx_optim_chunk_elements", "dfx_grad_sqnorm_f32", "dfx_adamw_step_f32")
ONE, ODD = 16, 20      # non-null addresses, 8-byte aligned and not: every call below fails (or is empty) before they would be used


def test_optimizer_symbols_are_declared_exported_and_bound():
    import re
    from dfx import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx_optim.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dfx_[a-z0-9_]+)\s*\(", text))) == sorted(OPTIM_SYMBOLS)
    lib = _lib.load()
    for name in OPTIM_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.abi_version() == 5
    chunk = lib.dfx_optim_chunk_elements()
    assert chunk > 0 and chunk % 4 == 0


def _refused(lib, name, args, cause):
    rc = getattr(lib, name)(*args, None)
    assert rc != 0 and cause in lib.dfx_last_error(), (name, args, rc, lib.dfx_last_error())


def test_optimizer_entries_refuse_bad_arguments_before_any_launch():
    from dfx import _lib
    lib = _lib.load()
    # tensors, chunks, n_chunks, partials
    _refused(lib, "dfx_grad_sqnorm_f32", (0, ONE, 3, ONE), b"null pointer")
    _refused(lib, "dfx_grad_sqnorm_f32", (ONE, 0, 3, ONE), b"null pointer")
    _refused(lib, "dfx_grad_sqnorm_f32", (ONE, ONE, 3, 0), b"null pointer")
    _refused(lib, "dfx_grad_sqnorm_f32", (ONE, ONE, -1, ONE), b"bad dimension")
    _refused(lib, "dfx_grad_sqnorm_f32", (ONE, ONE, 3, ODD), b"8-byte aligned")
    # tensors, chunks, n_chunks, partials | NULL, max_norm, norm_out | NULL
    _refused(lib, "dfx_adamw_step_f32", (0, ONE, 3, 0, 0.0, 0), b"null pointer")
    _refused(lib, "dfx_adamw_step_f32", (ONE, 0, 3, 0, 0.0, 0), b"null pointer")
    _refused(lib, "dfx_adamw_step_f32", (ONE, ONE, -2, 0, 0.0, 0), b"bad dimension")
    _refused(lib, "dfx_adamw_step_f32", (ONE, ONE, 3, ODD, 1.0, 0), b"8-byte aligned")
    _refused(lib, "dfx_adamw_step_f32", (ONE, ONE, 3, ONE, 0.0, 0), b"max_norm must be positive")
    _refused(lib, "dfx_adamw_step_f32", (ONE, ONE, 3, ONE, float("nan"), 0), b"max_norm must be positive")
    _refused(lib, "dfx_adamw_step_f32", (ONE, ONE, 3, ONE, 1.0, 18), b"4-byte aligned")


def test_optimizer_entries_take_an_empty_table_before_the_pointers():
    from dfx import _lib
    lib = _lib.load()
    assert lib.dfx_grad_sqnorm_f32(0, 0, 0, 0, None) == 0
    assert lib.dfx_adamw_step_f32(0, 0, 0, 0, 0.0, 0, None) == 0
    assert lib.dfx_adamw_step_f32(0, 0, 0, ODD, -1.0, 0, None) == 0


def test_chunk_table_layout():
    """one record per chunk, tensor after tensor, none for an empty tensor; the records are the header's structs"""
    from dfx import optim
    chunk = optim.chunk_elements()
    table = optim._chunk_table([5, 0, chunk, 2 * chunk + 7, 1])
    assert table["tensor"].tolist() == [0, 2, 3, 3, 3, 4]
    assert table["first"].tolist() == [0, 0, 0, chunk, 2 * chunk, 0]
    assert optim._TENSOR.itemsize == 72 and optim._CHUNK.itemsize == 16
    assert optim._TENSOR.fields["numel"][1] == 32 and optim._TENSOR.fields["scalars"][1] == 40
    assert len(optim._chunk_table([0, 0])) == 0 and len(optim._chunk_table([])) == 0
