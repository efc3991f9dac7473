"""CPU: the one statement of "have the weights changed" (models.fused.derived_key), what it sees and what it cannot see,
models.fused.drop_derived, and the tensors ClipRunner's key covers."""
import pytest
import torch
from torch import nn

from tests import _lifecycle as L


def _linear_bn():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(4, 3), nn.BatchNorm1d(3)).eval()


@pytest.mark.parametrize("name", ["weight", "bias"])
@pytest.mark.parametrize("kind", ["inplace", "optimizer", "load", "assign", "replace"])
def test_derived_key_moves_with_every_visible_edit_of_a_parameter(kind, name):
    from models.fused import derived_key
    m = _linear_bn()
    lin = m[0]
    key = derived_key(lin)
    assert key == derived_key(lin) and len(key) == 2
    other = "bias" if name == "weight" else "weight"
    untouched = derived_key(getattr(lin, other))
    L.EDITS[kind](lin, name)
    assert derived_key(lin) != key
    assert derived_key(getattr(lin, name)) != key[:1] and derived_key(getattr(lin, name)) != key[1:]
    assert derived_key(getattr(lin, other)) == untouched, "the edit kinds change one tensor"
    assert derived_key(lin) == derived_key(lin)


@pytest.mark.parametrize("kind", ["inplace", "replace", "load", "assign"])
def test_derived_key_moves_with_an_edit_of_a_buffer(kind):
    from models.fused import derived_key
    bn = _linear_bn()[1]
    key = derived_key(bn)
    assert len(key) == 5 and key == derived_key(bn)          # weight, bias, running_mean, running_var, num_batches_tracked
    L.EDITS[kind](bn, "running_var")
    now = derived_key(bn)
    # (nn.BatchNorm's own load hook re-creates a missing num_batches_tracked entry and copies it in as well: the counter's key
    # may move under ``load``; the four floating tensors are what the edit kinds are about)
    assert now != key and [a == b for a, b in zip(now[:4], key[:4])] == [True, True, True, False]


def test_replace_keeps_the_version_counter_so_the_pointer_is_what_moves():
    from models.fused import derived_key
    lin = _linear_bn()[0]
    (ptr, version), = derived_key(lin.bias)
    L.replace(lin, "bias")
    (ptr2, version2), = derived_key(lin.bias)
    assert version2 == version and ptr2 != ptr


def test_derived_key_cannot_see_in_place_writes_through_data():
    """Recorded, not wished for: torch does not bump ``_version`` for writes through ``.data`` (the EMA / weight-clipping
    spelling ``p.data.mul_(d)``), and the storage stays where it is.  No key built on (pointer, version) notices; the
    documented answer is drop_derived / ClipRunner.refresh."""
    from models.fused import derived_key
    lin = _linear_bn()[0]
    key, before = derived_key(lin), lin.weight.detach().clone()
    L.data_inplace(lin, "weight")
    assert not torch.equal(lin.weight, before)
    assert derived_key(lin) == key


def test_derived_key_of_modules_tensors_and_none():
    from models.fused import derived_key
    conv = nn.Conv2d(2, 2, 1, bias=False)
    bn = nn.BatchNorm2d(2)
    key = derived_key(conv, bn, None, bn.weight)
    assert key[0] == (conv.weight.data_ptr(), conv.weight._version) and key[1] is None          # the missing bias keeps its place
    assert len(key) == 2 + 5 + 1 + 1 and key[7] is None and key[8] == key[2]
    assert derived_key() == ()


def test_drop_derived_removes_exactly_the_derived_attributes():
    from models import fused
    from models.ops.modules import MSDeformAttn
    from models.resnet import Bottleneck
    from models.backbone_scratch import FrozenBatchNorm2d
    from util import memo
    block = Bottleneck(8, 4, 1, 1, None, FrozenBatchNorm2d)
    attn = MSDeformAttn(64, 1, 2, 4)
    root = nn.ModuleDict({"block": block, "attn": attn, "mha": nn.MultiheadAttention(8, 2)})
    memo.clear()                                      # (the memo is the process's: earlier tests may have left entries)
    assert fused.drop_derived(root) == 0 and not memo._MEMO
    keys, params, buffers = list(root.state_dict()), dict(root.named_parameters()), dict(root.named_buffers())
    state = {k: v.clone() for k, v in root.state_dict().items()}
    planted = 0
    for mod, names in ((block, ("_folded", "_plans1x1", "_chain_carry", "_stem_folded", "_plan")),
                       (attn, ("_qproj_cache", "_qproj_head", "_qproj_head_key", "_value_stack")),
                       (root["mha"], ("_kv_stack",))):
        for name in names:
            setattr(mod, name, ("key", torch.ones(1)))
            planted += 1
    assert planted == len(fused.DERIVED_ATTRIBUTES) and {n for m in root.modules() for n in m.__dict__ if n in fused.DERIVED_ATTRIBUTES} \
        == set(fused.DERIVED_ATTRIBUTES)
    block.not_derived = ("stays", torch.ones(1))
    t = torch.zeros(2)
    with torch.no_grad():
        assert memo.memo_on(t, "tag", lambda: 5) == 5
    assert len(memo._MEMO) == 1
    assert fused.drop_derived(root) == planted + 1
    assert not memo._MEMO
    assert not any(n in m.__dict__ for m in root.modules() for n in fused.DERIVED_ATTRIBUTES)
    assert block.not_derived[0] == "stays"
    assert list(root.state_dict()) == keys
    assert all(root.get_parameter(k) is v for k, v in params.items()) and all(root.get_buffer(k) is v for k, v in buffers.items())
    assert all(torch.equal(v, state[k]) for k, v in root.state_dict().items())
    assert fused.drop_derived(root) == 0


def test_dropped_modules_are_usable_like_new_ones(cpu_msda):
    """A never-run module has none of the attributes; a dropped one must not be told apart from it (no AttributeError from a
    site that expects its own None)."""
    from models import fused
    from models.ops.modules import MSDeformAttn
    from models.resnet import Bottleneck
    from models.backbone_scratch import FrozenBatchNorm2d
    block, attn = Bottleneck(8, 4, 1, 1, None, FrozenBatchNorm2d), MSDeformAttn(64, 1, 2, 4)
    for mod in (block, attn):
        assert not any(n in mod.__dict__ for n in fused.DERIVED_ATTRIBUTES)
    w, b = attn._qproj_params()
    wh, bh = attn._qproj_params_by_head()
    assert fused.drop_derived(attn) == 3
    w2, b2 = attn._qproj_params()
    wh2, bh2 = attn._qproj_params_by_head()
    assert w2 is not w and torch.equal(w2, w) and torch.equal(b2, b) and torch.equal(wh2, wh) and torch.equal(bh2, bh)
    L.replace(attn.sampling_offsets, "bias")
    assert not torch.equal(attn._qproj_params()[1], b) and not torch.equal(attn._qproj_params_by_head()[1], bh)


def test_clip_runner_key_visits_every_tensor_of_the_detector_once():
    from models import build_model
    from models.clip_inference import ClipRunner
    from models.config import transvodpp_args
    model, _, _ = build_model(transvodpp_args(num_ref_frames=3, device="cpu"))       # tests/test_clip_shard_gpu.py::_build, on the CPU
    model.register_buffer("not_persistent", torch.zeros(3), persistent=False)
    runner = ClipRunner(model.eval(), micro_batch=4, fused=False)
    key = runner.weights_key()
    slots = [table[name] for table, name in runner._key_sources]
    visited = [t for t in slots if t is not None]                 # (a missing bias keeps its place in the key, as None)
    assert len(key) == len(slots) and [k is None for k in key] == [t is None for t in slots]
    assert len({id(t) for t in visited}) == len(visited), "a tensor is visited twice"
    want = {id(t) for t in model.state_dict(keep_vars=True).values()} | {id(model.not_persistent)}
    assert {id(t) for t in visited} == want
    assert "not_persistent" not in model.state_dict()
    assert key == runner.weights_key()
    # a rebinding is seen although the walk over the modules is not repeated
    L.assign(model.transformer, "level_embed")
    L.replace(model.class_embed[0], "bias")
    now = runner.weights_key()
    assert len(now) == len(key) and sum(a != b for a, b in zip(now, key)) == 2
