"""GPU: the front of the detector routes on whether anything needs a gradient (models.fused.needs_grad), not on grad mode alone -
a frozen ResNet-50 body, a frozen prefix of it, a frozen input projection and a frozen depth backbone keep their fused
inference routes while autograd records, and whatever trains runs as before."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

CONVS = {"stem": 1, "layer1": 10, "layer2": 13, "layer3": 19, "layer4": 10}      # nn.Conv2d modules of ResNet-50 per part


def _backbone(frozen=("stem", "layer1", "layer2", "layer3", "layer4"), fused=True):
    """ResNet50(FrozenBatchNorm2d, dilated) inside FusionBackbone with the named parts frozen"""
    from models.backbone_scratch import FusionBackbone
    from tests._param_fill import fill_params_by_name
    bb = FusionBackbone("resnet50", "resnet18", True, None, True, True, "Baseline_rgb", [3], 256, False)
    fill_params_by_name(bb, seed=3)
    body = bb.body
    for name in frozen:
        for p in (body.conv1.parameters() if name == "stem" else getattr(body, name).parameters()):
            p.requires_grad_(False)
    for p in body.fc.parameters():              # (the unused classifier)
        p.requires_grad_(False)
    bb.fused_inference = fused
    return bb.cuda().eval()


def _frames(requires_grad=False):
    from util.misc import NestedTensor
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_(requires_grad)
    return NestedTensor(x, torch.zeros(2, 64, 96, dtype=torch.bool, device="cuda"))


@pytest.fixture
def conv_calls(monkeypatch):
    calls, real = [], nn.Conv2d.forward

    def spy(mod, x):
        calls.append(mod)
        return real(mod, x)

    monkeypatch.setattr(nn.Conv2d, "forward", spy)
    return calls


def _tensors(out):
    return {k: v.tensors for k, v in out[0].items()}


def test_frozen_body_keeps_the_fused_route_in_grad_mode(conv_calls):
    bb, nt = _backbone(), _frames()
    with torch.no_grad():
        quiet = _tensors(bb(nt))
    assert not conv_calls and len(quiet) == 3
    assert torch.is_grad_enabled()
    got = _tensors(bb(nt))
    assert not conv_calls, f"{len(conv_calls)} convolutions of a frozen body ran op by op in grad mode"
    for k in quiet:
        assert torch.equal(got[k], quiet[k]), k
        assert not got[k].requires_grad and got[k].grad_fn is None, k


def test_trainable_body_runs_every_convolution_through_its_module(conv_calls):
    bb, nt = _backbone(frozen=()), _frames()
    got = _tensors(bb(nt))
    assert len(conv_calls) == sum(CONVS.values())
    assert all(t.grad_fn is not None for t in got.values())
    assert bb.body.__dict__.get("_chain_carry") is None


def test_frozen_prefix_runs_fused_and_the_rest_trains(conv_calls):
    """Stem and layer1 frozen (DETR's default freeze): they run fused without computing layer2[0].conv1 for the trainable stage
    behind them; layer2-4 run op by op and their gradients agree with the all-op-by-op route."""
    parts = ("stem", "layer1")
    bb, plain, nt = _backbone(parts), _backbone(parts, fused=False), _frames()
    weights = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(7)).cuda() for k, v in _tensors(plain(nt)).items()}
    want_calls = len(conv_calls)
    assert want_calls == sum(CONVS.values())
    want = _tensors(plain(nt))
    gw = torch.autograd.grad(sum((want[k] * weights[k]).sum() for k in want), plain.body.layer2[0].conv1.weight)[0]
    del conv_calls[:]
    got = _tensors(bb(nt))
    trained = {id(m) for name in ("layer2", "layer3", "layer4") for m in getattr(bb.body, name).modules() if isinstance(m, nn.Conv2d)}
    assert len(conv_calls) == CONVS["layer2"] + CONVS["layer3"] + CONVS["layer4"] and {id(m) for m in conv_calls} == trained
    assert bb.body.__dict__.get("_chain_carry") is None, "a conv1 computed from detached weights waits for a stage that trains"
    gg = torch.autograd.grad(sum((got[k] * weights[k]).sum() for k in got), bb.body.layer2[0].conv1.weight)[0]
    for name, a, b in [(k, got[k], want[k]) for k in want] + [("grad layer2[0].conv1.weight", gg, gw)]:
        scale = b.abs().max().item()
        assert (a.detach() - b.detach()).abs().max().item() < 1e-4 * max(scale, 1.0), name      # (test_fused_backbone_matches_reference_formulation)
    assert gw.abs().max().item() > 0


def test_an_input_that_requires_grad_runs_a_frozen_body_op_by_op(conv_calls):
    bb, nt = _backbone(), _frames(requires_grad=True)
    got = _tensors(bb(nt))
    assert len(conv_calls) == sum(CONVS.values())
    assert all(t.grad_fn is not None for t in got.values())


def test_frozen_projection_takes_the_inference_route_until_its_norm_trains(monkeypatch):
    from dfx import ops
    from models.detector_common import _conv_gn
    torch.manual_seed(4)
    proj = _conv_gn(128, 256).cuda()
    for p in proj.parameters():
        p.requires_grad_(False)
    calls = []
    for name in ("conv1x1", "conv1x1_train", "group_norm"):
        def spy(*a, _real=getattr(ops, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    monkeypatch.setattr(nn.GroupNorm, "forward", lambda *a: pytest.fail("nn.GroupNorm.forward on a fused route"))
    monkeypatch.setattr(nn.Conv2d, "forward", lambda *a: pytest.fail("nn.Conv2d.forward on a fused route"))
    x = torch.randn(2, 128, 13, 20, device="cuda", requires_grad=True)
    with torch.no_grad():
        quiet = proj(x)
    del calls[:]
    frozen = proj((x * 2).detach() / 2)                  # grad mode, nothing to differentiate
    assert calls == ["conv1x1", "group_norm"] and frozen.grad_fn is None and not frozen.requires_grad
    assert torch.equal(frozen, quiet)
    proj[1].weight.requires_grad_(True)
    from models import fused
    monkeypatch.setattr(fused, "CONVGN_TRAIN_MIN_PIXELS", 0)      # (a 13 x 20 map: the size rule is a speed matter)
    del calls[:]
    y = proj(x.detach())
    assert calls[0] == "conv1x1_train" and calls[-1] == "group_norm" and y.requires_grad and torch.equal(y.detach(), quiet)
    (g,) = torch.autograd.grad(y.sum(), proj[1].weight)
    assert g.shape == (256,) and torch.isfinite(g).all()


def test_frozen_depth_backbone_takes_the_folded_route_in_grad_mode(monkeypatch):
    from models.dformer_backbone import DFormerBackbone
    from tests._param_fill import fill_params_by_name
    from util.misc import NestedTensor
    bb = fill_params_by_name(DFormerBackbone(train_backbone=False, freeze_batchnorm=True), seed=2).cuda().eval()
    assert not any(p.requires_grad for p in bb.depth_backbone.downsample_layers_e[:-1].parameters())
    folded, real = [], DFormerBackbone._forward_folded

    def spy(self, stages, x):
        folded.append(1)
        return real(self, stages, x)

    monkeypatch.setattr(DFormerBackbone, "_forward_folded", spy)
    d = torch.rand(2, 1, 64, 96, generator=torch.Generator().manual_seed(5)).cuda()
    nt = NestedTensor(d, torch.zeros(2, 64, 96, dtype=torch.bool, device="cuda"))
    with torch.no_grad():
        quiet = bb(nt)["0"].tensors
    assert len(folded) == 1 and torch.is_grad_enabled()
    got = bb(nt)["0"].tensors
    assert len(folded) == 2 and got.grad_fn is None and torch.equal(got, quiet)
    bb.depth_backbone.downsample_layers_e[1][0].train()      # a BatchNorm in training mode: batch statistics, the module route
    live = bb(nt)["0"].tensors
    assert len(folded) == 2 and live.shape == got.shape
    bb.eval()
    next(bb.depth_backbone.downsample_layers_e[0].parameters()).requires_grad_(True)      # something trains: the module route
    assert bb(nt)["0"].tensors.grad_fn is not None and len(folded) == 2
