"""GPU: which routes of models.dformer_backbone.DFormerBackbone take dfx.ops.batch_norm_train (models.fused.DFORMER_TRAIN), what
the stem computes on them against the reference's own training pass (tests/golden/dformer_train*.npz,
tools/gen_golden_dformer_train.py) and against the modules, and the routes that stay as they were.  The size rule is set to 0
pixels here: the stem runs on 2 depth maps of 64 x 96."""
import os

import pytest
import torch
from torch import nn

from tests import _dformer_train_cases as dc
from tests import _golden
from tests._param_fill import fill_params_by_name

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def routed(monkeypatch):
    """size rule 0, switch on, and a list that receives (channels, act) per call of the new entry"""
    from dfx import ops
    from models import fused
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS", 0)
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS_GELU", 0)
    monkeypatch.setattr(fused, "DFORMER_TRAIN", True)
    calls, real = [], ops.batch_norm_train

    def spy(x, bn, act=None):
        calls.append((x.shape[1], act))
        return real(x, bn, act)

    monkeypatch.setattr(ops, "batch_norm_train", spy)
    return calls


STEM_CALLS = [(16, "gelu"), (32, None), (32, None), (64, None)]


def _stem(**kw):
    from models.dformer_backbone import DFormerBackbone
    torch.manual_seed(0)
    net = DFormerBackbone(train_backbone=True, freeze_batchnorm=False, **kw)
    fill_params_by_name(net, seed=dc.STEM_SEED)
    return net.cuda().train()


def _input(requires_grad=False):
    from util.misc import NestedTensor
    depth, g = dc.stem_inputs()
    depth = depth.float().cuda().requires_grad_(requires_grad)
    return NestedTensor(depth, torch.zeros(depth.shape[0], depth.shape[2], depth.shape[3], dtype=torch.bool, device="cuda")), g.float().cuda()


def _gpu_pass():
    from models.dformer_backbone import DFormerBackbone
    from util.misc import NestedTensor
    return dc.run_stem(DFormerBackbone, NestedTensor, fill_params_by_name, torch.float32, device="cuda")


def test_stem_on_the_kernels_meets_the_references_training_pass(routed):
    """Every stored name within YARDSTICK_FACTOR x the error of the reference's own fp32 pass, both against its fp64 pass.
    For the gradients that are mathematically zero (tests/_dformer_train_cases.STEM_ZERO_GRADS) both errors are divided by the
    same (rounding-noise) magnitude: the rule compares the absolute errors."""
    gold = _golden.load(os.path.join(ROOT, "tests", "golden"), "dformer_train")
    ref = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("ref.")}
    f32 = {k[4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("f32.")}
    _, got = _gpu_pass()
    assert routed == STEM_CALLS, routed
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = []
    for n in sorted(ref):
        if not ref[n].is_floating_point():
            assert torch.equal(got[n], ref[n]), n
            continue
        y, err = dc.rel_err(f32[n], ref[n]), dc.rel_err(got[n], ref[n])
        print(f"  stem {n}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}, "
              f"max |ref| {ref[n].abs().max().item():.3e}")
        if not err <= dc.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {dc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, "; ".join(worst)


def test_switch_on_against_switch_off(routed, monkeypatch):
    from models import fused
    gold = _golden.load(os.path.join(ROOT, "tests", "golden"), "dformer_train")
    net_on, on = _gpu_pass()
    assert routed == STEM_CALLS
    del routed[:]
    monkeypatch.setattr(fused, "DFORMER_TRAIN", False)
    net_off, off = _gpu_pass()
    assert not routed, "DFX_DFORMER_TRAIN=0 keeps the modules"
    assert list(net_on.state_dict()) == list(net_off.state_dict()) and set(on) == set(off)
    assert not any("_folded" in k or "stats" in k for k in net_on.state_dict())
    for n in on:
        if not on[n].is_floating_point():
            assert torch.equal(on[n], off[n]), n              # num_batches_tracked moves alike
            continue
        # two fp32 evaluations of one function: each within the rule of the fp64 reference, so of each other within twice it
        ref, f32 = torch.from_numpy(gold["ref." + n]), torch.from_numpy(gold["f32." + n])
        top = ref.abs().max().item() or 1.0
        allowed = 2 * dc.YARDSTICK_FACTOR * dc.rel_err(f32, ref) * top
        assert (on[n].double() - off[n].double()).abs().max().item() <= allowed, n
    assert int(net_on.depth_backbone.downsample_layers_e[0][1].num_batches_tracked) == 1


def test_routes_that_keep_the_modules(routed, monkeypatch):
    from models import fused
    nt, g = _input()
    net = _stem()
    # autocast
    with torch.autocast("cuda", dtype=torch.bfloat16):
        net(nt)
    assert not routed
    # a forward hook on one BatchNorm: that layer alone keeps its module
    bn16 = net.depth_backbone.downsample_layers_e[0][1]
    seen = []
    h = bn16.register_forward_hook(lambda m, i, o: seen.append(1))
    net(nt)
    assert seen == [1] and routed == STEM_CALLS[1:], routed
    h.remove()
    del routed[:]
    # a hook on a stage: the whole stage is called as it is
    h = net.depth_backbone.downsample_layers_e[1].register_forward_hook(lambda m, i, o: seen.append(2))
    net(nt)
    assert seen == [1, 2] and routed == [STEM_CALLS[0], STEM_CALLS[1], STEM_CALLS[3]], routed
    h.remove()
    del routed[:]
    # below the size rule: per layer, on the BatchNorm's own input (2 x 32 x 48 after the first convolution, 2 x 16 x 24 ...)
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS", 2 * 32 * 48)
    net(nt)
    assert routed == STEM_CALLS[:1], routed
    # ... the BatchNorm + GELU call has a rule of its own
    del routed[:]
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS_GELU", 2 * 32 * 48 + 1)
    net(nt)
    assert not routed
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS_GELU", 2 * 32 * 48)
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS", 2 * 16 * 24)
    net(nt)
    assert routed == STEM_CALLS[:3], routed
    monkeypatch.setattr(fused, "DFORMER_TRAIN_MIN_PIXELS", 0)
    del routed[:]
    # a BatchNorm put in eval mode inside a training graph keeps its module (running statistics, untouched)
    bn16.eval()
    before = (bn16.running_mean.clone(), int(bn16.num_batches_tracked))
    out = net(nt)["0"].tensors
    assert routed == STEM_CALLS[1:] and out.grad_fn is not None
    assert torch.equal(bn16.running_mean, before[0]) and int(bn16.num_batches_tracked) == before[1]
    bn16.train()
    del routed[:]
    # no_grad in train mode: nothing to differentiate, the modules (batch statistics) as before
    with torch.no_grad():
        net(nt)
    assert not routed
    # frozen parameters, but the input asks for a gradient: the kernels, computing the input gradient alone
    net.requires_grad_(False)
    nt_grad, _ = _input(requires_grad=True)
    out = net(nt_grad)["0"].tensors
    assert routed == STEM_CALLS
    (out * g).sum().backward()
    assert nt_grad.tensors.grad is not None and all(p.grad is None for p in net.parameters())


def test_frozen_stem_in_eval_keeps_the_folded_route(routed, monkeypatch):
    from models.dformer_backbone import DFormerBackbone
    nt, _ = _input()
    net = _stem().eval().requires_grad_(False)
    folded = []
    real = DFormerBackbone._forward_folded
    monkeypatch.setattr(DFormerBackbone, "_forward_folded", lambda self, stages, x: folded.append(1) or real(self, stages, x))
    assert torch.is_grad_enabled()
    out = net(nt)["0"].tensors
    assert folded == [1] and not routed and out.grad_fn is None


LR = 1e-3


def _two_steps(net, nt, g):
    """forward, backward, SGD step, forward -> {out1, out2, every parameter and buffer after the step} (detached, CPU)"""
    opt = torch.optim.SGD(net.parameters(), lr=LR)
    out1 = net(nt)["0"].tensors
    (out1 * g).sum().backward()
    opt.step()
    out2 = net(nt)["0"].tensors
    res = {"out1": out1, "out2": out2}
    res.update({"state." + k: v for k, v in net.state_dict().items() if v.is_floating_point()})
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _cpu_two_steps(dtype):
    from models.dformer_backbone import DFormerBackbone
    from util.misc import NestedTensor
    torch.manual_seed(0)
    net = fill_params_by_name(DFormerBackbone(train_backbone=True, freeze_batchnorm=False), seed=dc.STEM_SEED).to(dtype).train()
    depth, g = dc.stem_inputs()
    nt = NestedTensor(depth.to(dtype), torch.zeros(depth.shape[0], depth.shape[2], depth.shape[3], dtype=torch.bool))
    return _two_steps(net, nt, g.to(dtype))


def _within_yardstick(ref, yard, got, what):
    worst = []
    for n in sorted(ref):
        y, err = dc.rel_err(yard[n], ref[n]), dc.rel_err(got[n], ref[n])
        print(f"  {what} {n}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}")
        if not err <= dc.YARDSTICK_FACTOR * y:
            worst.append(f"{n}: gpu {err:.3e} against {dc.YARDSTICK_FACTOR} x {y:.3e}")
    assert not worst, what + ": " + "; ".join(worst)


def test_next_forward_after_an_optimizer_step_uses_the_new_weights_and_statistics(routed, monkeypatch):
    """The route keeps nothing derived from the weights (the BatchNorm kernels read the parameters in place), and the running
    statistics it writes move ``derived_key``: the folded eval route that follows a training step is rebuilt from them.
    Both forwards, the stepped parameters and the running statistics meet the fp64 CPU module within the yardstick rule
    (yardstick: the fp32 CPU module), on the route and, as a control, with the switch off."""
    from models import fused
    ref, yard = _cpu_two_steps(torch.float64), _cpu_two_steps(torch.float32)
    assert dc.rel_err(ref["out2"], ref["out1"]) > 1e3 * dc.rel_err(yard["out2"], ref["out2"]), "the step must show in the next forward"
    nt, g = _input()
    net = _stem()
    stages = net.depth_backbone.downsample_layers_e[:-1]
    mods = [m for m in stages.modules() if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))]
    net.eval()
    with torch.no_grad():
        y_before = net(nt)["0"].tensors.clone()                # builds the folded plan
    key_before, plan_before = fused.derived_key(*mods), net._folded[1]
    net.train()
    got = _two_steps(net, nt, g)
    assert len(routed) == 2 * len(STEM_CALLS)
    _within_yardstick(ref, yard, got, "route on")
    assert fused.derived_key(*mods) != key_before, "the kernel's running-statistics update must be visible to derived_key"
    net.eval()
    with torch.no_grad():
        y_after = net(nt)["0"].tensors
    assert net._folded[1] is not plan_before and net._folded[0] == fused.derived_key(*mods) and not torch.equal(y_after, y_before)
    assert fused.drop_derived(net) >= 1 and net.__dict__.get("_folded") is None
    # the same two steps on the modules
    del routed[:]
    monkeypatch.setattr(fused, "DFORMER_TRAIN", False)
    _within_yardstick(ref, yard, _two_steps(_stem(), nt, g), "route off")
    assert not routed


def _interm(net, nt):
    return {k: v.tensors.detach().cpu() for k, v in net(nt).items()}


def test_return_interm_layers_gives_the_modules_maps(routed, monkeypatch):
    """The three per-stage maps, route on and route off, each within the yardstick rule of the fp64 CPU module's maps."""
    from models import fused
    from models.dformer_backbone import DFormerBackbone
    from util.misc import NestedTensor
    depth, _ = dc.stem_inputs()
    cpu = {}
    for dtype in (torch.float64, torch.float32):
        torch.manual_seed(0)
        m = fill_params_by_name(DFormerBackbone(train_backbone=True, freeze_batchnorm=False, return_interm_layers=True), seed=dc.STEM_SEED)
        cpu[dtype] = _interm(m.to(dtype).train(), NestedTensor(depth.to(dtype), torch.zeros(2, 64, 96, dtype=torch.bool)))
    nt, _ = _input()
    on_nt = _stem(return_interm_layers=True)(nt)
    assert routed == STEM_CALLS and sorted(on_nt) == ["0", "1", "2"]
    assert all(v.tensors.grad_fn is not None for v in on_nt.values())
    _within_yardstick(cpu[torch.float64], cpu[torch.float32], {k: v.tensors.detach().cpu() for k, v in on_nt.items()}, "maps, route on")
    monkeypatch.setattr(fused, "DFORMER_TRAIN", False)
    off_nt = _stem(return_interm_layers=True)(nt)
    assert routed == STEM_CALLS
    _within_yardstick(cpu[torch.float64], cpu[torch.float32], {k: v.tensors.detach().cpu() for k, v in off_nt.items()}, "maps, route off")
    for k in on_nt:
        assert on_nt[k].tensors.shape == off_nt[k].tensors.shape and torch.equal(on_nt[k].mask, off_nt[k].mask)
