"""GPU: which routes take dfx.ops.add_layernorm_train (models.fused.ADDLN_TRAIN) - the tails of an encoder and a decoder layer
in train mode - what they compute against the module chain and the fp64 CPU layer, and the routes that stay as they were.
The size rule is set to 0 rows here: the layers run on 2 frames of a 5 x 6 level."""
import copy

import pytest
import torch
from torch import nn

from tests import test_msda_fused_backward_gpu as fb       # the layer-level yardstick helpers (unclear queries, leaves)
from tests._addln_cases import YARDSTICK_FACTOR, rel_err

pytestmark = pytest.mark.gpu

SIZES = [(5, 6)]
N, S, LQ = 2, 30, 21


@pytest.fixture()
def routed(monkeypatch):
    """size rule 0, and a list that receives (rows, C, live dropout) per call of the new entry"""
    from dfx import ops
    from models import fused
    monkeypatch.setattr(fused, "ADDLN_TRAIN_MIN_ROWS", 0)
    calls, real = [], ops.add_layernorm_train

    def spy(x, residual, norm, dropout=None):
        calls.append((x.numel() // x.shape[-1], x.shape[-1], dropout is not None and dropout.training and dropout.p > 0))
        return real(x, residual, norm, dropout)

    monkeypatch.setattr(ops, "add_layernorm_train", spy)
    return calls


def _layer(kind, p):
    from models import transformer_layers as tl
    torch.manual_seed(5)
    cls = {"encoder": tl.DeformableTransformerEncoderLayer, "decoder": tl.DeformableTransformerDecoderLayer}[kind]
    layer = cls(256, 1024, p, "relu", 1, 8, 4).train()
    attn = layer.self_attn if kind == "encoder" else layer.cross_attn
    with torch.no_grad():     # the initialisation zeroes these; give the sampling something to differentiate
        attn.sampling_offsets.weight.normal_(0, 0.02)
        attn.attention_weights.weight.normal_(0, 0.02)
    g = torch.Generator().manual_seed(6)
    shapes, lsi = fb.fc.level_tensors(SIZES)
    if kind == "encoder":
        leaves = {"src": torch.randn(N, S, 256, generator=g), "pos": torch.randn(N, S, 256, generator=g)}
        ref_points, gout = 0.1 + 0.8 * torch.rand(N, S, 1, 2, generator=g), torch.randn(N, S, 256, generator=g)
    else:
        leaves = {"tgt": torch.randn(N, LQ, 256, generator=g), "query_pos": torch.randn(N, LQ, 256, generator=g),
                  "src": torch.randn(N, S, 256, generator=g)}
        ref_points, gout = 0.1 + 0.8 * torch.rand(N, LQ, 1, 2, generator=g), torch.randn(N, LQ, 256, generator=g)

    def run_on(device, dt, layer=layer):
        mod = copy.deepcopy(layer).to(device=device, dtype=dt)
        rp, sh, ls = ref_points.to(device=device, dtype=dt), shapes.to(device), lsi.to(device)
        if kind == "encoder":
            return mod, (lambda t: mod(t["src"], t["pos"], rp, sh, ls)), None
        return mod, (lambda t: mod(t["tgt"], t["query_pos"], rp, t["src"], sh, ls)), None

    return layer, leaves, gout, run_on


def _gpu_run(run_on, leaves, gout, seed=21):
    mod, fn, _ = run_on("cuda", torch.float32)
    torch.manual_seed(seed)
    return fb._leaves_run(fn, leaves, dict(mod.named_parameters()), gout, "cuda", torch.float32)


@pytest.mark.parametrize("kind,tails", [("encoder", 2), ("decoder", 3)])
def test_layers_in_train_mode_take_the_route_and_agree_with_the_modules(kind, tails, routed, monkeypatch):
    import models.ops.functions.ms_deform_attn_func as f
    from models import fused
    real_msda = f.MSDeformAttnFunction
    # p = 0 first: the layer is the same function on every device, so the fp64 CPU layer is the reference and the fp32 CPU
    # layer the yardstick (rows of grad_out of queries that sample within noise of a pixel edge zeroed, as in
    # tests/test_msda_fused_backward_gpu.py)
    _, leaves, gout, run_on0 = _layer(kind, 0.0)
    masked, ref, cpu32 = fb._cpu_yardsticks(run_on0, SIZES, leaves, gout, monkeypatch)
    monkeypatch.setattr(f, "MSDeformAttnFunction", real_msda)
    assert not routed                                       # CPU runs keep the modules
    out0, got0 = _gpu_run(run_on0, leaves, masked)
    assert len(routed) == tails and not any(live for _, _, live in routed), routed
    assert set(got0) == set(ref), set(ref) ^ set(got0)
    fb._compare(ref, cpu32, got0, sorted(ref), what=f"{kind} p=0 ")
    # p = 0.1 under one seed: route off (the modules, on the GPU) is the reference.  Both are fp32 evaluations of one function
    # with one mask, so they may differ by what the rule allows two such evaluations: 4 x the fp32 CPU figure of that gradient
    # (taken from the p = 0 layer above: the CPU draws another mask).  Another mask would differ at order 1.
    del routed[:]
    _, _, _, run_on = _layer(kind, 0.1)
    out_on, got_on = _gpu_run(run_on, leaves, masked)
    assert len(routed) == tails and all(live for _, _, live in routed), routed
    assert {r for r, _, _ in routed} == {N * (S if kind == "encoder" else LQ)} and {c for _, c, _ in routed} == {256}
    del routed[:]
    monkeypatch.setattr(fused, "ADDLN_TRAIN", False)
    out_off, got_off = _gpu_run(run_on, leaves, masked)
    assert not routed
    assert set(got_on) == set(got_off) == set(ref)
    print(f"  {kind} p=0.1 output: on against off {rel_err(out_on, out_off):.3e}")
    assert (out_on - out_off).abs().max().item() <= 2e-5
    worst = []
    for k in sorted(ref):
        yard, err = rel_err(cpu32[k], ref[k]), rel_err(got_on[k], got_off[k])
        print(f"  {kind} p=0.1 d{k}: cpu fp32 {yard:.3e}, on against off {err:.3e}")
        if err > YARDSTICK_FACTOR * yard:
            worst.append(f"d{k}: {err:.3e} against {YARDSTICK_FACTOR} x {yard:.3e}")
    assert not worst, "; ".join(worst)


def _sites(norm, drop, linear, r, y, x):
    from models import fused, transformer_layers as tl
    return {"apply_post": lambda: fused.apply_post((r, norm, drop), y),
            "_norm_add": lambda: tl._norm_add(norm, r, y, dropout=drop),
            "_linear_norm_add": lambda: tl._linear_norm_add(linear, x, norm, r, dropout=drop)}


def test_each_site_takes_the_route_once_in_grad_mode(routed):
    from models import fused
    norm, drop, linear = nn.LayerNorm(256).cuda(), nn.Dropout(0.1).train(), fused.Linear(64, 256).cuda()
    r, y, x = (torch.randn(2, 7, c, device="cuda", requires_grad=True) for c in (256, 256, 64))
    for name, site in _sites(norm, drop, linear, r, y, x).items():
        del routed[:]
        out = site()
        assert routed == [(14, 256, True)] and out.grad_fn is not None, name


def test_routes_that_stay_as_they_are(routed, monkeypatch):
    from dfx import ops
    from models import fused
    norm, drop, linear = nn.LayerNorm(256).cuda(), nn.Dropout(0.1).train(), fused.Linear(64, 256).cuda()
    r, y, x = (torch.randn(2, 7, c, device="cuda", requires_grad=True) for c in (256, 256, 64))
    # a frozen norm with inputs that need no gradient: the modules, and no grad_fn
    frozen, frozen_linear = copy.deepcopy(norm).requires_grad_(False), copy.deepcopy(linear).requires_grad_(False)
    for name, site in _sites(frozen, drop, frozen_linear, r.detach(), y.detach(), x.detach()).items():
        out = site()
        assert out.grad_fn is None and not out.requires_grad and not routed, name
    # no_grad, autocast, fp64, a hooked norm, the switch off: no call to the new entry
    with torch.no_grad():
        for name, site in _sites(norm, drop, linear, r, y, x).items():
            site()
            assert not routed, name
    with torch.autocast("cuda", dtype=torch.bfloat16):
        for name, site in _sites(norm, drop, linear, r, y, x).items():
            assert site().grad_fn is not None and not routed, name
    n64, l64 = copy.deepcopy(norm).double(), copy.deepcopy(linear).double()
    for name, site in _sites(n64, drop, l64, r.double(), y.double(), x.double()).items():
        assert site().dtype == torch.float64 and not routed, name
    hooked = copy.deepcopy(norm)
    hooked.register_forward_hook(lambda *a: None)
    for name, site in _sites(hooked, drop, linear, r, y, x).items():
        assert site().grad_fn is not None and not routed, name
    monkeypatch.setattr(fused, "ADDLN_TRAIN", False)
    for name, site in _sites(norm, drop, linear, r, y, x).items():
        assert site().grad_fn is not None and not routed, name
    monkeypatch.setattr(fused, "ADDLN_TRAIN", True)
    # no_grad in eval mode: the same ops.add_layernorm call as before, bit for bit
    seen, real = [], ops.add_layernorm
    monkeypatch.setattr(ops, "add_layernorm", lambda *a: seen.append(a) or real(*a))
    idle = nn.Dropout(0.1).eval()
    with torch.no_grad():
        from models import transformer_layers as tl
        got = tl._norm_add(norm, r, y, dropout=idle)
        assert len(seen) == 1 and seen[0][0].data_ptr() == r.data_ptr() and seen[0][1].data_ptr() == y.data_ptr() and seen[0][2] is norm and torch.equal(got, real(r, y, norm))
        got = tl._linear_norm_add(linear, x, norm, r, dropout=idle)
        assert len(seen) == 2 and torch.equal(got, ops.linear(x.contiguous(), linear.weight, linear.bias, residual=r.contiguous(), norm=norm))
    assert not routed


def test_the_size_rule_keeps_smaller_tails_on_the_modules(routed, monkeypatch):
    from models import fused, transformer_layers as tl
    monkeypatch.setattr(fused, "ADDLN_TRAIN_MIN_ROWS", 15)
    norm, drop = nn.LayerNorm(256).cuda(), nn.Dropout(0.1).train()
    r, y = (torch.randn(2, 7, 256, device="cuda", requires_grad=True) for _ in range(2))
    tl._norm_add(norm, r, y, dropout=drop)
    assert not routed
    monkeypatch.setattr(fused, "ADDLN_TRAIN_MIN_ROWS", 14)
    tl._norm_add(norm, r, y, dropout=drop)
    assert routed == [(14, 256, True)]
