"""GPU: the opt-in bf16 Linear route of grad mode (models.fused.LINEAR_BF16_TRAIN -> dfx.ops.linear_bf16_train).  On: a
models.fused.Linear is one linear_bf16_train call, bit-equal to linear_bf16 forwards and to linear_bf16_backward backwards; off (the
default) nothing changes; everything the route does not take keeps its present route; frozen parameters make no launch of their
own; the two bf16 weight copies follow every weight update; an encoder layer routes its Linears and nothing else; and a small
regression still trains."""
import types

import pytest
import torch
import torch.nn.functional as F

from _param_fill import fill_params_by_name

pytestmark = pytest.mark.gpu

U, EPS = 2.0 ** -8, 2.0 ** -23
BF16_NAMES = ("linear_bf16", "linear_bf16_train", "linear_bf16_backward")


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def switch(monkeypatch, on, min_elements=0):
    """(the switch and the size rule are read at call time; the rule is a speed matter, so these small cases set it aside)"""
    from models import fused
    monkeypatch.setattr(fused, "LINEAR_BF16_TRAIN", on)
    monkeypatch.setattr(fused, "LINEAR_BF16_TRAIN_MIN_ELEMENTS", min_elements)


class Spy:
    """Records the outermost call of every public function of dfx.ops: (name, shapes of its tensor arguments)."""

    def __init__(self, monkeypatch):
        from dfx import ops
        self.calls, self.depth, self.real = [], 0, {}
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == ops.__name__:
                self.real[name] = fn
                monkeypatch.setattr(ops, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def wrapped(*args, **kw):
            if self.depth == 0:
                self.calls.append((name, tuple(tuple(a.shape) for a in args if torch.is_tensor(a)), args, kw))
            self.depth += 1
            try:
                return fn(*args, **kw)
            finally:
                self.depth -= 1
        return wrapped

    def names(self):
        return [c[0] for c in self.calls]

    def count(self, name):
        return self.names().count(name)

    def reset(self):
        self.calls = []


def make_linear(n_in, n_out, seed=3, bias=True):
    from models import fused
    lin = fused.Linear(n_in, n_out, bias=bias)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / n_in ** 0.5)
    return lin.cuda()


def run(lin, x, go):
    """forward + backward -> (y, grad_x, grad_w, grad_b), detached clones"""
    x = x.detach().clone().requires_grad_(True)
    for p in lin.parameters():
        p.grad = None
    y = lin(x)
    y.backward(go)
    return (y.detach().clone(), x.grad.clone(), lin.weight.grad.clone(), None if lin.bias is None else lin.bias.grad.clone())


# ---- switch on -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(256, 1024), (1024, 256)])
def test_switch_on_is_one_linear_bf16_train_call_with_the_operator_bits(n_in, n_out, monkeypatch, capsys):
    from dfx import ops
    lin, x, go = make_linear(n_in, n_out), rnd(1, 2, 30, n_in), rnd(2, 2, 30, n_out)
    spy = Spy(monkeypatch)
    switch(monkeypatch, True)
    y, gx, gw, gb = run(lin, x, go)
    assert spy.count("linear_bf16_train") == 1 and spy.count("linear_train") == 0 and spy.count("linear_bf16_backward") == 1
    wb = lin.weight.detach().to(torch.bfloat16)
    assert torch.equal(y, spy.real["linear_bf16"](x, wb, lin.bias))
    ox, ow, ob = spy.real["linear_bf16_backward"](go, x, wb.t().contiguous())
    assert torch.equal(gx, ox) and torch.equal(gw, ow) and torch.equal(gb, ob)
    assert gw.shape == lin.weight.shape and gw.dtype == torch.float32
    # ... and the operator bounds against fp64 (tests/test_linear_bf16_train_gpu.py), with M = 60 rows
    M = 60
    g2, x2 = go.reshape(M, n_out), x.reshape(M, n_in)
    gr, xr, wd = g2.to(torch.bfloat16).double(), x2.to(torch.bfloat16).double(), wb.double()
    ratios = {
        "grad_x": ((gx.reshape(M, n_in).double() - gr @ wd).abs() / (n_out * EPS * (gr.abs() @ wd.abs()) + EPS * (gr @ wd).abs())).max().item(),
        "grad_w": ((gw.double() - gr.t() @ xr).abs() / (M * EPS * (gr.abs().t() @ xr.abs()) + EPS * (gr.t() @ xr).abs())).max().item(),
        "grad_w vs unrounded": ((gw.double() - g2.double().t() @ x2.double()).abs()
                                / (M * EPS * (gr.abs().t() @ xr.abs()) + EPS * (gr.t() @ xr).abs()
                                   + (2 * U + U * U) * (g2.double().abs().t() @ x2.double().abs()))).max().item(),
        "grad_b": ((gb.double() - g2.double().sum(0)).abs() / (M * EPS * g2.double().abs().sum(0))).max().item(),
    }
    with capsys.disabled():
        print(f"\n  {n_in} -> {n_out}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1, ratios
    assert "_weight_bf16_pair" in lin.__dict__ and "_weight_bf16" not in lin.__dict__


# ---- switch off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(256, 1024), (1024, 256)])
def test_switch_off_is_linear_train_bit_for_bit_and_leaves_no_attribute(n_in, n_out, monkeypatch):
    import os
    from dfx import ops
    from models import fused
    assert fused.LINEAR_BF16_TRAIN == (os.environ.get("DFX_LINEAR_BF16_TRAIN", "0") == "1")
    lin, x, go = make_linear(n_in, n_out), rnd(1, 2, 30, n_in), rnd(2, 2, 30, n_out)
    before = set(lin.__dict__)
    spy = Spy(monkeypatch)
    switch(monkeypatch, False)
    y, gx, gw, gb = run(lin, x, go)
    assert spy.count("linear_train") == 1 and not any(n in BF16_NAMES for n in spy.names())
    assert set(lin.__dict__) == before
    xr = x.detach().clone().requires_grad_(True)
    w, b = lin.weight.detach().clone().requires_grad_(True), lin.bias.detach().clone().requires_grad_(True)
    yr = spy.real["linear_train"](xr, w, b)
    yr.backward(go)
    assert torch.equal(y, yr.detach()) and torch.equal(gx, xr.grad) and torch.equal(gw, w.grad) and torch.equal(gb, b.grad)


# ---- fallbacks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["in_not_8", "out_not_8", "wide", "cpu", "fp64", "autocast", "no_grad"])
def test_what_the_route_does_not_take_keeps_its_route_and_makes_no_bf16_call(case, monkeypatch):
    n_in, n_out = {"in_not_8": (252, 256), "out_not_8": (256, 252), "wide": (256, 1032)}.get(case, (256, 256))
    lin, x = make_linear(n_in, n_out), rnd(1, 2, 30, n_in)
    if case == "cpu":
        lin, x = lin.cpu(), x.cpu()
    if case == "fp64":
        lin, x = lin.double(), x.double()

    def forward(record):
        spy = Spy(monkeypatch) if record else None
        xi = x.detach().clone().requires_grad_(True)
        if case == "autocast":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = lin(xi)
        elif case == "no_grad":
            with torch.no_grad():
                y = lin(xi)
        else:
            y = lin(xi)
        if y.requires_grad:
            y.float().sum().backward()
        return y.detach().clone(), spy

    switch(monkeypatch, False)
    want, spy_off = forward(True)
    monkeypatch.undo()
    switch(monkeypatch, True)
    got, spy_on = forward(True)
    assert spy_on.names() == spy_off.names() and not any(n in BF16_NAMES for n in spy_on.names())
    assert torch.equal(got, want) and "_weight_bf16_pair" not in lin.__dict__
    expected = {"in_not_8": ["linear_train", "linear_backward"], "out_not_8": ["linear_train", "linear_backward"], "wide": [],
                "cpu": [], "fp64": [], "autocast": [], "no_grad": ["linear"]}[case]
    assert spy_on.names() == expected


def test_the_size_rule_keeps_small_calls_on_the_fp32_route(monkeypatch):
    from models import fused
    assert fused.LINEAR_BF16_TRAIN_MIN_ELEMENTS > 300 * (256 + 1024), "300 rows measured slower on this route"
    lin, go = make_linear(256, 256), rnd(2, 64, 256)
    spy = Spy(monkeypatch)
    switch(monkeypatch, True, min_elements=64 * (256 + 256))
    run(lin, rnd(1, 64, 256), go)                              # rows x (in + out) reaches the rule: taken
    assert spy.names() == ["linear_bf16_train", "linear_bf16_backward"]
    spy.reset()
    switch(monkeypatch, True, min_elements=64 * (256 + 256) + 1)
    run(lin, rnd(1, 64, 256), go)
    assert spy.names() == ["linear_train", "linear_backward"]


# ---- frozen parameters ---------------------------------------------------------------------------------------------------
def test_a_frozen_weight_makes_no_weight_gradient_launch_and_nothing_to_train_makes_no_node(monkeypatch):
    from dfx import ops
    switch(monkeypatch, True)
    lin, x, go = make_linear(256, 256), rnd(1, 2, 30, 256), rnd(2, 2, 30, 256)
    want = run(lin, x, go)
    launches, real = [], ops._call

    def counting(what, name, *a):
        launches.append(name)
        return real(what, name, *a)

    monkeypatch.setattr(ops, "_call", counting)
    lin.weight.requires_grad_(False)
    lin.bias.requires_grad_(False)
    lin.weight.grad = lin.bias.grad = None                     # (of the run above)
    xi = x.detach().clone().requires_grad_(True)
    y = lin(xi)
    y.backward(go)
    assert launches == ["dfx_gemm_bf16", "dfx_gemm_bf16"], "the forward and the input gradient"
    assert lin.weight.grad is None and lin.bias.grad is None
    assert torch.equal(y.detach(), want[0]) and torch.equal(xi.grad, want[1])
    del launches[:]
    lin.bias.requires_grad_(True)                              # a bias gradient on its own: grad_out.sum(0), still no weight launch
    y = lin(x.detach())
    y.backward(go)
    assert launches == ["dfx_gemm_bf16"] and torch.equal(lin.bias.grad, go.reshape(-1, 256).sum(0))
    lin.bias.requires_grad_(False)
    del launches[:]                                            # nothing requires a gradient: no node, the same forward bits
    y = ops.linear_bf16_train(x.detach(), lin.weight, lin.bias, *lin.__dict__["_weight_bf16_pair"][1:])
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, want[0]) and launches == ["dfx_gemm_bf16"]


# ---- lifecycle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edit", ["adamw", "load", "replace"])
def test_the_copies_follow_every_weight_update(edit, monkeypatch):
    from dfx import optim
    switch(monkeypatch, True)
    lin, x, go = make_linear(256, 1024), rnd(1, 2, 30, 256), rnd(2, 2, 30, 1024)
    first = run(lin, x, go)
    kept = lin.__dict__["_weight_bf16_pair"]
    assert run(lin, x, go)[0].equal(first[0]) and lin.__dict__["_weight_bf16_pair"] is kept      # no edit: the copies stay
    if edit == "adamw":
        optim.AdamW(lin.parameters(), lr=1e-2).step()         # (the gradients of the run above)
    elif edit == "load":
        lin.load_state_dict({k: v * 1.25 + 0.01 for k, v in lin.state_dict().items()})
    else:
        lin.weight.data = lin.weight.detach() * 1.25 + 0.01
    fresh = make_linear(256, 1024, seed=99)
    fresh.load_state_dict(lin.state_dict())
    got, want = run(lin, x, go), run(fresh, x, go)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], first[0]) and not torch.equal(got[1], first[1])
    w, wt = lin.__dict__["_weight_bf16_pair"][1:]
    assert torch.equal(w, lin.weight.detach().to(torch.bfloat16)) and torch.equal(wt, w.t())


def test_drop_derived_removes_the_copies_and_counts_them(monkeypatch):
    from torch import nn
    from models import fused
    from util import memo
    switch(monkeypatch, True)
    net = nn.Sequential(make_linear(256, 256), nn.ReLU(), make_linear(256, 64, seed=4))
    x = rnd(1, 2, 30, 256).requires_grad_(True)
    y0 = net(x).detach().clone()
    holders = [m for m in net.modules() if "_weight_bf16_pair" in m.__dict__]
    assert holders == [net[0], net[2]]
    memo.clear()
    assert fused.drop_derived(net) == 2 and not any("_weight_bf16_pair" in m.__dict__ for m in net.modules())
    assert torch.equal(net(x).detach(), y0)


# ---- an encoder layer ----------------------------------------------------------------------------------------------------
def test_an_encoder_layer_routes_its_linears_and_nothing_else(monkeypatch, capsys):
    from models import transformer_layers as tl
    layer = fill_params_by_name(tl.DeformableTransformerEncoderLayer(256, 1024, 0.1, "relu", 1, 8, 4), seed=2).cuda().train()
    shapes, lsi = tl.make_level_tensors([(5, 6)], torch.device("cuda"))
    grid = tl.get_reference_points(shapes, torch.ones(2, 1, 2, device="cuda"), "cuda")
    src, pos, go = rnd(10, 2, 30, 256), rnd(11, 2, 30, 256), rnd(12, 2, 30, 256)
    spy = Spy(monkeypatch)

    def once(on):
        switch(monkeypatch, on)
        spy.reset()
        torch.manual_seed(5)                                   # the dropouts of train mode draw the same masks in both runs
        layer.zero_grad(set_to_none=True)
        s = src.detach().clone().requires_grad_(True)
        out = layer(s, pos, grid, shapes, lsi, None)
        out.backward(go)
        grads = {n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None}
        grads["src"] = s.grad.clone()
        return out.detach().clone(), grads, [(c[0], c[1]) for c in spy.calls]

    out_off, grads_off, calls_off = once(False)
    out_on, grads_on, calls_on = once(True)
    rename = {"linear_train": "linear_bf16_train", "linear_backward": "linear_bf16_backward"}
    n_lin = sum(name == "linear_train" for name, _ in calls_off)
    assert n_lin == 6, "linear1, linear2 and the four projections of MSDeformAttn"
    assert sum(name == "linear_bf16_train" for name, _ in calls_on) == n_lin and not any(name in rename for name, _ in calls_on)
    assert len(calls_on) == len(calls_off)
    for (na, sa), (nb, sb) in zip(calls_on, calls_off):
        if nb in rename:       # (x, weight, bias) / (grad_out, x) lead both signatures; the weight copies follow
            k = 3 if nb == "linear_train" else 2
            assert na == rename[nb] and sa[:k] == sb[:k], (na, nb)
        else:
            assert (na, sa) == (nb, sb)
    assert torch.isfinite(out_on).all() and all(torch.isfinite(g).all() for g in grads_on.values())
    assert set(grads_on) == set(grads_off)
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()      # noqa: E731
    with capsys.disabled():
        print(f"\n  encoder layer, bf16 Linear training against the fp32 route: output relative L2 {rel(out_on, out_off):.3e}; "
              f"gradients: worst {max(rel(grads_on[n], grads_off[n]) for n in grads_on):.3e} "
              f"(src {rel(grads_on['src'], grads_off['src']):.3e})")


# ---- training still trains -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["fp32", "bf16"])
def test_a_two_layer_regression_still_trains(on, monkeypatch, capsys):
    """Two fused.Linear (32 -> 64, ReLU, 64 -> 32) fitted to a fixed random two-layer net of the same shape on 96 rows, 60 steps of
    dfx.optim.AdamW(lr=1e-2, weight_decay=1e-4): the last step's MSE is at most 0.05 of the first step's.  (The recipe on the CPU with
    nn.Linear ends at 0.010 - 0.012 of the first loss over eight seeds, on fp32 and on a bf16-rounded emulation of this route alike.)"""
    from dfx import optim
    switch(monkeypatch, on)
    spy = Spy(monkeypatch)
    ta, tb = make_linear(32, 64, seed=20), make_linear(64, 32, seed=21)
    a, b = make_linear(32, 64, seed=22), make_linear(64, 32, seed=23)
    x = rnd(24, 96, 32)
    with torch.no_grad():
        y = tb(F.relu(ta(x)))
    opt = optim.AdamW([*a.parameters(), *b.parameters()], lr=1e-2, weight_decay=1e-4)
    spy.reset()
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = F.mse_loss(b(F.relu(a(x))), y)
        loss.backward()
        opt.step()
        losses.append(loss)
    losses = [v.item() for v in losses]
    with capsys.disabled():
        print(f"\n  {'bf16' if on else 'fp32'} route: first MSE {losses[0]:.4e}, last {losses[-1]:.4e}, ratio {losses[-1] / losses[0]:.4f}")
    assert spy.count("linear_bf16_train" if on else "linear_train") == 120 and spy.count("linear_train" if on else "linear_bf16_train") == 0
    assert losses[-1] <= 0.05 * losses[0]
