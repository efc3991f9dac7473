"""GPU: the opt-in bf16 FFN route of the transformer layers (models.fused.LINEAR_BF16, transformer_layers._ffn_bf16).
Every layer type runs on 2 frames of a 5 x 6 level, or 21 queries, in eval() under no_grad with a spy on dfx.ops.linear and on
dfx.ops.linear_bf16: off (the default) nothing changes; on, the FFN is two linear_bf16 calls (one for the single-Linear GELU
FFN of the fusion layers) plus add_layernorm, bit-equal to the same calls composed by hand, and every other linear call is
untouched.  The layer outputs' deviation from the fp32 route is printed, not asserted: what is asserted is the operator's
bounds (tests/test_gemm_bf16_gpu.py)."""
import pytest
import torch

import _lifecycle as L
from _param_fill import fill_params_by_name

pytestmark = pytest.mark.gpu

KINDS = ["enc", "dec", "tqe", "tdtd", "fusion_v2", "latefusion"]
PAIR = {"enc", "dec", "tqe", "tdtd"}            # linear1 + ReLU + linear2; the fusion layers have one Linear + GELU


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def build(kind, d_ffn=1024):
    from models import transformer_layers as tl
    ctor = {"enc": lambda: tl.DeformableTransformerEncoderLayer(256, d_ffn, 0.1, "relu", 1, 8, 4),
            "dec": lambda: tl.DeformableTransformerDecoderLayer(256, d_ffn, 0.1, "relu", 1, 8, 4),
            "tqe": lambda: tl.TemporalQueryEncoderLayer(256, d_ffn, 0.1, "relu", 8),
            "tdtd": lambda: tl.TemporalDeformableTransformerEncoderLayer(256, d_ffn, 0.1, "relu", 1, 8, 4),
            "fusion_v2": lambda: tl.DeformableTransformerFusionLayerV2(256, d_ffn, 0.1, "gelu", 1, 8, 4),
            "latefusion": lambda: tl.DepthDeformableTransformerEncoderLayer(256, d_ffn, 0.1, "relu", 1, 8, 4, True, True, True)}[kind]
    return fill_params_by_name(ctor(), seed=KINDS.index(kind) + 2).cuda().eval()


def inputs(kind):
    from models import transformer_layers as tl
    shapes, lsi = tl.make_level_tensors([(5, 6)], torch.device("cuda"))
    S = 30
    grid = tl.get_reference_points(shapes, torch.ones(2, 1, 2, device="cuda"), "cuda")
    src, pos, depth = rnd(10, 2, S, 256), rnd(11, 2, S, 256), rnd(15, 2, S, 256)
    tgt, qpos = rnd(12, 2, 21, 256), rnd(13, 2, 21, 256)
    ref4 = (torch.rand(2, 21, 1, 4, generator=torch.Generator().manual_seed(14)) * torch.tensor([1, 1, 0.4, 0.4])).cuda()
    return {"enc": (src, pos, grid, shapes, lsi, None),
            "dec": (tgt, qpos, ref4, src, shapes, lsi, None),
            "tqe": (tgt[:1], rnd(16, 1, 55, 256)),
            "tdtd": (tgt, qpos, ref4[:, :, :, :2].contiguous(), src, shapes, lsi, None),
            "fusion_v2": (src, pos, grid, depth, shapes, lsi, None),
            "latefusion": (src, pos, None, shapes, grid, None, depth, shapes, lsi, None, None)}[kind]


def ffn_rows(kind):
    return {"enc": 60, "dec": 42, "tqe": 21, "tdtd": 42, "fusion_v2": 60, "latefusion": 60}[kind]


def ffn_norm(layer, kind):
    return {"enc": "norm2", "fusion_v2": "norm2"}.get(kind, "norm3")


class Spy:
    """Records the outermost calls of ops.linear (linear(norm=...) calls itself) and every call of ops.linear_bf16."""

    def __init__(self, monkeypatch):
        from dfx import ops
        self.linear, self.bf16, self.depth = [], [], 0
        self.real_linear, self.real_bf16 = ops.linear, ops.linear_bf16

        def linear(x, weight, *args, **kw):
            if self.depth == 0:
                self.linear.append({"x": x.detach().clone() if torch.is_tensor(x) else x, "weight": weight, "nargs": len(args),
                                    "kw": tuple(sorted(k for k, v in kw.items() if v is not None and v is not False))})
            self.depth += 1
            try:
                return self.real_linear(x, weight, *args, **kw)
            finally:
                self.depth -= 1

        def linear_bf16(x, weight, bias=None, act=None, residual=None, out_dtype=torch.float32):
            self.bf16.append({"x": x.detach().clone(), "weight": weight, "bias": bias, "act": act, "residual": residual, "out_dtype": out_dtype})
            return self.real_bf16(x, weight, bias, act=act, residual=residual, out_dtype=out_dtype)

        monkeypatch.setattr(ops, "linear", linear)
        monkeypatch.setattr(ops, "linear_bf16", linear_bf16)

    def reset(self):
        self.linear, self.bf16 = [], []


def signature(call):
    x = call["x"]
    shape = tuple(x[0].shape) + tuple(x[1].shape) if isinstance(x, tuple) else tuple(x.shape)
    return (shape, call["weight"].data_ptr(), tuple(call["weight"].shape), call["nargs"], call["kw"])


def switch(monkeypatch, on):
    from models import fused
    monkeypatch.setattr(fused, "LINEAR_BF16", on)


def is_ffn(call, layer, kind):
    ws = [layer.linear1.weight] + ([layer.linear2.weight] if kind in PAIR else [])
    return any(call["weight"] is w for w in ws)


@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_is_the_default_and_makes_no_bf16_call(kind, monkeypatch):
    from models import fused
    import os
    assert fused.LINEAR_BF16 == (os.environ.get("DFX_LINEAR_BF16", "0") == "1")
    switch(monkeypatch, False)
    layer, args, spy = build(kind), inputs(kind), Spy(monkeypatch)
    with torch.no_grad():
        layer(*args)
    assert spy.bf16 == []
    ffn = [c for c in spy.linear if is_ffn(c, layer, kind)]
    # the fp32 fused FFN as it stands: linear1 with the activation in its epilogue, linear2 through linear(norm=...)
    assert [tuple(c["weight"].shape) for c in ffn] == ([(1024, 256), (256, 1024)] if kind in PAIR else [(256, 256)])
    assert "norm" in ffn[-1]["kw"] and all(c["x"].dtype == torch.float32 for c in ffn)
    assert not any("_weight_bf16" in m.__dict__ for m in layer.modules())


@pytest.mark.parametrize("kind", KINDS)
def test_switch_on_routes_the_ffn_and_nothing_else(kind, monkeypatch, capsys):
    from dfx import ops
    layer, args, spy = build(kind), inputs(kind), Spy(monkeypatch)
    switch(monkeypatch, False)
    with torch.no_grad():
        out_fp32 = layer(*args)
    off = spy.linear
    spy.reset()
    switch(monkeypatch, True)
    with torch.no_grad():
        out = layer(*args)
    rows = ffn_rows(kind)
    norm = getattr(layer, ffn_norm(layer, kind))
    W1, b1 = layer.linear1.weight.detach().to(torch.bfloat16), layer.linear1.bias
    if kind in PAIR:
        assert len(spy.bf16) == 2, "exactly two linear_bf16 calls per FFN"
        c1, c2 = spy.bf16
        assert c1["x"].dtype == torch.float32 and c1["x"].numel() == rows * 256 and c1["out_dtype"] == torch.bfloat16
        assert tuple(c1["weight"].shape) == (1024, 256) and c1["act"] == "relu" and c1["residual"] is None and c1["bias"] is b1
        assert c2["x"].dtype == torch.bfloat16 and c2["x"].numel() == rows * 1024 and c2["out_dtype"] == torch.float32
        assert tuple(c2["weight"].shape) == (256, 1024) and c2["act"] is None and c2["bias"] is layer.linear2.bias
        assert torch.equal(c2["residual"], c1["x"]), "the FFN's input is the residual of the second product"
        W2 = layer.linear2.weight.detach().to(torch.bfloat16)
        assert torch.equal(c1["weight"], W1) and torch.equal(c2["weight"], W2)
        x = c1["x"]
        h = spy.real_bf16(x, W1, b1, act="relu", out_dtype=torch.bfloat16)
        assert torch.equal(c2["x"], h)
        want = ops.add_layernorm(spy.real_bf16(h, W2, layer.linear2.bias, residual=x), None, norm)
    else:
        assert len(spy.bf16) == 1, "the GELU FFN of the fusion layers has one Linear"
        c1, = spy.bf16
        assert c1["x"].dtype == torch.float32 and c1["x"].numel() == rows * 256 and c1["out_dtype"] == torch.float32
        assert tuple(c1["weight"].shape) == (256, 256) and c1["act"] == "gelu" and c1["residual"] is None and c1["bias"] is b1
        assert torch.equal(c1["weight"], W1)
        x = c1["x"]
        want = ops.add_layernorm(spy.real_bf16(x, W1, b1, act="gelu"), x, norm)
    assert out.dtype == torch.float32 and torch.equal(out, want.reshape(out.shape)), "the layer is these operator calls, bit for bit"
    # every non-FFN linear call is the one the switch-off run made: same operands, same arguments, same order
    others_off = [c for c in off if not is_ffn(c, layer, kind)]
    assert not any(is_ffn(c, layer, kind) for c in spy.linear)
    assert [signature(c) for c in spy.linear] == [signature(c) for c in others_off] and len(off) - len(others_off) == (2 if kind in PAIR else 1)
    for a, b in zip(spy.linear, others_off):
        assert all(torch.equal(p, q) for p, q in zip(L.tensors_of(a["x"]), L.tensors_of(b["x"])))
    rel = ((out - out_fp32).norm() / out_fp32.norm()).item()
    worst = ((out - out_fp32).abs().max() / out_fp32.abs().max()).item()
    with capsys.disabled():
        print(f"\n  {kind}: bf16 FFN against the fp32 route: relative L2 {rel:.3e}, max |diff| / max |out| {worst:.3e}")
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("kind", KINDS)
def test_grad_mode_keeps_fp32(kind, monkeypatch):
    switch(monkeypatch, True)
    layer, args, spy = build(kind), inputs(kind), Spy(monkeypatch)
    with torch.enable_grad():
        out = layer(*args)
    assert spy.bf16 == [] and out.requires_grad
    assert not any("_weight_bf16" in m.__dict__ for m in layer.modules())


def test_cpu_and_fp64_keep_fp32(monkeypatch):
    switch(monkeypatch, True)
    spy = Spy(monkeypatch)
    tgt, refq = inputs("tqe")
    with torch.no_grad():
        build("tqe").cpu()(tgt.cpu(), refq.cpu())
        build("tqe").double()(tgt.double(), refq.double())
    assert spy.bf16 == []


def test_in_features_not_a_multiple_of_8_keep_fp32(monkeypatch):
    switch(monkeypatch, True)
    spy = Spy(monkeypatch)
    layer = build("tqe", d_ffn=1020)                       # linear2.in_features = 1020: a multiple of 4 (the fp32 route), not of 8
    with torch.no_grad():
        layer(*inputs("tqe"))
    assert spy.bf16 == []
    assert [tuple(c["weight"].shape) for c in spy.linear if is_ffn(c, layer, "tqe")] == [(1020, 256), (256, 1020)]


@pytest.mark.parametrize("kind,which", [("tqe", "linear1"), ("tqe", "linear2"), ("fusion_v2", "linear1")])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64], ids=["bf16", "f64"])
def test_weights_in_another_dtype_make_no_bf16_call(kind, which, dtype, monkeypatch):
    """(a layer whose weights do not match its fp32 input does what it did before - the mismatch is refused downstream)"""
    switch(monkeypatch, True)
    spy = Spy(monkeypatch)
    layer = build(kind)
    getattr(layer, which).to(dtype)
    with torch.no_grad():
        try:
            layer(*inputs(kind))
        except RuntimeError:
            pass
    assert spy.bf16 == []


LIFECYCLE = [("dec", "linear1"), ("dec", "linear2"), ("fusion_v2", "linear1")]


@pytest.mark.parametrize("kind,owner", LIFECYCLE, ids=lambda v: v)
@pytest.mark.parametrize("edit", ["inplace", "load", "replace", "assign"])
def test_weight_copy_follows_every_edit(kind, owner, edit, monkeypatch):
    """in-place add under no_grad, load_state_dict, p.data = new, load_state_dict(assign=True): the next call equals a fresh
    module holding the new weights, bit for bit."""
    switch(monkeypatch, True)
    args = inputs(kind)

    def after_first_runs(layer):
        assert "_weight_bf16" in getattr(layer, owner).__dict__, "the first runs took the bf16 route and kept the copy"

    L.assert_follows(lambda: build(kind), lambda m: m(*args), owner, "weight", edit, after_first_runs)


def test_drop_derived_removes_the_copies_and_counts_them(monkeypatch):
    from models import fused
    from util import memo
    switch(monkeypatch, True)
    layer, args = build("dec"), inputs("dec")
    with torch.no_grad():
        y0 = layer(*args)
    holders = [m for m in layer.modules() if "_weight_bf16" in m.__dict__]
    assert holders == [layer.linear1, layer.linear2]
    others = sum(name in m.__dict__ for m in layer.modules() for name in fused.DERIVED_ATTRIBUTES) + len(memo._MEMO)
    assert fused.drop_derived(layer) == others + 2
    assert not any("_weight_bf16" in m.__dict__ for m in layer.modules())
    with torch.no_grad():
        assert torch.equal(layer(*args), y0)
