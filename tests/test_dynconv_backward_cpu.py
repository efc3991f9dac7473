"""CPU: the yardstick and the host logic of the fused DynamicConv backward - the case builder's cap on zeroed rows, the
fp64 restatement of the backward against autograd, the route rule of ``DynamicConv.forward`` and the entry point's
argument checks.  Nothing here launches a kernel."""
import pytest
import torch

from tests import _dynconv_cases as dc


@pytest.mark.parametrize("K,R,extra", dc.OPERATOR_CASES + dc.PADDING_CASES)
def test_builder_keeps_its_cap_and_the_restatement_equals_autograd(K, R, extra):
    """make_case asserts that at most 3 % of the rows are zeroed; the restated backward (the GPU tests' reference) equals
    fp64 autograd through bmm + layer_norm + relu to 1e-12 of each gradient's largest magnitude."""
    case = dc.make_case(K, R, extra, bias=2.0 if (K, R, extra) in dc.PADDING_CASES else None)
    assert case["fraction"] <= dc.MAX_UNCLEAR and case["noise"] > 0
    assert (case["grad_out"][case["unclear"]] == 0).all() and case["grad_out"].abs().max() > 0
    want, got = dc.autograd_backward(case, torch.float64), dc.restated_backward(case)
    for k in dc.OUTPUTS:
        assert got[k].shape == want[k].shape
        assert dc.rel_err(got[k], want[k]) < 1e-12, k
    if extra:
        assert got["params"][:, 2 * dc.C * dc.DD:].abs().max() == 0


class _FakeFeats:
    """What DynamicConv._fused_route reads of a tensor, claiming to live on the GPU."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, rows=49, contiguous=True):
        self.shape, self._contiguous = (3, rows, 256), contiguous

    def is_contiguous(self):
        return self._contiguous


def _dynamic_conv():
    from models.sparse_roi_head.head import DynamicConv
    cfg = {"MODEL": {"SparseRCNN": {"HIDDEN_DIM": 256, "DIM_DYNAMIC": 64, "NUM_DYNAMIC": 2},
                     "ROI_BOX_HEAD": {"POOLER_RESOLUTION": 1}}}
    return DynamicConv(cfg)


def test_route_rule_in_grad_mode_and_under_no_grad(monkeypatch):
    from models.sparse_roi_head import head
    m, feats = _dynamic_conv(), _FakeFeats()
    with torch.no_grad():
        assert m._fused_route(feats)
    assert m._fused_route(feats), "grad mode takes the fused route"
    assert not m._fused_route(_FakeFeats(rows=65)) and not m._fused_route(_FakeFeats(contiguous=False))
    assert not m._fused_route(torch.zeros(3, 49, 256)), "CPU tensors stay on the library route"
    monkeypatch.setattr(head, "DYNCONV_TRAIN", False)
    assert not m._fused_route(feats)
    with torch.no_grad():
        assert m._fused_route(feats), "the switch is about grad mode only"


@pytest.mark.parametrize("where", ["activation", "norm1", "norm2"])
@pytest.mark.parametrize("kind", ["forward_pre", "forward", "backward"])
def test_a_hook_selects_the_unfused_route_in_grad_mode_only(where, kind):
    m, feats = _dynamic_conv(), _FakeFeats()
    mod = getattr(m, where)
    handle = {"forward_pre": lambda: mod.register_forward_pre_hook(lambda mod_, args: None),
              "forward": lambda: mod.register_forward_hook(lambda mod_, args, out: None),
              "backward": lambda: mod.register_full_backward_hook(lambda mod_, gi, go: None)}[kind]()
    assert not m._fused_route(feats)
    with torch.no_grad():
        assert m._fused_route(feats), "no_grad keeps ignoring hooks"
    handle.remove()
    assert m._fused_route(feats)


def test_a_global_module_hook_selects_the_unfused_route_in_grad_mode():
    from torch.nn.modules.module import register_module_forward_hook
    m, feats = _dynamic_conv(), _FakeFeats()
    handle = register_module_forward_hook(lambda mod, args, out: None)
    try:
        assert not m._fused_route(feats)
        with torch.no_grad():
            assert m._fused_route(feats)
    finally:
        handle.remove()
    assert m._fused_route(feats)


def test_grad_mode_forward_calls_the_operator_and_no_bmm(monkeypatch):
    """DynamicConv.forward with the route predicate forced on and dfx.ops.dynamic_conv replaced by a recorder (CPU
    tensors): grad mode hands feats [K,R,C], params [K, 2*C*dd] and the two LayerNorms to the operator."""
    from dfx import ops
    m = _dynamic_conv()
    calls = []

    def recorder(feats, params, norm1, norm2):
        calls.append((tuple(feats.shape), tuple(params.shape), norm1, norm2, torch.is_grad_enabled()))
        return feats * 1.0

    monkeypatch.setattr(ops, "dynamic_conv", recorder)
    monkeypatch.setattr(type(m), "_fused_route", lambda self, feats: True)
    monkeypatch.setattr(torch, "bmm", lambda *a, **k: pytest.fail("the fused route must not call torch.bmm"))
    out = m(torch.randn(1, 3, 256), torch.randn(1, 3, 256))
    assert out.shape == (3, 256) and out.requires_grad
    assert calls == [((3, 1, 256), (3, 2 * 256 * 64), m.norm1, m.norm2, True)]


def test_backward_entry_rejects_bad_arguments_before_any_launch():
    from dfx import _lib
    lib = _lib.load()
    one, ws = 16, 32

    def call(go=one, feats=one, params=one, p_stride=2 * 256 * 64, g1=one, gf=one, gp=one, gp_stride=2 * 256 * 64, gln=one,
             wsp=ws, K=1, R=49, C=256, dd=64):
        return lib.dfx_dynamic_conv_backward_f32(go, feats, params, p_stride, g1, one, one, one, gf, gp, gp_stride, gln, wsp,
                                                 K, R, C, dd, 1e-5, None)

    for bad, text in ((dict(C=128), b"C = 256"), (dict(dd=32), b"C = 256"), (dict(R=65), b"64 rows"), (dict(R=0), b"bad dimension"),
                      (dict(K=-1), b"bad dimension"), (dict(go=0), b"null"), (dict(feats=0), b"null"), (dict(params=0), b"null"),
                      (dict(g1=0), b"null"), (dict(gln=0), b"null"), (dict(wsp=0), b"null"), (dict(go=20), b"aligned"),
                      (dict(gf=20), b"aligned"), (dict(gp=24), b"aligned"), (dict(p_stride=100), b"2*C*dd"),
                      (dict(gp_stride=2 * 256 * 64 + 2), b"2*C*dd")):
        rc = call(**bad)
        assert rc != 0 and text in lib.dfx_last_error(), (bad, lib.dfx_last_error())
