"""GPU: the fused attention in grad mode - dfx_mha_train_forward_f32 and dfx_mha_backward_f32 (csrc/mha.hip,
csrc/mha_backward.hip) against the fp64 restatement of tests/_mha_cases.py, the autograd surface of ``dfx.ops.mha``, the
grad-mode route of models/fused_mha.py with and without attention dropout, and the unchanged inference path."""
import copy
import functools

import pytest
import torch
from torch import nn

from tests import _mha_cases as mc

pytestmark = pytest.mark.gpu

YARDSTICK_FACTOR = 4      # the GPU may be this many times the CPU's own fp32 error (the project's factor: test_roi_backward_gpu)


@functools.lru_cache(maxsize=None)
def _case(shape, p, grad_scale=1.0):
    """(case, fp64 reference, the same restatement in fp32 on the CPU), computed once per case and never modified"""
    case = mc.make_case(*shape, p=p, grad_scale=grad_scale)
    return case, mc.restated(case), mc.restated(mc.cast(case, torch.float32))


def _gpu(case, requires=("q", "k", "v")):
    t = {n: case[n].float().cuda() for n in ("q", "k", "v", "grad_out")}
    t["drop"] = None if case["drop"] is None else case["drop"].float().cuda()
    for n in requires:
        t[n].requires_grad_()
    return t


def _run(case, requires=("q", "k", "v"), tensors=None):
    """{out, lse, grad_q, grad_k, grad_v} of the operator on the GPU: lse from the train forward entry, the rest through
    ops.mha and autograd."""
    from dfx import ops
    t = tensors or _gpu(case, requires)
    out = ops.mha(t["q"], t["k"], t["v"], case["heads"], case["scale"], drop=t["drop"])
    assert out.grad_fn is not None
    out.backward(t["grad_out"])
    with torch.no_grad():
        out2, lse = ops.mha_train_forward(t["q"], t["k"], t["v"], case["heads"], case["scale"], t["drop"])
    torch.cuda.synchronize()
    assert torch.equal(out2, out.detach())
    return {"out": out.detach(), "lse": lse, "grad_q": t["q"].grad, "grad_k": t["k"].grad, "grad_v": t["v"].grad}


def _cancellation_bound(case):
    """Where the reference gradient is identically zero (grad_q, grad_k at Lk = 1: dS = P (dP - delta) with P = 1 and
    delta = dP) the result is the rounding of two 32-term dot products that cancel: each within 32 u sum|a||b| (u = 2^-24),
    times the mask value, the scale and the one key / query row it multiplies."""
    H = case["heads"]
    go, v = (mc._split(case[n], H).abs() for n in ("grad_out", "v"))
    top = (go @ v.transpose(-1, -2)).max().item()
    mask = 1.0 if case["drop"] is None else case["drop"].max().item()
    return 2 * 32 * 2.0 ** -24 * top * max(mask, 1.0) * case["scale"] * max(case["q"].abs().max().item(), case["k"].abs().max().item())


ULP = 2.0 ** -23      # one unit in the last place of an fp32 result's largest magnitude


def _compare(case, ref, cpu32, got, names=mc.OUTPUTS):
    """Per output: error relative to the reference's largest magnitude, at most 4x the CPU fp32 figure.
    Lk = 1 only (the softmax of one key is the constant 1): the CPU's exp(0) = 1 makes its out and grad_v exact, a figure of
    zero that no other evaluation order has to match, so there the CPU figure counts as at least one fp32 ulp; and grad_q,
    grad_k are zero up to the rounding of the reference itself, so there the error is absolute against
    ``_cancellation_bound``.  Every other shape keeps 4x the measured figure as it is."""
    one_key = case["shape"][3] == 1
    worst = []
    for n in names:
        top = ref[n].abs().max().item()
        if one_key and n in ("grad_q", "grad_k"):
            err, bound = (got[n].cpu().double() - ref[n]).abs().max().item(), _cancellation_bound(case)
            print(f"  {n}: gpu {err:.3e} absolute (the reference is zero: max |ref| {top:.3e}), bound {bound:.3e}")
        else:
            yard, err = mc.rel_err(cpu32[n], ref[n]), mc.rel_err(got[n].cpu(), ref[n])
            bound = YARDSTICK_FACTOR * (max(yard, ULP) if one_key else yard)
            print(f"  {n}: cpu fp32 {yard:.3e}, gpu {err:.3e}, max |ref| {top:.3e}")
        if err > bound:
            worst.append(f"{n}: gpu {err:.3e} against {bound:.3e}")
    assert not worst, "; ".join(worst)


# ---- operator against fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, mc.DROP_P])
@pytest.mark.parametrize("shape", mc.OPERATOR_SHAPES)
def test_operator_matches_fp64_within_the_measured_yardstick(shape, p):
    """out, lse and the three gradients, in full, against the fp64 restatement; the error is relative to each output's
    largest magnitude and may be 4x what the same restatement in fp32 on the CPU shows."""
    case, ref, cpu32 = _case(shape, p)
    got = _run(case)
    for n in mc.GRADS:
        assert got[n].shape == case[n[5:]].shape and got[n].is_contiguous()
    _compare(case, ref, cpu32, got)


def test_operands_may_be_column_slices_of_a_joint_projection():
    case, ref, cpu32 = _case((2, 8, 70, 70), mc.DROP_P)
    t = _gpu(case, requires=())
    joint = torch.cat([t["q"], t["k"], t["v"]], -1).requires_grad_()
    E = 256
    views = dict(t, q=joint[..., :E], k=joint[..., E:2 * E], v=joint[..., 2 * E:])
    assert views["k"].stride(1) == 3 * E
    from dfx import ops
    out = ops.mha(views["q"], views["k"], views["v"], 8, case["scale"], drop=t["drop"])
    out.backward(t["grad_out"])
    g = joint.grad
    got = {"out": out.detach(), "grad_q": g[..., :E], "grad_k": g[..., E:2 * E], "grad_v": g[..., 2 * E:]}
    _compare(case, ref, cpu32, got, names=("out",) + mc.GRADS)
    plain = _run(case)
    for n in ("out",) + mc.GRADS:
        assert torch.equal(got[n], plain[n]), n


# ---- the forward keeps its bits --------------------------------------------------------------------------------
def _raw_forward(t, case):
    from dfx import _lib
    B, H, Lq, Lk = case["shape"]
    E = 32 * H
    out = torch.empty(B, Lq, E, device="cuda")
    q, k, v = t["q"], t["k"], t["v"]
    code = _lib.load().dfx_mha_f32(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(),
                                   v.stride(0), v.stride(1), out.data_ptr(), Lq * E, E, B, H, Lq, Lk, case["scale"],
                                   torch.cuda.current_stream().cuda_stream)
    assert code == 0
    return out


@pytest.mark.parametrize("groups", [None, 1, 2, 4])
@pytest.mark.parametrize("shape", [(1, 8, 70, 130), (2, 8, 300, 300), (1, 2, 65, 97)])
def test_train_forward_without_a_mask_is_bit_equal_to_the_inference_entry(shape, groups, dfx_env):
    from dfx import ops
    dfx_env("DFX_MHA_GROUPS", groups)
    case, _, _ = _case(shape, 0.0)
    t = _gpu(case, requires=())
    raw = _raw_forward(t, case)
    out, _ = ops.mha_train_forward(t["q"], t["k"], t["v"], case["heads"], case["scale"])
    assert torch.equal(out, raw)
    tracked = ops.mha(t["q"].clone().requires_grad_(), t["k"], t["v"], case["heads"], case["scale"])
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), raw)


def test_no_node_without_a_gradient_to_carry():
    from dfx import ops
    case, _, _ = _case((2, 8, 33, 31), 0.0)
    t = _gpu(case, requires=())
    raw = _raw_forward(t, case)
    plain = ops.mha(t["q"], t["k"], t["v"], case["heads"], case["scale"])
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, raw)
    tg = _gpu(case)
    with torch.no_grad():
        quiet = ops.mha(tg["q"], tg["k"], tg["v"], case["heads"], case["scale"])
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, raw)


# ---- needs_input_grad ------------------------------------------------------------------------------------------
def test_unrequested_gradients_are_skipped_and_the_others_unchanged(monkeypatch):
    from dfx import ops
    case, _, _ = _case((1, 8, 70, 130), mc.DROP_P)
    asked, real = [], ops.mha_backward

    def spy(*a, need_q=True, need_kv=True, **k):
        asked.append((need_q, need_kv))
        res = real(*a, need_q=need_q, need_kv=need_kv, **k)
        assert (res[0] is None) == (not need_q) and (res[1] is None) == (not need_kv) and (res[2] is None) == (not need_kv)
        return res

    monkeypatch.setattr(ops, "mha_backward", spy)
    full, only_q, only_kv, only_v = _run(case), _run(case, requires=("q",)), _run(case, requires=("k", "v")), _run(case, requires=("v",))
    assert asked == [(True, True), (True, False), (False, True), (False, True)]
    assert only_q["grad_k"] is None and only_q["grad_v"] is None and torch.equal(only_q["grad_q"], full["grad_q"])
    assert only_kv["grad_q"] is None and torch.equal(only_kv["grad_k"], full["grad_k"]) and torch.equal(only_kv["grad_v"], full["grad_v"])
    assert only_v["grad_q"] is None and only_v["grad_k"] is None and torch.equal(only_v["grad_v"], full["grad_v"])


def test_backward_entry_checks_its_arguments():
    from dfx import _lib, ops
    case, _, _ = _case((2, 8, 33, 31), 0.0)
    t = _gpu(case, requires=())
    out, lse = ops.mha_train_forward(t["q"], t["k"], t["v"], 8, case["scale"])
    none = ops.mha_backward(t["grad_out"], t["q"], t["k"], t["v"], out, lse, 8, case["scale"], need_q=False, need_kv=False)
    assert none == (None, None, None)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    gk = torch.empty_like(t["k"])
    six = lambda x: (x.data_ptr(), x.stride(0), x.stride(1))
    args = (*six(t["grad_out"]), *six(t["q"]), *six(t["k"]), *six(t["v"]), *six(out), lse.data_ptr(), None)
    code = lib.dfx_mha_backward_f32(*args, None, 0, 0, *six(gk), None, 0, 0, 2, 8, 33, 31, case["scale"], st)
    assert code != 0 and b"both or neither" in lib.dfx_last_error()
    code = lib.dfx_mha_backward_f32(*args, None, 0, 0, *six(gk), *six(gk), 2, 8, 33, 0, case["scale"], st)
    assert code != 0 and b"no keys" in lib.dfx_last_error()
    assert lib.dfx_mha_backward_f32(*args, None, 0, 0, *six(gk), *six(gk), 0, 8, 33, 31, case["scale"], st) == 0
    code = lib.dfx_mha_backward_f32(*args, None, 0, 0, gk.data_ptr() + 4, gk.stride(0), gk.stride(1), *six(gk), 2, 8, 33, 31,
                                    case["scale"], st)
    assert code != 0 and b"aligned" in lib.dfx_last_error()


# ---- bit-reproducible ------------------------------------------------------------------------------------------
def test_two_backward_calls_give_the_same_bits():
    """No atomics and fixed summation orders; the outputs are allocated with ``empty``."""
    case, _, _ = _case((2, 8, 300, 300), mc.DROP_P)
    a = _run(case)
    b = _run(case)
    for n in mc.GRADS:
        assert torch.equal(a[n], b[n]), n
        assert torch.isfinite(b[n]).all(), n


# ---- padding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, mc.DROP_P])
def test_padded_rows_and_keys_contribute_nothing(p):
    """33 queries and 31 keys: 31 padded queries in the key role's second tile, one padded key in the query role's only
    tile, loaded from the last valid row.  With grad_out of order 1000 a padded row or key that is not zeroed exactly adds
    terms of the size of the gradients themselves, far beyond the yardstick."""
    case, ref, cpu32 = _case((1, 8, 33, 31), p, 1024.0)
    _compare(case, ref, cpu32, _run(case))


# ---- the module ------------------------------------------------------------------------------------------------
def _module(dropout, seed=41):
    torch.manual_seed(seed)
    m = nn.MultiheadAttention(256, 8, dropout=dropout).train()
    with torch.no_grad():
        m.in_proj_bias.normal_(0, 0.1)
        m.out_proj.bias.normal_(0, 0.1)
    return m


def _module_inputs(kind, seed=42):
    g = torch.Generator().manual_seed(seed)
    B, Lq, Lk = 2, 30, 30 if kind == "self" else 45
    x = {"a": torch.randn(B, Lq, 256, generator=g), "b": torch.randn(B, Lk, 256, generator=g),
         "c": torch.randn(B, Lk, 256, generator=g), "weight": torch.randn(B, Lq, 256, generator=g)}
    return x


def _call_module(m, x, kind, device, dtype, fn=None):
    """(output, {name: gradient}) of loss = sum(out * weight) through transformer_layers._mha (or ``fn`` in its place):
    self-attention with positional q / k (q = k = a + b, v = a), or cross-attention (q = a, k = b, v = c)."""
    from models.transformer_layers import _mha
    m = copy.deepcopy(m).to(device=device, dtype=dtype)
    t = {n: v.to(device=device, dtype=dtype) for n, v in x.items()}
    leaves = {n: t[n].requires_grad_() for n in (("a", "b") if kind == "self" else ("a", "b", "c"))}
    if kind == "self":
        qk = t["a"] + t["b"]
        out = (fn or _mha)(m, qk, qk, t["a"])
    else:
        out = (fn or _mha)(m, t["a"], t["b"], t["c"])
    leaves.update(dict(m.named_parameters()))
    grads = torch.autograd.grad((out * t["weight"]).sum(), list(leaves.values()))
    return out.detach().cpu().double(), {n: g.detach().cpu().double() for n, g in zip(leaves, grads)}


class _Spy:
    def __init__(self, monkeypatch):
        self.calls = 0
        for name in ("bmm", "baddbmm"):
            monkeypatch.setattr(torch, name, self._wrap(getattr(torch, name)))

    def _wrap(self, real):
        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)
        return spy


def _assert_within_yardstick(ref, cpu32, runs):
    bad = []
    for n in ref:
        yard = mc.rel_err(cpu32[n], ref[n])
        figures = {label: mc.rel_err(g[n], ref[n]) for label, g in runs.items()}
        print(f"  d{n}: cpu fp32 {yard:.3e}, " + ", ".join(f"gpu {label} {e:.3e}" for label, e in figures.items()))
        bad += [f"d{n} ({label}): gpu {e:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}" for label, e in figures.items()
                if e > YARDSTICK_FACTOR * yard]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_module_trains_on_the_fused_route(kind, monkeypatch):
    """nn.MultiheadAttention(256, 8, dropout=0).train() through _mha: the fused route against the module route
    (DFX_MHA_TRAIN off; the forward test's tolerance) and every input and parameter gradient against the fp64 CPU module
    (4x the CPU fp32 figure); torch.bmm / torch.baddbmm are not called on the fused route and are on the other."""
    from models import fused_mha
    m, x = _module(0.0), _module_inputs(kind)
    ref, cpu32 = _call_module(m, x, kind, "cpu", torch.float64), _call_module(m, x, kind, "cpu", torch.float32)
    spy = _Spy(monkeypatch)
    assert fused_mha.MHA_TRAIN
    fused = _call_module(m, x, kind, "cuda", torch.float32)
    assert spy.calls == 0, "grad mode still ran the library route"
    monkeypatch.setattr(fused_mha, "MHA_TRAIN", False)
    library = _call_module(m, x, kind, "cuda", torch.float32)
    assert spy.calls >= 2
    assert torch.allclose(fused[0], library[0], rtol=1e-4, atol=2e-5), (fused[0] - library[0]).abs().max().item()
    assert set(fused[1]) == set(ref[1]) and len(ref[1]) == (2 if kind == "self" else 3) + 4
    _assert_within_yardstick(ref[1], cpu32[1], {"fused": fused[1]})


def test_a_hook_on_the_module_selects_the_module_route(monkeypatch):
    from models import fused_mha
    from models.transformer_layers import _mha
    m = _module(0.0).cuda()
    x = torch.randn(2, 30, 256, device="cuda", requires_grad=True)
    spy = _Spy(monkeypatch)
    assert fused_mha.usable(m, x, x, x)
    _mha(m, x, x, x)
    assert spy.calls == 0
    seen = []
    handle = m.register_forward_hook(lambda mod, args, out: seen.append(1))
    try:
        assert not fused_mha.usable(m, x, x, x)
        _mha(m, x, x, x)
        assert seen and spy.calls >= 2
        with torch.no_grad():
            assert fused_mha.usable(m, x, x, x)
    finally:
        handle.remove()
    handle = m.out_proj.register_forward_pre_hook(lambda mod, args: None)
    try:
        assert not fused_mha.usable(m, x, x, x)
    finally:
        handle.remove()
    assert fused_mha.usable(m, x, x, x)


# ---- attention dropout -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_dropout_draws_the_masks_the_module_draws(kind, monkeypatch):
    """dropout = 0.2 in train mode, torch.manual_seed(s) before each route: the fused route, whose mask comes from
    ``attention_dropout_mask``, and the module, which draws inside, agree in the output (the forward test's tolerance), and
    the gradients of both are within the yardstick of the fp64 CPU restatement with the mask the helper drew under that
    seed - which for the module route holds only if its own mask is that mask."""
    from models import fused_mha
    seed, m, x = 77, _module(0.2), _module_inputs(kind)
    B, Lq, Lk = 2, 30, x["b"].shape[1]
    torch.manual_seed(seed)
    mask = fused_mha.attention_dropout_mask(m, B, Lq, Lk, torch.device("cuda")).cpu()
    assert 0.1 < (mask == 0).float().mean().item() < 0.3
    restated = lambda dtype: (lambda mod, q, k, v: mc.module_reference(mod, q, k, v, mask, dtype))
    ref = _call_module(m, x, kind, "cpu", torch.float64, restated(torch.float64))
    cpu32 = _call_module(m, x, kind, "cpu", torch.float32, restated(torch.float32))
    spy = _Spy(monkeypatch)
    torch.manual_seed(seed)
    fused = _call_module(m, x, kind, "cuda", torch.float32)
    assert spy.calls == 0
    monkeypatch.setattr(fused_mha, "MHA_TRAIN", False)
    torch.manual_seed(seed)
    library = _call_module(m, x, kind, "cuda", torch.float32)
    assert spy.calls >= 2
    print(f"  output: fused against module {(fused[0] - library[0]).abs().max().item():.3e}, "
          f"fused against fp64 {(fused[0] - ref[0]).abs().max().item():.3e}")
    assert torch.allclose(fused[0], library[0], rtol=1e-4, atol=2e-5), (fused[0] - library[0]).abs().max().item()
    _assert_within_yardstick(ref[1], cpu32[1], {"fused": fused[1], "module": library[1]})


# ---- inference unchanged ---------------------------------------------------------------------------------------
def test_inference_is_bit_equal_to_the_raw_forward_entry():
    """ClipRunner under no_grad with ops.mha as shipped against the same run with ops.mha forced onto the inference entry
    point of the library (no autograd wrapper, no mask operand in between)."""
    from dfx import _lib, ops
    from models.clip_inference import ClipRunner
    from tests.test_models_gpu import _build, _clip
    calls = [0]

    def raw(q, k, v, heads, scale):
        calls[0] += 1
        assert not torch.is_grad_enabled()
        B, Lq, E = q.shape
        out = torch.empty((B, Lq, E), dtype=torch.float32, device=q.device)
        code = _lib.load().dfx_mha_f32(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                                       v.data_ptr(), v.stride(0), v.stride(1), out.data_ptr(), Lq * E, E, B, heads, Lq,
                                       k.shape[1], float(scale), torch.cuda.current_stream().cuda_stream)
        assert code == 0
        return out

    clip = _clip(4, 21).cuda()
    model, _ = _build("cuda")
    model = model.cuda()
    with torch.no_grad():
        got = ClipRunner(model, micro_batch=2)(clip)
        saved = ops.mha
        ops.mha = raw
        try:
            want = ClipRunner(model, micro_batch=2)(clip)
        finally:
            ops.mha = saved
    assert calls[0] > 0
    assert torch.equal(got["pred_logits"], want["pred_logits"]) and torch.equal(got["pred_boxes"], want["pred_boxes"])
