"""GPU: grad_value of single-level fused MSDA summed in LDS (csrc/msda_level_backward.hip) against the fp64 statement of
tests/_msda_fused_cases.py on the single-level cases of tests/_msda_level_bwd_cases.py, the C entry's contract (one writer,
every element written, exact zeros, argument checks), the route inside ``dfx.ops.msda_fused_backward`` and ``MSDeformAttn``
in grad mode above the shipped threshold.

Bounds.  Against fp64 the GPU may be at most 4x the CPU's own fp32 autograd error of the same case, relative to the
gradient's largest magnitude (the project's rule, tests/test_msda_fused_backward_gpu.py: two fp32 evaluations of one
computation that differ in summation order).  Against the global-atomic route of the same tree (the switch off) 1e-5,
that file's figure for order-dependent last bits."""
import copy

import pytest
import torch

from tests import _msda_fused_cases as fc
from tests import _msda_level_bwd_cases as lc

pytestmark = pytest.mark.gpu

YARDSTICK_FACTOR = 4
ATOMIC_TOL = 1e-5
KINK_FACTOR, MAX_UNCLEAR = 8, 0.05
ENTRY = "dfx_msda_level_grad_value_f32"


def _gpu_rows(case, strided=False):
    """grad_out, ref, offsets, logits on the GPU; strided: offsets and logits as column slices of one wider buffer."""
    t = {k: case[k].detach().cuda() for k in ("grad_out", "ref", "offsets", "logits")}
    if strided:
        wide = torch.zeros(*t["offsets"].shape[:2], 64 + 32 + 8, device="cuda")
        wide[..., :64], wide[..., 64:96] = t["offsets"], t["logits"]
        t["offsets"], t["logits"] = wide[..., :64], wide[..., 64:96]
        assert t["offsets"].stride(1) == 104 and not t["logits"].is_contiguous()
    return t


def _atomic_route(case, t, monkeypatch):
    """grad_value of the same tree's global-atomic kernel: ops.msda_fused_backward with the switch off."""
    from dfx import ops
    with monkeypatch.context() as mp:
        mp.setattr(ops, "USE_LEVEL_BWD", False)
        return ops.msda_fused_backward(t["grad_out"], case["value"].cuda(), case["shapes"].cuda(), case["lsi"].cuda(),
                                       t["ref"], t["offsets"], t["logits"], need_value=True)[0]


def _within_yardstick(what, got, want, cpu32, other=None):
    yard, err = fc.rel_err(cpu32, want), fc.rel_err(got.cpu(), want)
    extra = "" if other is None else f", atomic route {fc.rel_err(other.cpu(), want):.3e}"
    print(f"  {what}: cpu fp32 {yard:.3e}, gpu {err:.3e}{extra}, max |ref| {want.abs().max().item():.3e}")
    assert err <= YARDSTICK_FACTOR * yard, f"{what}: gpu {err:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}"


# ---- 1. against fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("H,W,N,Lq,strided", lc.KERNEL_CASES)
def test_grad_value_matches_fp64_and_the_atomic_route(H, W, N, Lq, strided, ref_dim, monkeypatch):
    from dfx import ops
    case = lc.make_level_case(H, W, ref_dim, N, Lq)
    want, cpu32 = lc.references(H, W, ref_dim, N, Lq)
    t = _gpu_rows(case, strided)
    got = ops.msda_level_grad_value(t["grad_out"], t["ref"], t["offsets"], t["logits"], N, H, W)
    torch.cuda.synchronize()
    assert got.shape == (N, H * W, 8, 32) and got.is_contiguous()
    atomic = _atomic_route(case, t, monkeypatch)
    _within_yardstick(f"({H}x{W}, N {N}, Lq {Lq}, ref_dim {ref_dim})", got, want, cpu32, atomic)
    diff = fc.rel_err(got, atomic)
    print(f"  against the atomic route {diff:.3e}")
    assert diff < ATOMIC_TOL


# ---- 2. one writer, every element ------------------------------------------------------------------------------
def _raw_entry(t, ref_dim, N, H, W, Lq, grad_value_ptr, off_pitch=None, logit_pitch=None):
    from dfx import _lib
    rc = _lib.load().dfx_msda_level_grad_value_f32(
        t["ref"].data_ptr(), ref_dim, t["offsets"].data_ptr(), t["offsets"].stride(1) if off_pitch is None else off_pitch,
        t["logits"].data_ptr(), t["logits"].stride(1) if logit_pitch is None else logit_pitch, t["grad_out"].data_ptr(),
        N, H, W, Lq, grad_value_ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _embedded(N, S, pad=64):
    """A buffer of 7s with room for grad_value [N,S,8,32] `pad` floats (16-byte aligned) from either end."""
    buf = torch.full((pad + N * S * 256 + pad,), 7.0, device="cuda")
    return buf, buf[pad:pad + N * S * 256].view(N, S, 8, 32)


def test_entry_writes_every_element_once_and_nothing_else():
    from dfx import ops
    H, W, N, Lq = 5, 7, 9, 37
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = _gpu_rows(case)
    buf, inside = _embedded(N, H * W)
    assert _raw_entry(t, 2, N, H, W, Lq, inside.data_ptr()) == 0
    assert (buf[:64] == 7).all() and (buf[-64:] == 7).all()
    assert not (inside == 7).any()
    want = ops.msda_level_grad_value(t["grad_out"], t["ref"], t["offsets"], t["logits"], N, H, W)
    assert fc.rel_err(inside, want) < ATOMIC_TOL
    # no queries: exact zeros in every element, nothing outside
    buf, inside = _embedded(N, H * W)
    empty = {"ref": t["ref"][:, :0].contiguous(), "offsets": t["offsets"][:, :0].contiguous(),
             "logits": t["logits"][:, :0].contiguous(), "grad_out": t["grad_out"][:, :0].contiguous()}
    assert _raw_entry(empty, 2, N, H, W, 0, inside.data_ptr(), 64, 32) == 0
    assert inside.abs().max() == 0 and (buf[:64] == 7).all() and (buf[-64:] == 7).all()
    # zero grad_out: exact zeros
    buf, inside = _embedded(N, H * W)
    assert _raw_entry(dict(t, grad_out=torch.zeros_like(t["grad_out"])), 2, N, H, W, Lq, inside.data_ptr()) == 0
    assert inside.abs().max() == 0 and (buf[:64] == 7).all() and (buf[-64:] == 7).all()


# ---- 3. outside the map ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_samples_far_outside_the_map_give_exact_zeros(ref_dim, sign):
    H, W, N, Lq = 5, 7, 3, 37
    case = lc.make_level_case(H, W, ref_dim, N, Lq)
    t = _gpu_rows(case)
    t["offsets"] = sign * (t["offsets"].abs() + 1) * 1000       # every location thousands of pixels beyond the map
    buf, inside = _embedded(N, H * W)
    assert _raw_entry(t, ref_dim, N, H, W, Lq, inside.data_ptr()) == 0
    assert inside.abs().max() == 0 and (buf[:64] == 7).all() and (buf[-64:] == 7).all()


# ---- 4. collisions ---------------------------------------------------------------------------------------------
def test_every_query_adding_into_the_same_tokens(monkeypatch):
    from dfx import ops
    H, W, N, Lq = 20, 31, 1, 1100
    case = lc.make_level_case(H, W, 2, N, Lq, True)
    want, cpu32 = lc.references(H, W, 2, N, Lq, True)
    assert (want.abs().amax((0, 2, 3)) > 0).sum() <= 8 * 4 * 4          # at most 32 samples x 4 corners hold anything
    t = _gpu_rows(case)
    got = ops.msda_level_grad_value(t["grad_out"], t["ref"], t["offsets"], t["logits"], N, H, W)
    _within_yardstick("collisions", got, want, cpu32, _atomic_route(case, t, monkeypatch))


# ---- 5. argument checks ----------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_before_any_launch():
    from dfx import _lib
    H, W, N, Lq = 5, 7, 3, 37
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = _gpu_rows(case)
    buf = torch.full((N * 60 * 100 * 256,), 7.0, device="cuda")         # large enough for the level that is refused
    err = lambda: _lib.load().dfx_last_error()
    assert _raw_entry(t, 2, N, 60, 100, Lq, buf.data_ptr()) != 0 and b"does not fit" in err()
    assert _raw_entry(t, 3, N, H, W, Lq, buf.data_ptr()) != 0 and b"ref_dim" in err()
    assert _raw_entry(t, 2, N, H, W, Lq, buf.data_ptr(), off_pitch=66) != 0 and b"pitches" in err()
    assert _raw_entry(t, 2, N, H, W, Lq, None) != 0 and b"null pointer" in err()
    assert (buf == 7).all()


# ---- 6. the route ----------------------------------------------------------------------------------------------
def _spy_on_calls(monkeypatch):
    from dfx import ops
    names, real = [], ops._call

    def spy(what, name, dev, *args):
        names.append(name)
        return real(what, name, dev, *args)

    monkeypatch.setattr(ops, "_call", spy)
    return names


def _fused_backward(case, **kw):
    from dfx import ops
    t = {k: case[k].cuda() for k in ("grad_out", "value", "shapes", "lsi", "ref", "offsets", "logits")}
    res = ops.msda_fused_backward(t["grad_out"], t["value"], t["shapes"], t["lsi"], t["ref"], t["offsets"], t["logits"], **kw)
    torch.cuda.synchronize()
    return res


def test_fused_backward_takes_the_level_route(monkeypatch):
    from dfx import ops
    case = lc.make_level_case(5, 7, 4, 3, 37)
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", False)
    off = _fused_backward(case, need_value=True, need_ref=True)
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", True)
    monkeypatch.setattr(ops, "LEVEL_BWD_MIN_QUERIES", 0)
    names = _spy_on_calls(monkeypatch)
    on = _fused_backward(case, need_value=True, need_ref=True)
    assert names == ["dfx_msda_fused_backward_f32", ENTRY]
    for a, b in zip(on[1:], off[1:]):
        assert torch.equal(a, b)
    assert on[0].shape == off[0].shape and fc.rel_err(on[0], off[0]) < ATOMIC_TOL
    del names[:]
    none = _fused_backward(case, need_value=False, need_ref=True)
    assert names == ["dfx_msda_fused_backward_f32"] and none[0] is None
    del names[:]
    _fused_backward(fc.make_case(2, 2, 3, 37), need_value=True)
    assert names == ["dfx_msda_fused_backward_f32"]


def test_below_the_threshold_the_atomic_route_stays(monkeypatch):
    from dfx import ops
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", True)
    assert 3 * 37 < ops.LEVEL_BWD_MIN_QUERIES
    names = _spy_on_calls(monkeypatch)
    _fused_backward(lc.make_level_case(5, 7, 2, 3, 37), need_value=True)
    assert names == ["dfx_msda_fused_backward_f32"]


# ---- 7. the module ---------------------------------------------------------------------------------------------
# (helpers as in tests/test_msda_fused_backward_gpu.py)
class _CoreOp:
    """Stand-in for MSDeformAttnFunction on CPU tensors: the differentiable plain-tensor statement; records the locations."""

    def __init__(self, sizes):
        self.sizes, self.locs = sizes, []

    def apply(self, value, shapes, lsi, loc, aw, step):
        self.locs.append(loc.detach().double())
        return fc.ms_deform_attn_core_pytorch(value, self.sizes, loc, aw)


class _Forbidden:
    def apply(self, *a):
        raise AssertionError("MSDeformAttnFunction called on the fused training route")


def _unclear_queries(loc64, loc32, sizes):
    """[N,Lq] mask of the queries with a pixel coordinate within KINK_FACTOR x (worst fp32 - fp64 coordinate difference)
    of an integer in the fp64 run, and that difference."""
    wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=torch.float64)[None, None, None, :, None, :]
    p64, p32 = loc64 * wh - 0.5, loc32 * wh - 0.5
    noise = (p32 - p64).abs().max().item()
    near = (p64 - torch.round(p64)).abs() < KINK_FACTOR * noise
    return near.flatten(2).any(-1), noise


def _leaves_run(fn, leaves, params, gout, device, dtype):
    """Run fn(leaves on device) -> out; (out, {name: gradient}) of sum(out * gout) for every leaf and parameter."""
    t = {k: v.detach().to(device=device, dtype=dtype).requires_grad_() for k, v in leaves.items()}
    out = fn(t)
    if gout is None:
        return out.detach().cpu().double(), None
    named = dict(t, **params)
    grads = torch.autograd.grad((out * gout.to(device=device, dtype=dtype)).sum(), list(named.values()), allow_unused=True)
    return out.detach().cpu().double(), {k: g.detach().cpu().double() for k, g in zip(named, grads) if g is not None}


# 1100 queries per frame on the 50 x 84 level; 9 frames put the launch (9900 queries) above the shipped threshold of 9600,
# the smallest launch measured faster than the atomics (one frame, 1100 queries, is below it and takes the atomics)
MODULE_SIZE, MODULE_N, MODULE_LQ = (50, 84), 9, 1100


def module_case(ref_dim):
    from models.ops.modules import MSDeformAttn
    torch.manual_seed(40 + ref_dim)
    m = MSDeformAttn(256, 1, 8, 4).train()
    with torch.no_grad():     # the initialisation zeroes these; give the sampling something to differentiate
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    sizes = [MODULE_SIZE]
    shapes, lsi = fc.level_tensors(sizes)
    N, Lq, S = MODULE_N, MODULE_LQ, MODULE_SIZE[0] * MODULE_SIZE[1]
    g = torch.Generator().manual_seed(400 + ref_dim)
    ref = 0.1 + 0.8 * torch.rand(N, Lq, 1, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = 0.2 + 0.4 * torch.rand(N, Lq, 1, 2, generator=g)
    leaves = {"query": torch.randn(N, Lq, 256, generator=g), "input_flatten": torch.randn(N, S, 256, generator=g)}
    return m, ref, leaves, torch.randn(N, Lq, 256, generator=g), sizes, shapes, lsi


def _module_on(m, ref, shapes, lsi, device, dtype):
    mod = copy.deepcopy(m).to(device=device, dtype=dtype)
    rp, sh, ls = ref.to(device=device, dtype=dtype), shapes.to(device), lsi.to(device)
    return mod, (lambda t: mod(t["query"], rp, t["input_flatten"], sh, ls))


def cpu_yardsticks(m, ref, shapes, lsi, sizes, leaves, gout, monkeypatch):
    """fp64 and fp32 CPU runs with the rows of grad_out of the unclear queries zeroed -> (masked grad_out, fp64 gradients,
    CPU fp32 gradients, the unclear share)."""
    import models.ops.functions.ms_deform_attn_func as f
    locs = {}
    for dt in (torch.float64, torch.float32):
        op = _CoreOp(sizes)
        monkeypatch.setattr(f, "MSDeformAttnFunction", op)
        _, fn = _module_on(m, ref, shapes, lsi, "cpu", dt)
        _leaves_run(fn, leaves, {}, None, "cpu", dt)
        locs[dt] = op.locs[-1]
    unclear, noise = _unclear_queries(locs[torch.float64], locs[torch.float32], sizes)
    fraction = unclear.float().mean().item()
    print(f"  coordinate noise {noise:.2e}, {fraction:.2%} of the queries unclear")
    assert fraction <= MAX_UNCLEAR
    masked = gout * (~unclear)[..., None]
    res = {}
    for dt in (torch.float64, torch.float32):
        monkeypatch.setattr(f, "MSDeformAttnFunction", _CoreOp(sizes))
        mod, fn = _module_on(m, ref, shapes, lsi, "cpu", dt)
        res[dt] = _leaves_run(fn, leaves, dict(mod.named_parameters()), masked, "cpu", dt)[1]
    return masked, res[torch.float64], res[torch.float32], fraction


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_module_trains_with_grad_value_summed_in_lds(ref_dim, monkeypatch):
    """MSDeformAttn(256, 1, 8, 4).train() on a 50 x 84 level, 9 frames of 1100 queries: gradients of every parameter, the query and
    input_flatten against the fp64 CPU module within 4x the CPU fp32 figure; the level entry ran, once."""
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    assert ops.USE_LEVEL_BWD and ops.level_backward_supported(1, *MODULE_SIZE, MODULE_N, MODULE_LQ)
    m, ref_points, leaves, gout, sizes, shapes, lsi = module_case(ref_dim)
    masked, ref, cpu32, _ = cpu_yardsticks(m, ref_points, shapes, lsi, sizes, leaves, gout, monkeypatch)
    monkeypatch.setattr(f, "MSDeformAttnFunction", _Forbidden())
    names = _spy_on_calls(monkeypatch)
    mod, fn = _module_on(m, ref_points, shapes, lsi, "cuda", torch.float32)
    _, got = _leaves_run(fn, leaves, dict(mod.named_parameters()), masked, "cuda", torch.float32)
    assert names.count(ENTRY) == 1 and names.count("dfx_msda_fused_backward_f32") == 1
    assert set(got) == set(ref), set(ref) ^ set(got)
    worst = []
    for k in sorted(ref):
        yard, err = fc.rel_err(cpu32[k], ref[k]), fc.rel_err(got[k], ref[k])
        print(f"  d{k}: cpu fp32 {yard:.3e}, gpu {err:.3e}, max |ref| {ref[k].abs().max().item():.3e}")
        if err > YARDSTICK_FACTOR * yard:
            worst.append(f"d{k}: gpu {err:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}")
    assert not worst, "; ".join(worst)
