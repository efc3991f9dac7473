"""GPU: the MSDA operator with a bf16 / fp16 value map and fp32 sampling locations and attention weights
(csrc/msda_forward.hip, csrc/msda_backward.hip; include/dfx_msda.h, dfx_msda_forward_bf16 ...) - what MSDeformAttn
hands the op under torch.autocast.

References are the CPU oracle in fp64 on the half inputs upcast exactly.  u is the unit roundoff of the value
dtype (2^-8 bf16, 2^-11 fp16): half outputs and grad_value within rtol = 2u, atol = 1e-5 * max|ref|; fp32 grad_loc /
grad_aw within test_msda_gpu.py's F32_TOL (its atol as a fraction of the largest reference element, as that file
states it).

Forward elements equal to the fp64 reference rounded to the dtype: at least 99 % for bf16, 97 % for fp16.  The sum
is fp32 (like the fp32 operator's: test_fast_path_rounds_the_fp32_result_once checks the bits), and its error,
relative to the terms, is ~1e-6; where the terms cancel to a small output, fp16's spacing (2^-11 of the output)
is fine enough that the fp32 and fp64 sums round to neighbouring values for 1.3-1.5 % of the elements at the
full-size geometries (bf16: well under 1 %).

The backward geometries keep every sample off the pixel grid lines (see off_grid): there the bilinear
interpolant has a kink, grad_loc jumps, and the fp32 pixel coordinate loc * W - 0.5 may land on the other side of
a line than the fp64 one.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
F32_TOL = dict(rtol=1e-4, atol=2e-5)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")


@pytest.fixture(scope="module")
def msda():
    import MultiScaleDeformableAttention as MSDA
    from dfx import _lib
    _lib.load()
    return MSDA


def lsi_of(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def half_case(seed, dt, N, M, D, Lq, P, shape_list, lo=0.0, hi=1.0, R=None):
    """value in `dt`, loc / aw fp32; R > L gives the over-long location buffer of the temporal decoder."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(shape_list, dtype=torch.long)
    L, S = shapes.shape[0], int(shapes.prod(1).sum())
    value = torch.randn(N, S, M, D, generator=g).to(dt)
    loc = torch.rand(N, Lq, M, R or L, P, 2, generator=g) * (hi - lo) + lo
    aw = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    return value, shapes, lsi_of(shapes), loc, aw


def off_grid(loc, shapes, N, Lq, M, P):
    """Move samples whose pixel coordinate is within 1e-3 of an integer by 3e-3 pixels (in place, on the
    prefix the operator reads: level l of the flat [N, Lq, M, L, P, 2] view)."""
    L = shapes.shape[0]
    view = loc.view(-1)[:N * Lq * M * L * P * 2].view(N, Lq, M, L, P, 2)
    for l in range(L):
        for k, size in ((0, int(shapes[l, 1])), (1, int(shapes[l, 0]))):
            c = view[:, :, :, l, :, k]
            px = c.double() * size - 0.5
            near = (px - px.round()).abs() < 1e-3
            c[near] += 3e-3 / size
    return loc


def gpu(ts):
    return [t.cuda() for t in ts]


def ref_forward(oracle, value, shapes, lsi, loc, aw):
    return oracle.msda_forward(value.double(), shapes, lsi, loc.double(), aw.double())


def assert_half_close(got, ref, dt):
    assert got.dtype == dt and got.shape == ref.shape
    assert torch.allclose(got.cpu().double(), ref, rtol=2 * U[dt], atol=1e-5 * ref.abs().max().item())


EXACT = {torch.bfloat16: 0.99, torch.float16: 0.97}


def assert_forward(out, ref, dt):
    assert_half_close(out, ref, dt)
    exact = (out.cpu() == ref.float().to(dt)).double().mean().item()
    assert exact >= EXACT[dt], f"only {exact:.4f} of the elements are the correctly rounded reference"


def assert_f32_close(got, ref):
    assert got.dtype == torch.float32 and got.shape == ref.shape
    got = got.cpu().double()
    scale = max(1.0, ref.abs().max().item())
    bad = ~torch.isclose(got, ref, rtol=F32_TOL["rtol"], atol=F32_TOL["atol"] * scale)
    if bad.any():
        i = (got - ref).abs().argmax().item()
        raise AssertionError(f"{int(bad.sum())} of {ref.numel()} elements outside F32_TOL; worst at flat index {i}: "
                             f"{got.view(-1)[i].item()} vs {ref.view(-1)[i].item()} (scale {scale})")


ML4 = [(100, 167), (50, 84), (25, 42), (13, 21)]
FAST = {
    # name: (N, M, D, Lq, P, shapes, lo, hi, R)
    "enc_l1": (2, 8, 32, 4200, 4, [(50, 84)], -0.05, 1.05, None),     # production encoder, full size
    "dec_l1": (2, 8, 32, 300, 4, [(50, 84)], 0.0, 1.0, None),
    "ms_l4": (1, 8, 32, 22223, 4, ML4, 0.0, 1.0, None),                # test_full_size_multiscale_call geometry
    "border": (3, 8, 32, 50, 4, [(9, 7)], -0.5, 1.5, None),
    "flat_r3": (1, 8, 32, 300, 4, [(50, 84)], 0.0, 1.0, 3),            # TransVOD over-long location buffer
    "odd_lq": (3, 8, 32, 77, 4, [(9, 7), (4, 3)], -0.1, 1.1, None),    # query pairs straddling batch elements
    "odd_lq_l1": (3, 8, 32, 77, 4, [(9, 7)], -0.1, 1.1, None),         # the same on the 16-byte gather (L = 1)
}
GENERIC = {f"d{d}": (1, 2, d, 2, 2, [(6, 4), (3, 2)], 0.0, 1.0, None) for d in (30, 32, 64, 71, 1025, 2048, 3096)}
GENERIC["p3"] = (2, 8, 32, 77, 3, [(9, 7), (4, 3)], -0.1, 1.1, None)  # P != 4
GENERIC["p1_l1"] = (2, 8, 32, 40, 1, [(6, 5)], -0.1, 1.1, None)
ALL = {**FAST, **GENERIC}


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(ALL))
def test_forward_matches_fp64_reference(msda, oracle, name, dt):
    N, M, D, Lq, P, shp, lo, hi, R = ALL[name]
    args = half_case(11 + Lq + D, dt, N, M, D, Lq, P, shp, lo, hi, R)
    out = msda.ms_deform_attn_forward(*gpu(args), 64)
    assert out.dtype == dt and out.shape == (N, Lq, M * D)
    assert_forward(out, ref_forward(oracle, *args), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(ALL))
def test_backward_matches_fp64_reference(msda, oracle, name, dt):
    N, M, D, Lq, P, shp, lo, hi, R = ALL[name]
    value, shapes, lsi, loc, aw = half_case(23 + Lq + D, dt, N, M, D, Lq, P, shp, lo, hi, R)
    off_grid(loc, shapes, N, Lq, M, P)
    go = torch.randn(N, Lq, M * D, generator=torch.Generator().manual_seed(5)).to(dt)
    rv, rl, ra = oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())
    gv, gl, ga = msda.ms_deform_attn_backward(*gpu([value, shapes, lsi, loc, aw, go]), 64)
    assert_half_close(gv, rv, dt)
    assert_f32_close(gl, rl)
    assert_f32_close(ga, ra)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_unaligned_buffers_take_the_generic_path(msda, oracle, dt):
    """value / out / grad_out not 16-byte aligned: same results through the scalar kernels."""
    value, shapes, lsi, loc, aw = half_case(3, dt, 2, 8, 32, 64, 4, [(9, 7)], -0.1, 1.1)
    off_grid(loc, shapes, 2, 64, 8, 4)
    go = torch.randn(2, 64, 256, generator=torch.Generator().manual_seed(6)).to(dt)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        s = buf[1:].view(t.shape)
        s.copy_(t)
        assert s.is_contiguous() and s.data_ptr() % 16 != 0
        return s

    v, sh, ls, lc, a = gpu([value, shapes, lsi, loc, aw])
    out = msda.ms_deform_attn_forward(shifted(v), sh, ls, lc, a, 64)
    assert_forward(out, ref_forward(oracle, value, shapes, lsi, loc, aw), dt)
    rv, rl, ra = oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())
    gv, gl, ga = msda.ms_deform_attn_backward(shifted(v), sh, ls, lc, a, shifted(go.cuda()), 64)
    assert_half_close(gv, rv, dt)
    assert_f32_close(gl, rl)
    assert_f32_close(ga, ra)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_fast_path_rounds_the_fp32_result_once(msda, dt):
    """The fast path sums exactly as the fp32 operator does: its output is the fp32 result on the upcast
    value, rounded once to the value's dtype (the same bits, not merely close)."""
    value, shapes, lsi, loc, aw = gpu(half_case(8, dt, 2, 8, 32, 4200, 4, [(50, 84)], -0.05, 1.05))
    out = msda.ms_deform_attn_forward(value, shapes, lsi, loc, aw, 64)
    want = msda.ms_deform_attn_forward(value.float(), shapes, lsi, loc, aw, 64).to(dt)
    assert torch.equal(out, want)
    # deterministic
    assert torch.equal(out, msda.ms_deform_attn_forward(value, shapes, lsi, loc, aw, 64))


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_narrow_gather_variant(msda, dfx_env, dt):
    """L = 1 takes the 16-byte gather; DFX_MSDA_HALF_NARROW=1 the 8-byte one of L > 1: the same bits."""
    value, shapes, lsi, loc, aw = gpu(half_case(9, dt, 3, 8, 32, 77, 4, [(9, 7)], -0.1, 1.1))
    wide = msda.ms_deform_attn_forward(value, shapes, lsi, loc, aw, 64)
    dfx_env("DFX_MSDA_HALF_NARROW", "1")
    narrow = msda.ms_deform_attn_forward(value, shapes, lsi, loc, aw, 64)
    assert torch.equal(wide, narrow)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_autograd_function(msda, dt):
    from models.ops.functions import MSDeformAttnFunction
    value, shapes, lsi, loc, aw = gpu(half_case(4, dt, 2, 8, 32, 300, 4, [(20, 31), (10, 16)], -0.1, 1.1))
    go = torch.randn(2, 300, 256, device="cuda").to(dt)
    v, l, a = (t.clone().requires_grad_(True) for t in (value, loc, aw))
    out = MSDeformAttnFunction.apply(v, shapes, lsi, l, a, 64)
    assert out.dtype == dt
    out.backward(go)
    assert (v.grad.dtype, l.grad.dtype, a.grad.dtype) == (dt, torch.float32, torch.float32)
    gv, gl, ga = msda.ms_deform_attn_backward(value, shapes, lsi, loc, aw, go, 64)
    assert torch.equal(l.grad, gl) and torch.equal(a.grad, ga)       # one atomic add per element: exact
    assert torch.allclose(v.grad.float(), gv.float(), rtol=2 * U[dt], atol=1e-5 * gv.float().abs().max().item())


class _Spy:
    """Stands in for MSDeformAttnFunction: records the operand dtypes, then calls ``inner``."""

    def __init__(self, inner, seen):
        self.inner, self.seen = inner, seen

    def apply(self, value, shapes, lsi, loc, aw, step):
        self.seen.append((value.dtype, loc.dtype, aw.dtype))
        return self.inner.apply(value, shapes, lsi, loc, aw, step)


class _Upcast:
    """``inner`` on an fp32 copy of value, result cast back to value's dtype (the comparison route)."""

    def __init__(self, inner):
        self.inner = inner

    def apply(self, value, shapes, lsi, loc, aw, step):
        return self.inner.apply(value.float(), shapes, lsi, loc, aw, step).to(value.dtype)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("L", [1, 4])
def test_module_under_autocast(msda, monkeypatch, dt, L):
    import models.ops.functions.ms_deform_attn_func as f
    from models.ops.modules import MSDeformAttn
    shp = [(20, 31)] if L == 1 else [(16, 20), (8, 10), (4, 5), (2, 3)]
    torch.manual_seed(0)
    m = MSDeformAttn(256, L, 8, 4).cuda().train()
    with torch.no_grad():     # the initialisation zeroes these; give the sampling something to differentiate
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    shapes = torch.as_tensor(shp, dtype=torch.long, device="cuda")
    lsi = lsi_of(shapes)
    N, Lq, S = 2, 100, int(shapes.prod(1).sum())
    g = torch.Generator().manual_seed(1)
    query = torch.randn(N, Lq, 256, generator=g).cuda()
    refp = torch.rand(N, Lq, L, 2, generator=g).cuda()
    inp = torch.randn(N, S, 256, generator=g).cuda().requires_grad_(True)   # (no input needing grad: fused inference route)
    gout = torch.randn(N, Lq, 256, generator=g).cuda()
    real = f.MSDeformAttnFunction

    def run(op):
        seen = []
        monkeypatch.setattr(f, "MSDeformAttnFunction", _Spy(op, seen))
        m.zero_grad()
        with torch.autocast("cuda", dtype=dt):
            out = m(query, refp, inp, shapes, lsi)
        (out.float() * gout).sum().backward()
        monkeypatch.setattr(f, "MSDeformAttnFunction", real)
        return seen, out.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    seen, out, grads = run(real)
    assert seen == [(dt, torch.float32, torch.float32)]
    assert out.dtype == dt
    _, want, want_grads = run(_Upcast(real))
    assert_half_close(out, want.cpu().double(), dt)
    for name, ref in want_grads.items():
        got = grads[name]
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        # grad_value sums fp32 atomics in a run-dependent order: single elements may round to a neighbouring
        # value of the dtype, and value_proj's half-precision weight-gradient GEMM spreads that over a row
        atol = (4 * U[dt] if name.startswith("value_proj") else 1e-5) * ref.abs().max().item()
        assert torch.allclose(got, ref, rtol=2 * U[dt], atol=atol), (name, (got - ref).abs().max().item(), atol)


PATH_A = r"""
import sys, types
PKG, DT = sys.argv[1], sys.argv[2]
sys.path[:0] = [PKG]
pkg = types.ModuleType("models")            # the namespace import of tests/test_integration_path_a.py
pkg.__path__ = [PKG + "/models"]
sys.modules["models"] = pkg
import torch
import models.ops.functions.ms_deform_attn_func as f
from models.ops.modules import MSDeformAttn
dt = getattr(torch, DT)
seen = []
fwd = f.MSDA.ms_deform_attn_forward
def spy(value, shapes, lsi, loc, aw, step):
    seen.append((value.dtype, loc.dtype, aw.dtype))
    return fwd(value, shapes, lsi, loc, aw, step)
f.MSDA.ms_deform_attn_forward = spy
torch.manual_seed(0)
m = MSDeformAttn(256, 1, 8, 4).cuda().train()
shapes = torch.tensor([[20, 31]], device="cuda"); lsi = torch.tensor([0], device="cuda")
q = torch.randn(2, 100, 256, device="cuda"); refp = torch.rand(2, 100, 1, 2, device="cuda")
x = torch.randn(2, 620, 256, device="cuda", requires_grad=True)
with torch.autocast("cuda", dtype=dt):
    out = m(q, refp, x, shapes, lsi)
out.float().square().mean().backward()
torch.cuda.synchronize()
assert seen == [(dt, torch.float32, torch.float32)], seen
assert out.dtype == dt and torch.isfinite(out.float()).all()
assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
print("PATH_A_AUTOCAST_OK")
"""


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_path_a_under_autocast(dt):
    out = subprocess.run([sys.executable, "-c", PATH_A, PKG, dt], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "PATH_A_AUTOCAST_OK" in out.stdout, out.stderr[-2000:]


def test_contract_errors(msda):
    shapes = torch.as_tensor([(3, 3)], dtype=torch.long).cuda()
    lsi = lsi_of(shapes)
    v = torch.randn(3, 9, 8, 32).cuda()
    loc = torch.rand(3, 4, 8, 1, 4, 2).cuda()
    aw = torch.rand(3, 4, 8, 1, 4).cuda()
    go = torch.randn(3, 4, 256).cuda()
    for vdt in DTYPES:
        for ldt in (torch.float16, torch.bfloat16, torch.float64):
            with pytest.raises(RuntimeError, match="fp32"):
                msda.ms_deform_attn_forward(v.to(vdt), shapes, lsi, loc.to(ldt), aw.to(ldt), 64)
            with pytest.raises(RuntimeError, match="fp32"):
                msda.ms_deform_attn_backward(v.to(vdt), shapes, lsi, loc.to(ldt), aw.to(ldt), go.to(vdt), 64)
        with pytest.raises(RuntimeError, match="fp32"):      # only the locations in half
            msda.ms_deform_attn_forward(v.to(vdt), shapes, lsi, loc.to(vdt), aw, 64)
        with pytest.raises(RuntimeError, match="grad_output"):
            msda.ms_deform_attn_backward(v.to(vdt), shapes, lsi, loc, aw, go, 64)
        with pytest.raises(RuntimeError, match="im2col_step"):
            msda.ms_deform_attn_forward(v.to(vdt), shapes, lsi, loc, aw, 2)
        with pytest.raises(RuntimeError, match="contiguous"):
            msda.ms_deform_attn_forward(v.to(vdt).transpose(0, 1).contiguous().transpose(0, 1), shapes, lsi, loc, aw, 64)
    for ldt in DTYPES:                                       # fp32 value: one dtype for all, as before
        with pytest.raises(RuntimeError):
            msda.ms_deform_attn_forward(v, shapes, lsi, loc.to(ldt), aw.to(ldt), 64)
        with pytest.raises(RuntimeError):
            msda.ms_deform_attn_forward(v, shapes, lsi, loc.to(ldt), aw, 64)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_empty_inputs(msda, dt):
    shapes = torch.as_tensor([(3, 3)], dtype=torch.long).cuda()
    lsi = lsi_of(shapes)
    v = torch.randn(2, 9, 8, 32).cuda().to(dt)
    out = msda.ms_deform_attn_forward(v, shapes, lsi, torch.rand(2, 0, 8, 1, 4, 2).cuda(), torch.rand(2, 0, 8, 1, 4).cuda(), 64)
    assert out.shape == (2, 0, 256) and out.dtype == dt
    gv, gl, ga = msda.ms_deform_attn_backward(v, shapes, lsi, torch.rand(2, 0, 8, 1, 4, 2).cuda(),
                                              torch.rand(2, 0, 8, 1, 4).cuda(), torch.randn(2, 0, 256).cuda().to(dt), 64)
    assert gv.dtype == dt and torch.count_nonzero(gv) == 0 and gl.numel() == 0 and ga.numel() == 0
    # S = 0: an empty map; every sample falls outside -> zeros of the value's dtype
    z_shapes = torch.as_tensor([(0, 0)], dtype=torch.long).cuda()
    v0 = torch.empty(2, 0, 8, 32, device="cuda", dtype=dt)
    loc = torch.rand(2, 5, 8, 1, 4, 2).cuda()
    aw = torch.rand(2, 5, 8, 1, 4).cuda()
    out = msda.ms_deform_attn_forward(v0, z_shapes, lsi_of(z_shapes), loc, aw, 64)
    assert out.shape == (2, 5, 256) and out.dtype == dt and torch.count_nonzero(out) == 0
    gv, gl, ga = msda.ms_deform_attn_backward(v0, z_shapes, lsi_of(z_shapes), loc, aw,
                                              torch.randn(2, 5, 256).cuda().to(dt), 64)
    assert gv.shape == v0.shape and gv.dtype == dt
    assert torch.count_nonzero(gl) == 0 and torch.count_nonzero(ga) == 0
    # all samples outside the map / NaN locations: exact zeros, as the fp32 operator
    for fill in (5.0, float("nan")):
        out = msda.ms_deform_attn_forward(v, shapes, lsi, torch.full((2, 6, 8, 1, 4, 2), fill).cuda(),
                                          torch.rand(2, 6, 8, 1, 4).cuda(), 64)
        assert out.dtype == dt and torch.count_nonzero(out) == 0
