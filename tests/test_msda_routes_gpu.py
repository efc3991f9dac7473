"""GPU: every kernel route of the MSDA operator (csrc/msda_forward.hip, msda_backward.hip, msda_fused.hip), the multi-pass
grids of the taps kernels, exact edges, a level_start_index that is not the running sum, 32-bit offsets at their bound and
atomic accumulation under heavy collision.

Most inputs come from the exact family of tests/_msda_cases.py: every product and partial sum is exactly representable in
fp32, so a kernel has to equal the fp64 oracle bit for bit (rounded once to the value dtype for bf16 / fp16), whatever its
summation order; torch.equal is the whole criterion (it takes -0.0 == 0.0).  tests/test_msda_exact_cases.py checks that
claim on the CPU oracle for every case used here.  Random inputs use the criteria the suite already states: F32_TOL
(test_msda_gpu.py), assert_forward (test_msda_half_gpu.py) and the fused test's rtol 1e-4 / atol 5e-5.

Which kernel a row of the route table launches is read from forward_impl / backward_impl; the library does not report it.
profiles/r07_msda_route_coverage.txt is the kernel-name summary of one run of this file under rocprofv3 --kernel-trace.
"""
import functools

import pytest
import torch

from tests import _msda_cases as C
from tests.test_msda_gpu import F32_TOL, rand_case
from tests.test_msda_half_gpu import assert_forward, half_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def msda():
    import MultiScaleDeformableAttention as MSDA
    from dfx import _lib
    _lib.load()  # fail loudly if the HIP library is missing
    return MSDA


def shifted(t):
    """`t` on the device, one element off the allocation's alignment (a slice of a buffer one element longer)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    s = buf[1:].view(t.shape)
    s.copy_(t)
    assert s.is_contiguous() and s.data_ptr() % 16 == t.element_size()
    return s


def device_operands(case, dt, mis=None):
    """The case as the operator takes it for value dtype `dt`; `mis` names the operand to misalign."""
    value, shapes, lsi, loc, aw, go = case
    ldt = torch.float64 if dt == torch.float64 else torch.float32
    ops = {"value": value.to(dt), "loc": loc.to(ldt), "aw": aw.to(ldt), "go": go.to(dt)}
    dev = {k: (shifted(t) if k == mis else t.cuda()) for k, t in ops.items()}
    for k, t in dev.items():
        if k != mis:
            assert t.data_ptr() % 16 == 0
    if mis == "loc":
        assert dev["loc"].data_ptr() % 8 == 4 and ldt == torch.float32      # 4-byte but not 8-byte aligned
    return dev["value"], shapes.cuda(), lsi.cuda(), dev["loc"], dev["aw"], dev["go"]


def oracle_results(oracle, case, backward=True):
    value, shapes, lsi, loc, aw, go = case
    out = oracle.msda_forward(value.double(), shapes, lsi, loc.double(), aw.double())
    if not backward:
        return out
    return (out, *oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double()))


def assert_exact(got, ref64, dt, what):
    """`got` is the fp64 reference rounded once to `dt`, and finite."""
    assert got.dtype == dt and got.shape == ref64.shape, what
    got = got.cpu()
    assert torch.isfinite(got).all(), what
    want = ref64.to(dt)
    if not torch.equal(got, want):
        bad = got != want
        i = bad.view(-1).nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} elements differ from the reference; first at flat "
                             f"index {i}: {got.view(-1)[i].item()!r} vs {want.view(-1)[i].item()!r}")


def run_exact(msda, oracle, case, dt, mis=None):
    """Forward and backward of an exact case against the fp64 oracle: all four results bit for bit."""
    v, shapes, lsi, loc, aw, go = device_operands(case, dt, mis)
    ref_out, ref_gv, ref_gl, ref_ga = oracle_results(oracle, case)
    out = msda.ms_deform_attn_forward(v, shapes, lsi, loc, aw, 64)
    assert_exact(out, ref_out, dt, "output")
    gv, gl, ga = msda.ms_deform_attn_backward(v, shapes, lsi, loc, aw, go, 64)
    gdt = torch.float64 if dt == torch.float64 else torch.float32
    assert_exact(gv, ref_gv, dt, "grad_value")
    assert_exact(gl, ref_gl, gdt, "grad_loc")
    assert_exact(ga, ref_ga, gdt, "grad_aw")


# ---- 1. the route matrix, 3. level_start_index with gaps and in reverse order -------------------------------------
@pytest.mark.parametrize("name,layout", [(n, "packed") for n in C.ROUTES] + [(n, "reversed") for n in C.LSI_ROUTES])
def test_route_on_an_exact_case(msda, oracle, dfx_env, name, layout):
    """One row of _msda_cases.ROUTES (the table names the kernels and the input property that selects them): N = 3,
    Lq = 37 (odd N * Lq, query pairs straddling batch elements), an empty level inside every pyramid of 3 and more levels,
    samples exactly on -1, -0.5, 0, size - 1, size - 0.5, size, NaN / inf / overflowing locations mixed with valid ones.
    layout "reversed": the levels back to front in the slab with unused tokens between them."""
    dt, M, D, P, L, mis, narrow, fwd, bwd = C.ROUTES[name]
    if narrow:
        dfx_env("DFX_MSDA_HALF_NARROW", "1")
    run_exact(msda, oracle, C.route_case(name, layout), C.DTYPES[dt], mis)


# ---- 5. collisions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["m8d32-f32", "m8d32-bf16", "generic-f32"])
@pytest.mark.parametrize("name", list(C.COLLISION_SHAPES))
def test_grad_value_under_heavy_collision(msda, oracle, name, route):
    """4096 queries on a (2, 2) / (1, 1) map: every grad_value element is the sum of thousands of atomic adds, all of them
    multiples of 2^-8 with magnitudes summing far below 2^16 - the sum is exact in any order, so one lost or doubled
    update changes the result."""
    dt = torch.bfloat16 if route.endswith("bf16") else torch.float32
    run_exact(msda, oracle, C.collision_case(name), dt, "go" if route.startswith("generic") else None)


# ---- 2. multi-pass grids --------------------------------------------------------------------------------------------
VARIANTS = {"f32": (torch.float32, False), "bf16": (torch.bfloat16, False), "bf16-narrow": (torch.bfloat16, True),
            "f16": (torch.float16, False)}
MULTIPASS = [(N, Lq, L, v) for N, Lq in C.MULTIPASS for L in (1, 4) for v in VARIANTS
             if not (v == "bf16-narrow" and L == 4)]          # L = 4 is the narrow gather anyway


@functools.lru_cache(maxsize=1)
def _multipass_exact(N, Lq, L):
    from oracle import msda_oracle
    case = C.multipass_exact_case(N, Lq, L)
    return case, oracle_results(msda_oracle, case, backward=False)


@functools.lru_cache(maxsize=1)
def _multipass_random(N, Lq, L, dt):
    from oracle import msda_oracle
    shp = C.MULTIPASS_RANDOM_SHAPES[L]
    if dt == torch.float32:
        args = rand_case(300 + Lq + L, N, 8, 32, Lq, 4, shp, lo=-0.1, hi=1.1)
    else:
        args = half_case(300 + Lq + L, dt, N, 8, 32, Lq, 4, shp, -0.1, 1.1)
    value, shapes, lsi, loc, aw = args
    return args, msda_oracle.msda_forward(value.double(), shapes, lsi, loc.double(), aw.double())


def in_chunks(fn, N, Lq, value, *per_query):
    """fn(value[b:b+1], operands[b:b+1, q0:q1] ...) over calls of one batch element and fewer than 32768 queries each - they
    run a single pass - put together as one [N, Lq, ...] result."""
    rows = []
    for b in range(N):
        parts = [fn(value[b:b + 1], *[t[b:b + 1, q0:q1].contiguous() for t in per_query])
                 for cb, q0, q1 in C.chunks(N, Lq) if cb == b]
        rows.append(torch.cat(parts, 1))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("N,Lq,L,variant", MULTIPASS, ids=[f"{n * q}-l{l}-{v}" for n, q, l, v in MULTIPASS])
def test_multi_pass_grid(msda, oracle, dfx_env, N, Lq, L, variant):
    """N * Lq on both sides of every step of `iters` (forward_impl: 2, 4, 8 passes from 32768, 65536, 131072 queries).
    Exact inputs: bit for bit the fp64 oracle.  Random inputs: the suite's existing criteria.  Both: the same bits as the
    call cut into single-pass calls (per query the arithmetic is the same)."""
    dt, narrow = VARIANTS[variant]
    if narrow:
        dfx_env("DFX_MSDA_HALF_NARROW", "1")

    case, ref = _multipass_exact(N, Lq, L)
    def forward_on(shapes, lsi):
        return lambda vv, ll, aa: msda.ms_deform_attn_forward(vv, shapes, lsi, ll, aa, 64)

    v, shapes, lsi, loc, aw, _ = device_operands(case, dt)
    fwd = forward_on(shapes, lsi)
    out = fwd(v, loc, aw)
    assert_exact(out, ref, dt, "output")
    assert torch.equal(out, in_chunks(fwd, N, Lq, v, loc, aw))
    del v, loc, aw, out

    args, ref = _multipass_random(N, Lq, L, dt)
    v, shapes, lsi, loc, aw = [t.cuda() for t in args]
    fwd = forward_on(shapes, lsi)
    out = fwd(v, loc, aw)
    if dt == torch.float32:
        assert torch.allclose(out.cpu().double(), ref, **F32_TOL)
    else:
        assert_forward(out, ref, dt)
    assert torch.equal(out, in_chunks(fwd, N, Lq, v, loc, aw))


@pytest.mark.parametrize("L,ref_dim", [(1, 2), (1, 4), (4, 2), (4, 4)])
def test_fused_front_end_multi_pass(msda, oracle, L, ref_dim):
    """ops.msda_fused_forward (csrc/msda_fused.hip, the same `iters` rule) at N * Lq = 131085, N = 3: the oracle at the
    tolerance of test_fused_front_end_matches_unfused, and the same bits as itself in single-pass calls."""
    from dfx import ops
    N, Lq = C.MULTIPASS[-1]
    M, D, P = 8, 32, 4
    g = torch.Generator().manual_seed(61 + L + ref_dim)
    shapes = torch.as_tensor(C.MULTIPASS_RANDOM_SHAPES[L], dtype=torch.long)
    lsi = C.lsi_of(shapes)
    S = int(shapes.prod(1).sum())
    value = torch.randn(N, S, M, D, generator=g)
    qproj = torch.randn(N, Lq, 3 * M * L * P, generator=g) * 2.0
    ref = torch.rand(N, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] *= 0.3
    off = qproj[..., : 2 * M * L * P].reshape(N, Lq, M, L, P, 2)
    aw = torch.softmax(qproj[..., 2 * M * L * P:].reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    if ref_dim == 2:
        norm = torch.stack([shapes[..., 1], shapes[..., 0]], -1)
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
    expect = oracle.msda_forward(value, shapes, lsi, loc.contiguous(), aw)
    shapes_d, lsi_d = shapes.cuda(), lsi.cuda()
    fused = lambda vv, rr, qq: ops.msda_fused_forward(vv, shapes_d, lsi_d, rr, qq, L, P)
    v, r, q = value.cuda(), ref.cuda(), qproj.cuda()
    got = fused(v, r, q)
    assert torch.allclose(got.cpu(), expect, rtol=1e-4, atol=5e-5)
    assert torch.equal(got, in_chunks(fused, N, Lq, v, r, q))


# ---- 4. offsets at the 32-bit bound -----------------------------------------------------------------------------
def bound_value(N, S, dt):
    """_msda_cases.bound_value_at over [N, S, 8, 32] on the device, a range of tokens at a time."""
    value = torch.empty(N, S, 8, 32, dtype=dt, device="cuda")
    m = torch.arange(8, device="cuda", dtype=torch.int32).view(1, 8, 1)
    d = torch.arange(32, device="cuda", dtype=torch.int32).view(1, 1, 32)
    step = 1 << 18
    for n in range(N):
        for s0 in range(0, S, step):
            s = torch.arange(s0, min(s0 + step, S), device="cuda", dtype=torch.int32).view(-1, 1, 1)
            k = (7 * s + 3 * m + d + 5 * n) % 17 - 8          # 7 * 2^22 fits int32
            value[n, s0:s0 + s.shape[0]] = (k.float() / 8).to(dt)
    return value


def check_bound_value(value):
    N, S = value.shape[:2]
    for n, s in ((0, 0), (N - 1, S - 1), (N - 1, (1 << 21) + 12345)):
        want = C.bound_value_at(torch.tensor(n), torch.tensor(s), torch.arange(8).view(8, 1), torch.arange(32))
        assert torch.equal(value[n, s].cpu().double(), want)


BOUND_LQ = 301     # odd: with N = 2 the pair (Lq - 1 of element 0, 0 of element 1) straddles, both reading last tokens


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_forward_at_the_32_bit_offset_bound(msda, dfx_env, dt):
    """S = 2^22 - 1 tokens (M = 8, D = 32): the largest slab the taps kernels' unsigned byte offsets take - the fp32 slab
    is 2^32 - 1024 bytes, and for a 2-byte value a tap offset plus the second batch element's slab (wide gather) reaches
    the same sum.  The level (1024, 2048) is the tail of the slab and the samples aim at its first and last rows.  With
    S = 2^22 the fast path declines and the generic kernel has to give the same answer.  The value map is a closed form
    generated on the device; the reference evaluates it in fp64 at the sampled corners (_msda_cases.bilinear_reference)."""
    dtype = C.DTYPES[dt]
    N = 1 if dt == "f32" else 2
    for S in (C.BOUND_S, C.BOUND_S + 1):
        fast = S * 1024 < 2 ** 32
        assert fast == (S == C.BOUND_S)
        shapes, lsi, loc, aw, go = C.bound_case(40 + N, N, BOUND_LQ, S)
        ref = C.bilinear_reference(C.bound_value_at, shapes, lsi, loc, aw, go, 8, 32)[0]
        value = bound_value(N, S, dtype)
        check_bound_value(value)
        ops_d = [t.cuda() for t in (shapes, lsi, loc, aw)]
        for narrow in ((False, True) if fast and dt != "f32" else (False,)):
            dfx_env("DFX_MSDA_HALF_NARROW", "1" if narrow else None)
            out = msda.ms_deform_attn_forward(value, *ops_d, 64)
            assert_exact(out, ref, dtype, f"output, S = {S}, narrow = {narrow}")
        del value, out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_at_the_32_bit_offset_bound(msda, dt):
    """msda_bwd_m8d32 on the same slab (its corner offset is an int of (y * W + x) * 256, the level start a long): grad_loc
    and grad_aw exact, grad_value exact on the touched tokens and zero everywhere else."""
    dtype, N, S = C.DTYPES[dt], 1, C.BOUND_S
    shapes, lsi, loc, aw, go = C.bound_case(50, N, BOUND_LQ, S)
    _, ref_gl, ref_ga, (keys, rows) = C.bilinear_reference(C.bound_value_at, shapes, lsi, loc, aw, go, 8, 32)
    value = bound_value(N, S, dtype)
    gv, gl, ga = msda.ms_deform_attn_backward(value, *[t.cuda() for t in (shapes, lsi, loc, aw)], go.to(dtype).cuda(), 64)
    del value
    assert_exact(gl, ref_gl, torch.float32, "grad_loc")
    assert_exact(ga, ref_ga, torch.float32, "grad_aw")
    assert gv.dtype == dtype and gv.shape == (N, S, 8, 32)
    assert keys[:, 1].max().item() == S - 1 and torch.count_nonzero(rows) > 0
    touched = gv[keys[:, 0].cuda(), keys[:, 1].cuda()]
    assert_exact(touched, rows, dtype, "grad_value on the touched tokens")
    assert torch.count_nonzero(gv).item() == torch.count_nonzero(rows.to(dtype)).item()     # nothing anywhere else
    del gv
    torch.cuda.empty_cache()
