"""CPU: the input builders of tests/_msda_cases.py, checked against the oracle alone.

For every case tests/test_msda_routes_gpu.py uses:
  * the fp32 oracle equals the fp64 oracle bit for bit on the forward and on all three gradients (so the case is exact in
    fp32 whatever the order of the sum: a GPU kernel may be held to torch.equal);
  * the measured sums of magnitudes (fp64 oracle on |value|, |aw|, |grad_out|) are inside the bit budget;
  * every result is finite although the locations hold NaN, +-inf and products that overflow;
  * at least half of the forward outputs are non-zero (a condition on the inputs: the case is not vacuous);
  * the samples really sit on the lines the case is built for.
"""
import pytest
import torch

from tests import _msda_cases as C


def _f64(case):
    value, shapes, lsi, loc, aw, go = case
    return value.double(), shapes, lsi, loc.double(), aw.double(), go.double()


def check_exact(oracle, case, backward=True):
    value, shapes, lsi, loc, aw, go = case
    v64, _, _, l64, a64, g64 = _f64(case)
    f32 = oracle.msda_forward(value, shapes, lsi, loc, aw)
    f64 = oracle.msda_forward(v64, shapes, lsi, l64, a64)
    assert torch.isfinite(f64).all()
    assert torch.equal(f32.double(), f64)
    share = (f64 != 0).double().mean().item()
    assert share >= 0.5, f"only {share:.3f} of the forward outputs are non-zero"
    # measured budget: terms are multiples of 2^-9, the sum of their magnitudes stays below 2^15
    mag = oracle.msda_forward(v64.abs(), shapes, lsi, l64, a64.abs())
    assert mag.max().item() < 2 ** (24 - 9)
    # exact in the 2-byte dtypes as well: the inputs survive the cast
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(value.to(dt).float(), value) and torch.equal(go.to(dt).float(), go)
    if not backward:
        return
    b32 = oracle.msda_backward(value, shapes, lsi, loc, aw, go)
    b64 = oracle.msda_backward(v64, shapes, lsi, l64, a64, g64)
    for name, a, b in zip(("grad_value", "grad_loc", "grad_aw"), b32, b64):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a.double(), b), name
        assert torch.count_nonzero(b) > 0, name
    gv_mag = oracle.msda_backward(v64.abs(), shapes, lsi, l64, a64.abs(), g64.abs())[0]
    assert gv_mag.max().item() < 2 ** (24 - 8)


def pixel_coordinates(case, l):
    value, shapes, lsi, loc, aw, go = case
    H, W = int(shapes[l, 0]), int(shapes[l, 1])
    return loc[:, :, :, l, :, 1].double() * H - 0.5, loc[:, :, :, l, :, 0].double() * W - 0.5, H, W


@pytest.mark.parametrize("name", list(C.ROUTES))
def test_route_cases_are_exact(oracle, name):
    case = C.route_case(name)
    dt, M, D, P, L, mis, narrow, fwd, bwd = C.ROUTES[name]
    value, shapes, lsi, loc, aw, go = case
    assert value.shape[2:] == (M, D) and loc.shape == (C.ROUTE_N, C.ROUTE_LQ, M, L, P, 2)
    assert (C.ROUTE_N * C.ROUTE_LQ) % 2 == 1 and C.ROUTE_LQ % 2 == 1
    if L >= 3:
        assert int(shapes[1:-1].prod(1).min()) == 0, "no empty level in the middle of the pyramid"
    check_exact(oracle, case)


@pytest.mark.parametrize("name", C.LSI_ROUTES)
def test_reversed_layout_cases_are_exact(oracle, name):
    case = C.route_case(name, "reversed")
    value, shapes, lsi, loc, aw, go = case
    assert not torch.equal(lsi, C.lsi_of(shapes))
    spans = sorted((int(s), int(s) + int(h * w)) for s, (h, w) in zip(lsi, shapes))
    assert spans[0][0] > 0 and spans[-1][1] < value.shape[1]
    assert all(a[1] < b[0] or a[0] == a[1] for a, b in zip(spans, spans[1:])), "levels overlap or touch"
    if shapes.shape[0] > 1:
        filled = [int(s) for s, (h, w) in zip(lsi, shapes) if h * w]
        assert filled == sorted(filled, reverse=True), "levels are not back to front"
    check_exact(oracle, case)


@pytest.mark.parametrize("name", list(C.COLLISION_SHAPES))
def test_collision_cases_are_exact(oracle, name):
    case = C.collision_case(name)
    check_exact(oracle, case)
    value, shapes, lsi, loc, aw, go = case
    # every grad_value element is hit, each by thousands of samples
    py, px, H, W = pixel_coordinates(case, 0)
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    assert inside.sum().item() / (H * W) > 1000
    gv = oracle.msda_backward(*_f64(case))[0]
    assert torch.count_nonzero(gv) >= 0.99 * gv.numel()


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("N,Lq", C.MULTIPASS)
def test_multipass_cases_are_exact(oracle, N, Lq, L):
    check_exact(oracle, C.multipass_exact_case(N, Lq, L), backward=False)
    for b, q0, q1 in C.chunks(N, Lq):
        assert 0 < q1 - q0 < 32768
    assert sum(q1 - q0 for _, q0, q1 in C.chunks(N, Lq)) == N * Lq


def test_exact_cases_sit_on_the_lines(oracle):
    """The pixel coordinates -1, -0.5, 0, size - 1, size - 0.5 and size all occur on both axes, in-range and skipped
    samples share queries, and the special values are all there."""
    case = C.route_case("f32-taps-l3")
    value, shapes, lsi, loc, aw, go = case
    for l in (0, 2):
        py, px, H, W = pixel_coordinates(case, l)
        for c, size in ((py, H), (px, W)):
            fin = c[torch.isfinite(c)]
            for want in (-1.5, -1.0, -0.5, 0.0, 0.5, size - 1.0, size - 0.5, float(size), size + 0.5, size + 1.0):
                assert (fin == want).any(), (l, size, want)
        inside = (py > -1) & (py < H) & (px > -1) & (px < W)
        per_query = inside.sum(-1)                       # over the points of one (query, head)
        mixed = (per_query > 0) & (per_query < inside.shape[-1])
        assert mixed.double().mean().item() > 0.3
    flat = loc.view(-1)
    assert torch.isnan(flat).any() and (flat == float("inf")).any() and (flat == float("-inf")).any()
    for s in (1e30, -1e30, 3e38, 1e-45):
        assert (flat == torch.tensor(s)).any(), s
    assert torch.isinf(torch.tensor(3e38) * 2)
    # an empty level in the middle holds finite locations and specials alike
    mid = loc[:, :, :, 1]
    assert torch.isfinite(mid).any() and not torch.isfinite(mid).all()


def test_plain_torch_reference_matches_the_oracle(oracle):
    """bilinear_reference (the reference of the 32-bit-bound tests, where no host array of the value map exists) against
    the oracle on a case whose value map is materialised: the same bits on all four results."""
    for name, layout in (("f32-taps-l3", "reversed"), ("f32-m8d32-p5", "packed"), ("f32-generic-m3d7", "packed")):
        case = C.route_case(name, layout)
        value, shapes, lsi, loc, aw, go = case
        M, D = value.shape[2:]
        v64 = value.double()
        out, gl, ga, (keys, rows) = C.bilinear_reference(lambda n, s, m, d: v64[n, s, m, d], shapes, lsi, loc, aw, go, M, D)
        assert torch.equal(out, oracle.msda_forward(*_f64(case)[:5]))
        gv, rl, ra = oracle.msda_backward(*_f64(case))
        assert torch.equal(gl, rl) and torch.equal(ga, ra)
        dense = torch.zeros_like(gv)
        dense[keys[:, 0], keys[:, 1]] = rows
        assert torch.equal(dense, gv)


@pytest.mark.parametrize("N", [1, 2])
def test_bound_case(oracle, N):
    """The case at the 32-bit offset bound: on a small stand-in geometry the closed-form reference is the oracle's result;
    at the real size the samples reach the first and the last token of the slab and the outputs are mostly non-zero."""
    S, Lq = C.BOUND_S, 301
    shapes, lsi, loc, aw, go = C.bound_case(5, N, Lq, S)
    assert S * 1024 < 2 ** 32 <= (S + 1) * 1024
    assert int(lsi[0]) + C.BOUND_H * C.BOUND_W == S
    out, gl, ga, (keys, rows) = C.bilinear_reference(C.bound_value_at, shapes, lsi, loc, aw, go, 8, 32)
    assert torch.isfinite(out).all() and (out != 0).double().mean().item() >= 0.5
    for n in range(N):
        toks = keys[keys[:, 0] == n, 1]
        assert toks.min().item() == int(lsi[0]) and toks.max().item() == S - 1
    # queries 0 and Lq - 1 (the two sides of a pair that straddles batch elements) read the last token
    py, px = loc[..., 1].double() * C.BOUND_H - 0.5, loc[..., 0].double() * C.BOUND_W - 0.5
    for q in (0, Lq - 1):
        assert (py[:, q, :, 0, 0] == C.BOUND_H - 1).all() and (px[:, q, :, 0, 0] == C.BOUND_W - 1).all()
    # materialised on a geometry the oracle can hold: the last 4 rows of the level as a level of their own
    rows_kept = 4
    small = torch.as_tensor([(rows_kept, C.BOUND_W)], dtype=torch.long)
    first = S - rows_kept * C.BOUND_W
    s_i = torch.arange(first, S).view(1, -1, 1, 1)
    value = C.bound_value_at(torch.arange(N).view(-1, 1, 1, 1), s_i, torch.arange(8).view(1, 1, -1, 1), torch.arange(32))
    assert value.shape == (N, rows_kept * C.BOUND_W, 8, 32) and value.abs().max() <= 1
    loc_s = loc.clone()
    py_s = py - (C.BOUND_H - rows_kept)                                  # the same samples seen from the small level
    loc_s[..., 1] = ((py_s + 0.5) / rows_kept).float()
    got = C.bilinear_reference(lambda n, s, m, d: C.bound_value_at(n, s + first, m, d), small, torch.zeros(1, dtype=torch.long),
                               loc_s, aw, go, 8, 32)[0]
    want = oracle.msda_forward(value, small, torch.zeros(1, dtype=torch.long), loc_s.double(), aw.double())
    assert torch.equal(got, want)
