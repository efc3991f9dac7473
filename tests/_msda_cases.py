"""Input builders of the MSDA operator tests (tests/test_msda_exact_cases.py on the CPU,
tests/test_msda_routes_gpu.py on the GPU).  Plain helpers, no fixtures.

The exact ("dyadic") family
---------------------------
``exact_case`` builds inputs for which every product and every partial sum of the operator is exactly
representable in fp32, so the result does not depend on the order of the sum or on FMA contraction: a
kernel has to equal the fp64 oracle bit for bit (rounded once to the value dtype for bf16 / fp16).

  * every non-empty level has power-of-two sides (H, W);
  * pixel coordinates are multiples of 1/2 from -1.5 to size + 1, locations (px + 0.5) / size: the
    location, loc * size - 0.5 (with or without FMA) and the bilinear fractions {0, 1/2} are exact, and the
    samples sit exactly on the skip-rule bounds (-1, size), on grid lines (integers), on the border cells
    (-0.5, size - 0.5) and in between;
  * values are k/8 with |k| <= 8 (exact in bf16 and fp16 as well), attention weights k/16 with |k| <= 6,
    grad_out k/4 with |k| <= 4;
  * some location components are then overwritten with NaN, +-inf, +-1e30, 3e38 (its product with a side
    >= 2 overflows fp32), 1e-45 (a denormal: 1e-45 * size - 0.5 is -0.5 whether or not it is flushed) and
    -0.0.  Empty levels (H or W == 0) get arbitrary finite locations plus the same specials.

Bit budget (``assert_budget``): all terms of a sum are multiples of 2^-q and the sum of their magnitudes is
below 2^(24-q), so every partial sum in any order is a multiple of 2^-q below 2^24 * 2^-q: exact.

    output       corner weight (2^-2) x attention weight (2^-4) x value (2^-3): q = 9,
                 sum |terms| <= L * P * max|aw| * max|value|     (the 4 corner weights of a sample sum to <= 1)
    grad_value   corner weight (2^-2) x grad_out (2^-2) x attention weight (2^-4): q = 8,
                 sum |terms| into one element <= Lq * L * P * max|aw| * max|grad_out|
    grad_aw      grad_out (2^-2) x corner weight (2^-2) x value (2^-3): q = 7,
                 sum |terms| <= D * max|grad_out| * max|value|
    grad_loc     size x fraction (2^-1) x value (2^-3) x grad_out x attention weight (2^-6): multiples of
                 size * 2^-10 with size a power of two, sum |terms| <= size * D * 2 max|value| max|grad_out| max|aw|,
                 so D * 2 * max|value| * max|grad_out| * max|aw| < 2^14 is enough for any size

These bounds come from the inputs alone.  tests/test_msda_exact_cases.py additionally measures the sums of
magnitudes with the fp64 oracle on |value|, |aw|, |grad_out| and checks fp32 oracle == fp64 oracle.
"""
import math

import torch

SPECIALS = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 3e38, 1e-45, -0.0]
DTYPES = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16, "f16": torch.float16}


def lsi_of(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def reversed_layout(shapes, gap=3):
    """level_start_index that is NOT the running sum: the levels lie back to front in the slab, with `gap`
    unused tokens in front of each of them.  -> (lsi, S)"""
    sizes = shapes.prod(1).tolist()
    lsi, at = [0] * len(sizes), 0
    for l in reversed(range(len(sizes))):
        at += gap
        lsi[l] = at
        at += sizes[l]
    return torch.as_tensor(lsi, dtype=torch.long), at + gap


def _is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def assert_budget(case, backward=True):
    """The bit budget of the module docstring, from the inputs alone (backward=False: a forward-only case)."""
    value, shapes, lsi, loc, aw, go = case
    N, S, M, D = value.shape
    L, Lq, P = shapes.shape[0], loc.shape[1], loc.shape[4]
    for h, w in shapes.tolist():
        assert h == 0 or w == 0 or (_is_pow2(h) and _is_pow2(w)), "non-empty levels need power-of-two sides"
    for l, (h, w) in enumerate(shapes.tolist()):      # every level lies inside the slab
        assert 0 <= int(lsi[l]) and int(lsi[l]) + h * w <= S
    for t, q in ((value, 3), (aw, 4), (go, 2)):
        assert torch.equal(t * 2 ** q, (t * 2 ** q).round()), "inputs must be multiples of 2^-q"
    v, a, g = value.abs().max().item(), aw.abs().max().item(), go.abs().max().item()
    assert L * P * a * v < 2 ** (24 - 9)                 # output
    assert not backward or Lq * L * P * a * g < 2 ** (24 - 8)    # grad_value
    assert D * g * v < 2 ** (24 - 7)                     # grad_aw
    assert D * 2 * v * g * a < 2 ** (24 - 10)            # grad_loc / size
    fin = loc[torch.isfinite(loc)]
    for l, (h, w) in enumerate(shapes.tolist()):         # non-special pixel coordinates are multiples of 1/2
        for k, size in ((0, w), (1, h)):
            if h and w:
                c = loc[:, :, :, l, :, k]
                c = c[torch.isfinite(c) & (c.abs() < 1e4) & (c.abs() > 1e-30)]
                assert torch.equal(c * (2 * size), (c * (2 * size)).round())
    assert fin.numel() < loc.numel(), "the case holds no NaN / inf location"


def exact_case(seed, N, M, D, Lq, P, shape_list, layout="packed", n_special=200, backward=True):
    """-> (value, shapes, lsi, loc, aw, grad_out), fp32 on the CPU; exact in bf16 / fp16 as well (cast value and
    grad_out with .to(dtype), the locations and weights stay fp32 there).  layout: "packed" (running-sum
    level_start_index) or "reversed" (reversed_layout); backward=False: used by forward tests only (no grad_value budget)."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(shape_list, dtype=torch.long).view(-1, 2)
    L = shapes.shape[0]
    if layout == "packed":
        lsi, S = lsi_of(shapes), int(shapes.prod(1).sum())
    else:
        lsi, S = reversed_layout(shapes)
    loc = torch.empty(N, Lq, M, L, P, 2)
    for l in range(L):
        H, W = int(shapes[l, 0]), int(shapes[l, 1])
        for k, size in ((0, W), (1, H)):
            shape = (N, Lq, M, P)
            if H == 0 or W == 0:        # empty level: nothing may be read, whatever the location says
                loc[:, :, :, l, :, k] = torch.randn(shape, generator=g) * 3
                continue
            # half of the samples anywhere in [-1.5, size + 1], half in [-1, size] (both bounds are skipped)
            wide = torch.randint(-3, 2 * size + 3, shape, generator=g)
            near = torch.randint(-2, 2 * size + 1, shape, generator=g)
            pick = torch.rand(shape, generator=g) < 0.5
            px = torch.where(pick, wide, near).float() / 2
            loc[:, :, :, l, :, k] = (px + 0.5) / size
    flat = loc.view(-1)
    n_special = min(n_special, flat.numel() // 8)
    pos = torch.randperm(flat.numel(), generator=g)[:n_special]
    flat[pos] = torch.tensor(SPECIALS).repeat(n_special // len(SPECIALS) + 1)[:n_special]
    value = torch.randint(-8, 9, (N, S, M, D), generator=g).float() / 8
    k = torch.randint(-2, 7, (N, Lq, M, L, P), generator=g)
    aw = torch.where(k == 0, torch.full_like(k, 3), k).float() / 16     # mostly positive, a few negative, none zero
    go = torch.randint(-4, 5, (N, Lq, M * D), generator=g).float() / 4
    case = (value, shapes, lsi, loc, aw, go)
    assert_budget(case, backward)
    return case


# ---- geometries ---------------------------------------------------------------------------------------------
# Every pyramid with L >= 3 holds an empty level in the middle; N = 3 with an odd Lq gives an odd N * Lq (a half-filled
# last wave) and query pairs that straddle two batch elements.
PYRAMID = {
    1: [(4, 8)],
    2: [(0, 5), (4, 8)],
    3: [(4, 8), (0, 4), (2, 2)],
    4: [(8, 4), (3, 0), (2, 2), (1, 2)],
    5: [(4, 8), (0, 4), (2, 2), (1, 1), (2, 4)],
    6: [(4, 8), (0, 4), (2, 2), (0, 0), (1, 1), (2, 4)],
}
ROUTE_N, ROUTE_LQ = 3, 37

# The route table.  Kernel selection as csrc/msda_forward.hip:forward_impl and csrc/msda_backward.hip:backward_impl
# decide it, from the properties on the right:
#   fast          M == 8, D == 32, value (and out) 16-byte aligned, S * 1024 < 2^32, fp32 / bf16 / fp16
#   taps          fast, P == 4, L <= 4, loc 8-byte aligned        -> msda_fwd_taps<L, V, wide>
#                 wide: 2-byte V, L == 1, DFX_MSDA_HALF_NARROW unset
#   m8d32         fast, fp32, not taps                              -> msda_fwd_m8d32
#   otherwise                                                       -> msda_fwd_generic<V>
#   backward      M == 8, D == 32, value and grad_out 16-byte aligned, not fp64 -> msda_bwd_m8d32<V>, else msda_bwd_generic<V>
# Each row: id -> (dtype, M, D, P, L, misaligned operand or None, DFX_MSDA_HALF_NARROW, forward kernel, backward kernel)
_V = {"f32": "float", "f64": "double", "bf16": "__hip_bfloat16", "f16": "_Float16"}


def _routes():
    rows = {}

    def add(name, dt, M, D, P, L, mis, narrow, fwd, bwd):
        rows[name] = (dt, M, D, P, L, mis, narrow, fwd, bwd)

    for L in (1, 2, 3, 4):
        add(f"f32-taps-l{L}", "f32", 8, 32, 4, L, None, False, f"msda_fwd_taps<{L}, float, false>", "msda_bwd_m8d32<float>")
    for dt in ("bf16", "f16"):
        v = _V[dt]
        add(f"{dt}-taps-wide", dt, 8, 32, 4, 1, None, False, f"msda_fwd_taps<1, {v}, true>", f"msda_bwd_m8d32<{v}>")
        for L in (1, 2, 3, 4):
            add(f"{dt}-taps-narrow-l{L}", dt, 8, 32, 4, L, None, L == 1, f"msda_fwd_taps<{L}, {v}, false>",
                f"msda_bwd_m8d32<{v}>")
    for P in (3, 5):
        add(f"f32-m8d32-p{P}", "f32", 8, 32, P, 3, None, False, "msda_fwd_m8d32", "msda_bwd_m8d32<float>")
    for L in (5, 6):
        add(f"f32-m8d32-l{L}", "f32", 8, 32, 4, L, None, False, "msda_fwd_m8d32", "msda_bwd_m8d32<float>")
    add("f32-m8d32-loc4", "f32", 8, 32, 4, 3, "loc", False, "msda_fwd_m8d32", "msda_bwd_m8d32<float>")
    add("f32-m8d32-loc4-l1", "f32", 8, 32, 4, 1, "loc", False, "msda_fwd_m8d32", "msda_bwd_m8d32<float>")
    for dt in ("f32", "f64", "bf16", "f16"):
        v = _V[dt]
        gen = (f"msda_fwd_generic<{v}>", f"msda_bwd_generic<{v}>")
        add(f"{dt}-generic-m3d7", dt, 3, 7, 4, 3, None, False, *gen)
        add(f"{dt}-generic-m4d16", dt, 4, 16, 2, 3, None, False, *gen)
        add(f"{dt}-generic-m8d32-value", dt, 8, 32, 4, 3, "value", False, *gen)
        add(f"{dt}-generic-m8d32-value-l1", dt, 8, 32, 4, 1, "value", False, *gen)
        # an unaligned grad_out alone: the forward keeps its fast route, the backward takes the generic kernel
        fwd = {"f32": "msda_fwd_taps<3, float, false>", "f64": gen[0]}.get(dt, f"msda_fwd_taps<3, {v}, false>")
        add(f"{dt}-bwd-generic-m8d32-grad-out", dt, 8, 32, 4, 3, "go", False, fwd, gen[1])
    add("f64-generic-m8d32", "f64", 8, 32, 4, 3, None, False, "msda_fwd_generic<double>", "msda_bwd_generic<double>")
    for dt in ("bf16", "f16"):
        v = _V[dt]
        add(f"{dt}-generic-p3", dt, 8, 32, 3, 3, None, False, f"msda_fwd_generic<{v}>", f"msda_bwd_m8d32<{v}>")
        add(f"{dt}-generic-l5", dt, 8, 32, 4, 5, None, False, f"msda_fwd_generic<{v}>", f"msda_bwd_m8d32<{v}>")
        add(f"{dt}-generic-loc4", dt, 8, 32, 4, 1, "loc", False, f"msda_fwd_generic<{v}>", f"msda_bwd_m8d32<{v}>")
    return rows


ROUTES = _routes()


def route_case(name, layout="packed"):
    """The exact case of one ROUTES row (fp32 tensors; the caller casts and misaligns)."""
    dt, M, D, P, L, mis, narrow, fwd, bwd = ROUTES[name]
    seed = 1000 + sorted(ROUTES).index(name)
    return exact_case(seed, ROUTE_N, M, D, ROUTE_LQ, P, PYRAMID[L], layout=layout)


# level_start_index with gaps, levels back to front: a taps route, msda_fwd_m8d32, both generic kernels, both backward kernels
LSI_ROUTES = ["f32-taps-l4", "bf16-taps-wide", "f16-taps-narrow-l3", "f32-m8d32-p5", "f32-generic-m3d7", "bf16-generic-l5",
              "f32-bwd-generic-m8d32-grad-out"]

# Multi-pass grids: (N, Lq) with N * Lq = 32767, 32768, 32769, 65536 + 9, 131072 + 13 - on both sides of every step of
# `iters` (1 below 32768, 2 from 32768, 4 from 65536, 8 from 131072); all but one with an odd Lq, so that query pairs
# straddle batch elements in the later passes, and the last with N = 3.
MULTIPASS = [(7, 4681), (2, 16384), (3, 10923), (5, 13109), (3, 43695)]
MULTIPASS_EXACT_SHAPES = {1: [(8, 16)], 4: [(8, 16), (0, 4), (4, 4), (2, 1)]}
MULTIPASS_RANDOM_SHAPES = {1: [(20, 31)], 4: [(16, 20), (8, 10), (4, 5), (2, 3)]}
assert [n * q for n, q in MULTIPASS] == [32767, 32768, 32769, 65536 + 9, 131072 + 13]


def multipass_exact_case(N, Lq, L):
    return exact_case(7000 + Lq + L, N, 8, 32, Lq, 4, MULTIPASS_EXACT_SHAPES[L], n_special=400, backward=False)


def chunks(N, Lq, limit=32000):
    """(batch element, first query, end query) ranges of at most `limit` (< 32768) queries: calls that run one pass."""
    per = math.ceil(Lq / math.ceil(Lq / limit))
    return [(b, q0, min(q0 + per, Lq)) for b in range(N) for q0 in range(0, Lq, per)]


# Collisions: every grad_value element of a (2, 2) or (1, 1) map receives thousands of atomic adds
COLLISION_SHAPES = {"2x2": [(2, 2)], "1x1": [(1, 1)]}
COLLISION_LQ = 4096


def collision_case(name):
    return exact_case(9000 + len(name) + COLLISION_SHAPES[name][0][0], 1, 8, 32, COLLISION_LQ, 4, COLLISION_SHAPES[name],
                      n_special=64)


# ---- 32-bit offsets at their bound ------------------------------------------------------------------------------
# One level (1024, 2048) = 2^21 tokens as the tail of a slab of S tokens, M = 8, D = 32.  With S = 2^22 - 1 the fp32 slab is
# 2^32 - 1024 bytes: the fast path's condition S * 1024 < 2^32 just holds and the last token of the level ends at byte
# S * 1024 - 1; with S = 2^22 the fast path has to decline.  The value map is a closed form in (batch element, token, head,
# channel), generated on the device and evaluated by the reference at the sampled corners only.
BOUND_H, BOUND_W = 1024, 2048
BOUND_S = (1 << 22) - 1


def bound_value_at(n, s, m, d):
    """Closed-form value map: k/8, |k| <= 8.  Integer tensors (or ints) in, float64 out."""
    return (((7 * s + 3 * m + d + 5 * n) % 17) - 8).to(torch.float64) / 8


def bound_case(seed, N, Lq, S):
    """-> (shapes, lsi, loc, aw, grad_out): exact inputs whose samples aim at the first and the last rows of the
    level; queries 0 and Lq - 1 of every batch element (the two sides of a straddling pair) hit its last token."""
    g = torch.Generator().manual_seed(seed)
    H, W, M, P = BOUND_H, BOUND_W, 8, 4
    shapes = torch.as_tensor([(H, W)], dtype=torch.long)
    lsi = torch.as_tensor([S - H * W], dtype=torch.long)
    assert int(lsi[0]) >= 0
    shape = (N, Lq, M, 1, P)
    top = torch.randint(-3, 6, shape, generator=g)                     # py in [-1.5, 2.5]
    bot = torch.randint(2 * H - 6, 2 * H + 3, shape, generator=g)      # py in [H - 3, H + 1]
    py = torch.where(torch.rand(shape, generator=g) < 0.5, top, bot).float() / 2
    xs = torch.cat([torch.arange(-3, 6), torch.arange(2 * W - 6, 2 * W + 3), torch.arange(W - 4, W + 4)])
    px = xs[torch.randint(0, len(xs), shape, generator=g)].float() / 2
    for q in (0, Lq - 1):
        py[:, q, :, 0, 0], px[:, q, :, 0, 0] = H - 1, W - 1            # the last token alone
        py[:, q, :, 0, 1], px[:, q, :, 0, 1] = H - 1.5, W - 1.5        # the last 2 x 2 tokens
        py[:, q, :, 0, 2], px[:, q, :, 0, 2] = H - 0.5, W - 0.5        # half outside: the last token, weight 1/4
    loc = torch.stack([(px + 0.5) / W, (py + 0.5) / H], -1)
    flat = loc.view(-1)
    pos = torch.randperm(flat.numel() - 64 * P * 2, generator=g)[:96] + 32 * P * 2     # (not in query 0 or Lq - 1)
    keep = (pos // (M * P * 2)) % Lq
    pos = pos[(keep != 0) & (keep != Lq - 1)]
    flat[pos] = torch.tensor(SPECIALS).repeat(12)[:pos.numel()]
    k = torch.randint(-2, 7, shape, generator=g)
    aw = torch.where(k == 0, torch.full_like(k, 3), k).float() / 16
    go = torch.randint(-4, 5, (N, Lq, M * 32), generator=g).float() / 4
    # the bit budget of the module docstring with max|value| = 1
    a, gm = aw.abs().max().item(), go.abs().max().item()
    assert P * a < 2 ** 15 and Lq * P * a * gm < 2 ** 16 and 32 * gm < 2 ** 17 and 32 * 2 * gm * a < 2 ** 14
    return shapes, lsi, loc, aw, go


def bilinear_reference(value_at, shapes, lsi, loc, aw, go, M, D):
    """Plain-torch fp64 restatement of the operator for a value map given as a function (n, token, head, channel) -> value,
    evaluated at the sampled corners only.  Follows the definition the oracle restates: pixel = loc * size - 0.5, a sample
    counts when -1 < pixel < size on both axes, corners outside the map read as zero.
    -> out [N, Lq, M*D], grad_loc, grad_aw, and grad_value as (tokens [K] (n * S is not folded in: pairs (n, token)),
    rows [K, M, D]) for the touched tokens only."""
    N, Lq, _, L, P, _ = loc.shape
    loc, aw, go = loc.double(), aw.double(), go.double().view(N, Lq, M, D)
    out = torch.zeros(N, Lq, M, D, dtype=torch.float64)
    gl, ga = torch.zeros_like(loc), torch.zeros_like(aw)
    n_i = torch.arange(N).view(N, 1, 1, 1).expand(N, Lq, M, P)
    m_i = torch.arange(M).view(1, 1, M, 1).expand(N, Lq, M, P)
    d_i = torch.arange(D)
    S_key = 1 << 40                                                      # (n, token) as one integer key
    keys, heads, adds = [], [], []
    for l in range(L):
        H, W, start = int(shapes[l, 0]), int(shapes[l, 1]), int(lsi[l])
        w_im = loc[:, :, :, l, :, 0] * W - 0.5
        h_im = loc[:, :, :, l, :, 1] * H - 0.5
        inr = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)       # NaN compares false
        h_s, w_s = torch.where(inr, h_im, torch.zeros_like(h_im)), torch.where(inr, w_im, torch.zeros_like(w_im))
        h0, w0 = h_s.floor(), w_s.floor()
        lh, lw = h_s - h0, w_s - w0
        a, top = aw[:, :, :, l, :], go[:, :, :, None, :]                # [N,Lq,M,P], [N,Lq,M,1,D]
        val = torch.zeros(N, Lq, M, P, D, dtype=torch.float64)
        g_h, g_w = torch.zeros_like(val), torch.zeros_like(val)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            y, x = (h0 + dy).long(), (w0 + dx).long()
            ok = inr & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
            wy, wx = (lh if dy else 1 - lh), (lw if dx else 1 - lw)
            tok = torch.where(ok, start + y * W + x, torch.zeros_like(y))
            v = value_at(n_i[..., None], tok[..., None], m_i[..., None], d_i) * ok[..., None]
            val += (wy * wx)[..., None] * v
            g_h += ((wx if dy else -wx))[..., None] * v
            g_w += ((wy if dx else -wy))[..., None] * v
            contrib = ((wy * wx * a)[..., None] * top) * ok[..., None]  # into grad_value[n, tok, m, :]
            keys.append(n_i[ok] * S_key + tok[ok])
            heads.append(m_i[ok])
            adds.append(contrib[ok])
        out += (val * a[..., None]).sum(3)
        ga[:, :, :, l, :] = (val * top).sum(-1)
        gl[:, :, :, l, :, 0] = W * (g_w * top).sum(-1) * a
        gl[:, :, :, l, :, 1] = H * (g_h * top).sum(-1) * a
    uniq, inv = torch.unique(torch.cat(keys), return_inverse=True)
    rows = torch.zeros(uniq.numel() * M, D, dtype=torch.float64)
    rows.index_add_(0, inv * M + torch.cat(heads), torch.cat(adds))
    return out.view(N, Lq, M * D), gl, ga, (torch.stack([uniq // S_key, uniq % S_key], 1), rows.view(-1, M, D))
