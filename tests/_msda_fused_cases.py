"""Shared builders of the fused MSDA backward tests: seeded operator cases whose samples stay clear of the bilinear
kinks, the reference statement (torch softmax, the module's location arithmetic, ``ms_deform_attn_core_pytorch``) under
autograd on the CPU, and a closed-form restatement of the backward the kernel implements (csrc/msda_fused_backward.hip).

Bilinear kinks.  The gradient with respect to a location is discontinuous where a pixel coordinate crosses an integer
(and where it crosses -1 or the map size: the in-range verdict).  The operator cases therefore CONSTRUCT their offsets:
target pixel coordinates are drawn in fp64 as integer + fraction with the fraction in [0.05, 0.95] - inside the map, in
the border band (-0.95, -0.05) / (size-0.95, size-0.05) where only some corners exist, and outside (below -1.05, above
size+0.05) - and the offset that produces them is solved from the reference point and rounded to fp32.  Recomputing the
coordinate in fp32 moves it by a few 1e-6 (asserted below 1e-4), four orders below the 0.05 margin, so no element is
excluded; ``make_case`` asserts that the fp32 and fp64 coordinates have the same floor and the same in-range verdict.
"""
import functools

import torch

from models.ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch

M, D, P = 8, 32, 4
LEVELS = {1: [(5, 7)], 2: [(7, 9), (3, 5)], 3: [(6, 4), (3, 5), (2, 3)], 4: [(16, 20), (8, 10), (4, 5), (2, 3)],
          "1x1": [(4, 6), (1, 1)]}
# (levels key, ref_dim, N, Lq, strided rows): every template instance (L = 1..4 x ref_dim 2 / 4), non-square levels, a 1x1
# level, 111 queries (a last workgroup with 3 of its 4 waves), one query, many workgroups (block remap), column slices
OPERATOR_CASES = [
    (1, 2, 3, 37, False), (1, 4, 2, 300, False),
    (2, 2, 2, 1100, False), (2, 4, 3, 37, False),
    (3, 2, 1, 1, False), (3, 4, 3, 37, False),
    (4, 2, 2, 300, False), (4, 4, 2, 1100, False),
    ("1x1", 2, 3, 37, False), (4, 4, 3, 37, True), (2, 2, 3, 37, True),
]
GRADS = ("value", "offsets", "logits", "ref")
MAX_COORD_NOISE = 1e-4


def level_tensors(sizes):
    shapes = torch.as_tensor(sizes, dtype=torch.long)
    areas = shapes[:, 0] * shapes[:, 1]
    return shapes, torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])


def locations(ref, offsets, sizes):
    """The module's location arithmetic (models/ops/modules/ms_deform_attn.py) in the dtype of the arguments:
    ref [N,Lq,L,2|4], offsets [N,Lq,M,L,P,2] -> [N,Lq,M,L,P,2]."""
    if ref.shape[-1] == 2:
        wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=ref.dtype)
        return ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
    return ref[:, :, None, :, None, :2] + offsets / P * ref[:, :, None, :, None, 2:] * 0.5


def pixel_coordinates(ref, offsets, sizes):
    """[N,Lq,M,L,P,2] pixel coordinates (x, y) = location * (W, H) - 0.5 in the dtype of the arguments."""
    wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=ref.dtype)
    return locations(ref, offsets, sizes) * wh[None, None, None, :, None, :] - 0.5


def _draw_pixels(g, shape, size):
    """fp64 coordinates integer + fraction, fraction in [0.05, 0.95]: ~60 % inside the map, ~25 % in the border band,
    ~15 % outside."""
    frac = 0.05 + 0.9 * torch.rand(shape, generator=g, dtype=torch.float64)
    kind = torch.rand(shape, generator=g)
    side = torch.rand(shape, generator=g) < 0.5
    far = torch.randint(0, 2, shape, generator=g)
    inside = torch.floor(torch.rand(shape, generator=g) * max(size - 1, 1)).long()
    band = torch.where(side, torch.full(shape, -1), torch.full(shape, size - 1))
    outside = torch.where(side, -2 - far, size + far)
    if size < 2:
        inside = band
    whole = torch.where(kind < 0.6, inside, torch.where(kind < 0.85, band, outside))
    return whole.double() + frac


@functools.lru_cache(maxsize=None)
def make_case(levels, ref_dim, N, Lq, seed=None):
    """fp32 CPU tensors value, ref, offsets [N,Lq,M*L*P*2], logits [N,Lq,M*L*P], grad_out plus sizes / shapes / lsi."""
    sizes = LEVELS[levels]
    L = len(sizes)
    g = torch.Generator().manual_seed(7919 * list(LEVELS).index(levels) + 1009 * ref_dim + 31 * N + Lq if seed is None else seed)
    shapes, lsi = level_tensors(sizes)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    value = torch.randn(N, S, M, D, generator=g)
    ref = 0.1 + 0.8 * torch.rand(N, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = 0.2 + 0.4 * torch.rand(N, Lq, L, 2, generator=g)
    target = torch.empty(N, Lq, M, L, P, 2, dtype=torch.float64)
    for l, (H, W) in enumerate(sizes):
        target[:, :, :, l, :, 0] = _draw_pixels(g, (N, Lq, M, P), W)
        target[:, :, :, l, :, 1] = _draw_pixels(g, (N, Lq, M, P), H)
    wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=torch.float64)[None, None, None, :, None, :]
    loc = (target + 0.5) / wh
    r64 = ref.double()
    if ref_dim == 2:
        off = (loc - r64[:, :, None, :, None, :]) * wh
    else:
        off = (loc - r64[:, :, None, :, None, :2]) / (r64[:, :, None, :, None, 2:] * 0.5) * P
    offsets = off.float()
    # the yardstick's own guarantee: fp32 and fp64 agree on every floor and every in-range verdict
    p64 = pixel_coordinates(r64, offsets.double(), sizes)
    p32 = pixel_coordinates(ref, offsets, sizes).double()
    noise = (p32 - p64).abs().max().item()
    assert noise < MAX_COORD_NOISE, noise
    assert torch.equal(torch.floor(p32), torch.floor(p64)) and torch.equal(torch.floor(p64), torch.floor(target))
    size = torch.as_tensor([(w, h) for h, w in sizes], dtype=torch.float64)[None, None, None, :, None, :]
    assert torch.equal((p32 > -1) & (p32 < size), (p64 > -1) & (p64 < size))
    frac = p64 - torch.floor(p64)
    assert frac.min() > 0.04 and frac.max() < 0.96
    return {"value": value, "ref": ref, "offsets": offsets.reshape(N, Lq, -1),
            "logits": torch.randn(N, Lq, M * L * P, generator=g), "grad_out": torch.randn(N, Lq, M * D, generator=g),
            "sizes": sizes, "shapes": shapes, "lsi": lsi, "noise": noise, "L": L}


def reference_forward(value, ref, offsets, logits, sizes):
    """The reference statement in the dtype of the arguments: torch softmax, the module's location arithmetic,
    ms_deform_attn_core_pytorch."""
    N, Lq, L = ref.shape[:3]
    aw = torch.softmax(logits.view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    return ms_deform_attn_core_pytorch(value, sizes, locations(ref, offsets.view(N, Lq, M, L, P, 2), sizes), aw)


def autograd_backward(case, dtype):
    """{gradient name: tensor} through autograd of the reference statement, on the CPU in ``dtype``."""
    t = {k: case[k].detach().to(dtype).clone().requires_grad_() for k in GRADS}
    out = reference_forward(t["value"], t["ref"], t["offsets"], t["logits"], case["sizes"])
    return dict(zip(GRADS, torch.autograd.grad(out, [t[k] for k in GRADS], case["grad_out"].to(dtype))))


def restated_backward(case, dtype=torch.float64):
    """The backward the kernel implements, formula by formula (csrc/msda_fused_backward.hip), in plain tensor arithmetic:
    g_a, g_x, g_y per (query, head, level, point) as in msda_bwd_m8d32, then the softmax, offset and reference-point
    gradients in closed form."""
    value, ref, logits = (case[k].to(dtype) for k in ("value", "ref", "logits"))
    sizes = case["sizes"]
    N, Lq, L, ref_dim = ref.shape
    offsets = case["offsets"].to(dtype).view(N, Lq, M, L, P, 2)
    top = case["grad_out"].to(dtype).view(N, Lq, M, 1, D)
    a = torch.softmax(logits.view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    pix = pixel_coordinates(ref, offsets, sizes)
    g_value = torch.zeros_like(value)
    g_a, g_x, g_y = (torch.zeros(N, Lq, M, L, P, dtype=dtype) for _ in range(3))
    start = 0
    for l, (H, W) in enumerate(sizes):
        flat = value[:, start:start + H * W].permute(0, 2, 1, 3)                       # [N,M,HW,D]
        g_flat = torch.zeros_like(flat)
        px, py = pix[:, :, :, l, :, 0], pix[:, :, :, l, :, 1]                         # [N,Lq,M,P]
        inr = (py > -1) & (px > -1) & (py < H) & (px < W)                             # the skip rule
        x0, y0 = torch.floor(px), torch.floor(py)
        lw, lh = px - x0, py - y0
        hw, hh = 1 - lw, 1 - lh
        for dy, dx, wgt, d_h, d_w in ((0, 0, hh * hw, -hw, -hh), (0, 1, hh * lw, -lw, hh),
                                      (1, 0, lh * hw, hw, -lh), (1, 1, lh * lw, lw, lh)):
            xi, yi = x0 + dx, y0 + dy
            ok = (inr & (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)).to(dtype)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            idx = idx.permute(0, 2, 1, 3).reshape(N, M, Lq * P, 1).expand(-1, -1, -1, D)
            v = torch.gather(flat, 2, idx).view(N, M, Lq, P, D).permute(0, 2, 1, 3, 4)  # [N,Lq,M,P,D]
            tv = (top * v).sum(-1)                                                     # grad_out . corner value
            g_a[:, :, :, l] += ok * wgt * tv
            g_x[:, :, :, l] += ok * W * a[:, :, :, l] * d_w * tv
            g_y[:, :, :, l] += ok * H * a[:, :, :, l] * d_h * tv
            contrib = (ok * wgt * a[:, :, :, l]).unsqueeze(-1) * top                   # [N,Lq,M,P,D]
            g_flat.scatter_add_(2, idx, contrib.permute(0, 2, 1, 3, 4).reshape(N, M, Lq * P, D))
        g_value[:, start:start + H * W] = g_flat.permute(0, 2, 1, 3)
        start += H * W
    dot = (a * g_a).sum((3, 4), keepdim=True)
    g_logits = a * (g_a - dot)
    g_xy = torch.stack([g_x, g_y], -1)                                                 # [N,Lq,M,L,P,2]
    g_ref = torch.zeros_like(ref)
    g_ref[..., :2] = g_xy.sum((2, 4))
    if ref_dim == 2:
        wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=dtype)[None, None, None, :, None, :]
        g_off = g_xy / wh
    else:
        g_off = g_xy * ref[:, :, None, :, None, 2:] * 0.5 / P
        g_ref[..., 2:] = (g_xy * offsets).sum((2, 4)) * 0.5 / P
    return {"value": g_value, "offsets": g_off.reshape(N, Lq, -1), "logits": g_logits.reshape(N, Lq, -1), "ref": g_ref}


def rel_err(got, ref):
    """max |got - ref| relative to the gradient's largest magnitude (as tests/_dynconv_cases.py)."""
    return ((got.double() - ref.double()).abs().max() / ref.abs().max().clamp(min=1e-300)).item()
