"""Shared builders of the single-level MSDA backward tests (csrc/msda_level_backward.hip): seeded cases over ONE level of a
given (H, W), built from the functions of tests/_msda_fused_cases.py - the same kink-free construction (target pixel
coordinates integer + fraction in [0.05, 0.95], the offset solved from the reference point in fp64 and rounded to fp32)
and the same assertions on floors and in-range verdicts - so that ``restated_backward`` and ``autograd_backward`` of that
file apply to them unchanged.  The references of a case are computed once and shared (``references``)."""
import functools

import torch

from tests import _msda_fused_cases as fc

M, D, P = fc.M, fc.D, fc.P
# (H, W, N, Lq, strided rows): fewer queries than the 1024 threads; a thread's second query; the 146 KB image of the
# 50 x 84 level (the LDS opt-in); 288 items on 256 CUs (the persistent loop, re-zeroing between items); a 1 x 1 level;
# offsets and logits as column slices of a wider buffer; a one-row and a one-column level with a single query (the flush
# walk's carry: every step a new row at W = 1); 1032 tokens with 1025 queries (a third flush pass of the float policy's
# 512 tokens per pass, a second of the fixed policy's 1024; one thread with a second query).  N = 9 is 288 float and
# 576 fixed items.  No queries at all cannot stand here (a case needs samples to check its own construction): the
# entry tests of both routes hold it (test_entry_writes_every_element_once_and_nothing_else, test_edges_give_exact_zeros).
KERNEL_CASES = [(5, 7, 3, 37, False), (20, 31, 2, 1100, False), (50, 84, 1, 1100, False), (5, 7, 9, 37, False),
                (1, 1, 2, 5, False), (5, 7, 3, 37, True), (1, 7, 2, 1, False), (7, 1, 2, 1, False), (24, 43, 1, 1025, False)]


@functools.lru_cache(maxsize=None)
def make_level_case(H, W, ref_dim, N, Lq, collide=False):
    """fp32 CPU tensors value [N,H*W,8,32], ref [N,Lq,1,ref_dim], offsets [N,Lq,64], logits [N,Lq,32], grad_out [N,Lq,256]
    plus sizes / shapes / lsi, as fc.make_case returns them.  collide: every query has the reference point and the offsets
    of the first, so all of them add into the same 2 x 2 blocks."""
    sizes = [(H, W)]
    g = torch.Generator().manual_seed(104729 * H + 1299709 * W + 1009 * ref_dim + 31 * N + Lq + (7 if collide else 0))
    shapes, lsi = fc.level_tensors(sizes)
    value = torch.randn(N, H * W, M, D, generator=g)
    ref = 0.1 + 0.8 * torch.rand(N, Lq, 1, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = 0.2 + 0.4 * torch.rand(N, Lq, 1, 2, generator=g)
    target = torch.empty(N, Lq, M, 1, P, 2, dtype=torch.float64)
    target[:, :, :, 0, :, 0] = fc._draw_pixels(g, (N, Lq, M, P), W)
    target[:, :, :, 0, :, 1] = fc._draw_pixels(g, (N, Lq, M, P), H)
    if collide:
        ref = ref[:1, :1].expand(N, Lq, 1, ref_dim).contiguous()
        target = target[:1, :1].expand(N, Lq, M, 1, P, 2).contiguous()
    wh = torch.as_tensor([(W, H)], dtype=torch.float64)[None, None, None, :, None, :]
    loc = (target + 0.5) / wh
    r64 = ref.double()
    if ref_dim == 2:
        off = (loc - r64[:, :, None, :, None, :]) * wh
    else:
        off = (loc - r64[:, :, None, :, None, :2]) / (r64[:, :, None, :, None, 2:] * 0.5) * P
    offsets = off.float()
    # the yardstick's own guarantee (as fc.make_case): fp32 and fp64 agree on every floor and every in-range verdict
    p64 = fc.pixel_coordinates(r64, offsets.double(), sizes)
    p32 = fc.pixel_coordinates(ref, offsets, sizes).double()
    noise = (p32 - p64).abs().max().item()
    assert noise < fc.MAX_COORD_NOISE, noise
    assert torch.equal(torch.floor(p32), torch.floor(p64)) and torch.equal(torch.floor(p64), torch.floor(target))
    assert torch.equal((p32 > -1) & (p32 < wh), (p64 > -1) & (p64 < wh))
    frac = p64 - torch.floor(p64)
    assert frac.min() > 0.04 and frac.max() < 0.96
    return {"value": value, "ref": ref, "offsets": offsets.reshape(N, Lq, -1),
            "logits": torch.randn(N, Lq, M * P, generator=g), "grad_out": torch.randn(N, Lq, M * D, generator=g),
            "sizes": sizes, "shapes": shapes, "lsi": lsi, "noise": noise, "L": 1}


@functools.lru_cache(maxsize=None)
def references(H, W, ref_dim, N, Lq, collide=False):
    """(fp64 restated grad_value, the CPU's own fp32 autograd grad_value) of a case; computed once, never written to."""
    case = make_level_case(H, W, ref_dim, N, Lq, collide)
    return fc.restated_backward(case)["value"], fc.autograd_backward(case, torch.float32)["value"]
