"""Every tile of the MFMA GEMM (csrc/gemm_f32.hip) through every epilogue of csrc/mfma_tile.h, at the smallest shapes that still
have a partial last tile on both axes.  The case list stands apart from its test (tests/test_gemm_tiles_gpu.py) so that a
job comparing two builds of the library bit for bit can run the same cases.

A case runs with DFX_GEMM_NO_ROWS=1 (the few-row kernel would take these shapes) and its ``env`` (DFX_GEMM_TILE forces a
tile; None leaves the choice to the rule, which picks 128 x 32 for N <= 32 and 128 x 96 for N <= 96)."""
from collections import namedtuple

import torch

# name, DFX_GEMM_TILE, N the rule needs (None: the case's own), tag_b = BM * 1000 + BN the profile hook must report, K per step
TILES = [
    ("128x128", "0", None, 128128, 16),
    ("128x64", "1", None, 128064, 16),
    ("64x128", "2", None, 64128, 16),
    ("64x64", "5", None, 64064, 16),
    ("64x64k64", "6", None, 64064, 64),
    ("256x128", "7", None, 256128, 16),
    ("128x32", None, 32, 128032, 16),
    ("128x96", None, 96, 128096, 16),
]
M = 300                      # a partial last tile for every BM
KS = (128, 72)               # LDS-DMA staging (two steps even at 64 per step); a K tail, staged through registers
LINEAR = ["plain", "bias_relu", "bias_res_relu_mask", "add_res_gelu", "scalar", "cblk4", "cblk12", "xblocked_res"]

Case = namedtuple("Case", "id kind tile env expect K N variant")


def _linear_n(variant, fixed):
    """N = 200 unless the tile rule or the variant fixes it.  scalar: N not a multiple of 4 (two more columns, or two fewer where
    the rule bounds N).  cblk12: N = 192 - the scalar column-block path, as 12 divides neither 128 nor 64 - and N = 96 on the
    128 x 96 tile, where it is the fast form; 12 does not divide 32."""
    if variant == "scalar":
        return 202 if fixed is None else fixed - 2
    if variant == "cblk12":
        return 192 if fixed is None else (96 if fixed == 96 else None)
    return 200 if fixed is None else fixed


def cases():
    out = []
    for name, env, fixed, expect, bk in TILES:
        for K in KS:
            for v in LINEAR:
                N = _linear_n(v, fixed)
                if N is not None:
                    out.append(Case(f"linear-{name}-K{K}-{v}", "linear", name, env, expect, K, N, v))
        if fixed is not None:
            continue                                         # the convolutions' N is their 10 x 20 map
        for Ci in (64, 72):
            out.append(Case(f"conv1x1-{name}-Ci{Ci}", "conv1x1", name, env, expect, Ci, 200, "bias_res_relu"))
        if 32 % bk == 0:                                     # (a two-segment operand needs K1 to be whole K-steps)
            out.append(Case(f"pair-{name}", "pair", name, env, expect, 48, 200, "bias_relu"))
        else:                                                # ... so the [K,N] operand by LDS-DMA at 64 k per step is reached without
            out.append(Case(f"conv1x1-{name}-Ci128", "conv1x1", name, env, expect, 128, 200, "bias_relu"))   # a residual instead
    return out


CASES = cases()


def inputs(case):
    """The case's operands on the GPU, from a generator seeded by the case alone."""
    g = torch.Generator().manual_seed(sum(map(ord, case.id)))
    r = lambda *s: torch.randn(*s, generator=g).cuda()       # noqa: E731
    K, N, v = case.K, case.N, case.variant
    if case.kind == "linear":
        t = {"x": r(M, K), "w": r(N, K) / K ** 0.5}
        if v != "plain":
            t["b"] = r(N)
        if v in ("bias_res_relu_mask", "add_res_gelu", "xblocked_res"):
            t["res"] = r(M, N)
        if v == "add_res_gelu":
            t["add"] = r(M, K)
        if v in ("bias_res_relu_mask", "cblk4", "cblk12"):
            t["mask"] = (torch.rand(M, generator=g) > 0.8).cuda()
        if v == "xblocked_res":                              # K-block-major [K/4][M][4]
            t["xb"] = t["x"].view(M, K // 4, 4).permute(1, 0, 2).contiguous()
        return t
    if case.kind == "conv1x1":
        t = {"x": r(2, K, 10, 20), "w": r(M, K) / K ** 0.5, "b": r(M)}
        if v == "bias_res_relu":
            t["res"] = r(2, M, 10, 20)
        return t
    return {"x1": r(2, 32, 10, 20), "x2": r(2, 16, 10, 20), "w": r(M, 48) / 48 ** 0.5, "b": r(M)}


def _act(case):
    return {"plain": None, "cblk4": None, "cblk12": None, "add_res_gelu": "gelu"}.get(case.variant, "relu")


def _cblk(case):
    return {"cblk4": 4, "cblk12": 12}.get(case.variant, 0)


def run(case, t):
    from dfx import ops
    if case.kind == "conv1x1":
        return ops.conv1x1(t["x"], t["w"], t["b"], residual=t.get("res"), relu=True)
    if case.kind == "pair":
        return ops.conv1x1_pair(t["x1"], t["x2"], t["w"], t["b"], relu=True)
    return ops.linear(t.get("xb", t["x"]), t["w"], t.get("b"), residual=t.get("res"), add=t.get("add"), row_mask=t.get("mask"), act=_act(case),
                      col_block=_cblk(case), x_blocked=case.variant == "xblocked_res")


def reference(case, t):
    """float64, in the layout of the result"""
    d = {k: v.double() for k, v in t.items() if k not in ("mask", "xb")}
    if case.kind == "linear":
        y = (d["x"] + d.get("add", 0)) @ d["w"].t() + d.get("b", 0) + d.get("res", 0)
    elif case.kind == "conv1x1":
        y = torch.einsum("ok,nkhw->nohw", d["w"], d["x"]) + d["b"][None, :, None, None] + d.get("res", 0)
    else:
        y = torch.einsum("ok,nkhw->nohw", d["w"], torch.cat([d["x1"], d["x2"]], 1)) + d["b"][None, :, None, None]
    act = _act(case)
    y = y.relu() if act == "relu" else torch.nn.functional.gelu(y) if act == "gelu" else y
    if "mask" in t:
        y = y.masked_fill(t["mask"][:, None], 0.0)
    w = _cblk(case)
    return y.view(M, case.N // w, w).permute(1, 0, 2) if w else y


def tolerance(case):
    """the GEMM tests' bound: exact-fp32 products summed in fp32, 4e-6 sqrt(K), doubled with a prologue add"""
    return 4e-6 * case.K ** 0.5 * (2.0 if case.variant == "add_res_gelu" else 1.0)
