"""Cases, the fp64 reference, the fp32 yardsticks and the host-arithmetic mirrors shared by tests/test_conv_cases_cpu.py and
tests/test_conv_edges_gpu.py.

The operators are the three hand-written convolutions behind dfx.ops.ConvPlan: Winograd F(2x2,3x3) (csrc/conv_wino.hip), the
implicit GEMM (csrc/conv_igemm.hip) and the LDS-tile kernel of few input channels (csrc/conv_tile.hip).

Two families of operands, both fp64 CPU tensors of fp32-representable values, seeded from the shape:
  exact   inputs in {-3..3}, integer biases, weights that are multiples of 4 in {-8..8} - or, with a per-channel scale out of
          {0.5, 1, 2}, multiples of 8.  Every product, every Winograd transform (its two 0.5 factors included) and every
          partial sum is then an integer far below 2^24: any summation order gives the same bits, and a correct kernel equals
          fp64 F.conv2d EXACTLY.  (The largest case: |U| <= 36, |V| <= 12, 72 channels, nine terms of A^T M A: < 2^19.)
          tests/test_conv_cases_cpu.py proves the condition on every listed shape with the fp32 yardsticks below.
  real    x = relu(2 randn + 1) + a per-channel offset (non-negative maps with non-zero means, as a convolution sees them after
          a ReLU), weights / sqrt(K), a scale in [0.5, 1.5), a bias.  The bound is the project's: rel_err of the GPU result at
          most YARDSTICK_FACTOR times the rel_err of the same arithmetic in fp32 on the CPU:
            direct_yardstick   one (tap, channel) term at a time in the kernels' K order: taps (ky, kx) major, channels minor
            wino_yardstick     gk = w * scale, U = G gk G^T with the 0.5 factors placed as wino_weights_kernel places them,
                               V = B^T d B per 4x4 patch of each dilation sub-lattice (rows, then columns, the kernel's signs),
                               the 16 products summed over the input channels one at a time, A^T M A, bias, activation
``reference`` is fp64 F.conv2d of weight * scale, plus the bias, then the activation.
"""
import functools

import torch
import torch.nn.functional as F

from tests._linear_train_cases import YARDSTICK_FACTOR, rel_err  # noqa: F401  (the project's factor and error measure)

# ---- exact cases -----------------------------------------------------------------------------------------------------
# (N, Ci, Co, H, W, dil): 3x3 / stride 1 / padding = dilation
WINO_EXACT = [
    (1, 8, 64, 1, 1, 1),           # a 1x1 map
    (2, 8, 64, 2, 3, 3),           # a map smaller than the dilation: the last tile row / column lies wholly outside it
    (3, 72, 64, 11, 13, 1),        # 9 chunks (the smallest count the host rule phases, odd), three images in one block
    (1, 24, 128, 9, 10, 2),        # 3 chunks, two channel blocks
    (1, 16, 64, 13, 21, 2),        # dilation 2, odd map
    (2, 8, 64, 160, 130, 1),       # 163 blocks: remainder > 160, one full-size launch whose last tile block is partial
    (1, 8, 128, 180, 182, 1),      # 256 blocks: remainder 0
    (1, 8, 64, 322, 322, 1),       # 406 blocks = 256 + 150 as quarter-size workgroups (a remainder near 160)
]
WINO_MULTI_ROUND = WINO_EXACT[5:]
# what tests name them for: [(kind, logical blocks), ...] of the host rule, and with DFX_WINO_NO_TAIL
WINO_REGIMES = {
    (1, 8, 64, 1, 1, 1): [("quarter", 1)],
    (2, 8, 64, 2, 3, 3): [("quarter", 1)],
    (3, 72, 64, 11, 13, 1): [("quarter", 2)],
    (1, 24, 128, 9, 10, 2): [("quarter", 2)],
    (1, 16, 64, 13, 21, 2): [("quarter", 2)],
    (2, 8, 64, 160, 130, 1): [("full", 163)],
    (1, 8, 128, 180, 182, 1): [("full", 256)],
    (1, 8, 64, 322, 322, 1): [("full", 256), ("quarter", 150)],
}
WINO_REGIMES_NO_TAIL = {
    (2, 8, 64, 160, 130, 1): [("full", 163)],
    (1, 8, 128, 180, 182, 1): [("full", 256)],
    (1, 8, 64, 322, 322, 1): [("full", 406)],
}

# (N, Ci, Co, H, W, kh, kw, stride, pad, dil)
IGEMM_EXACT = [
    (1, 1, 1, 1, 1, 1, 1, 1, 0, 1),          # the smallest problem
    (1, 16, 8, 4, 4, 1, 1, 1, 0, 1),         # one K-step, uniform tap
    (1, 2, 8, 11, 12, 8, 8, 1, 3, 1),        # 64 taps: bit 63 of the tap mask
    (2, 5, 24, 9, 14, 1, 7, 1, 0, 1),        # kh != kw
    (2, 5, 24, 14, 9, 5, 2, 2, 1, 1),        # kh != kw, stride 2
    (1, 16, 64, 5, 6, 3, 3, 1, 3, 1),        # padding beyond the kernel's reach: the border outputs are the bias alone
    (2, 16, 40, 17, 19, 3, 3, 3, 2, 2),      # stride 3 with dilation 2 (uniform-tap template)
    (2, 17, 40, 17, 19, 3, 3, 3, 2, 2),      # the same geometry through the general template
    (1, 16, 72, 12, 14, 3, 3, 1, 1, 1),      # P % 4 == 0, tile rows beyond Co
    (1, 16, 72, 13, 13, 3, 3, 1, 1, 1),      # scalar epilogue
]

# (N, Ci, Co, H, W, k, stride, pad) -> the conv_tile_kernel<MT, NS> template it runs on
TILE_EXACT = [
    ((2, 3, 32, 30, 45, 7, 2, 3), "1,9"),    # 3 -> 32 channels at 7x7/2: Co <= 32 with 9 staged elements per thread
    ((2, 4, 24, 21, 37, 3, 2, 1), "1,9"),    # four input channels
    ((3, 1, 16, 19, 35, 3, 2, 1), "1,3"),    # the DFormer stem's first convolution
    ((2, 3, 40, 17, 37, 5, 2, 2), "2,9"),    # two 32-channel blocks
]
# the persistent walk: (Ci, Co, k, stride, pad) on many tiny images of (H, W); N comes from the device (walk_images)
WALK_CONVS = [(1, 16, 3, 2, 1), (3, 64, 7, 2, 3)]
# 18x70 and 20x72 have 2 x 2 tiles per image: the grids of a 256-CU device (1024 and 512 workgroups) are multiples of 4, so a
# workgroup only ever steps from image to image on the same tile - the double-buffered staging and the image advance, no carry.
# 36x140 and 40x144 (18x70 and 20x72 OUTPUT maps) have 3 x 3 tiles: 1024 = 113 * 9 + 2 * 3 + 1, 512 = 56 * 9 + 2 * 3 + 2, so
# every step moves the tile column and the tile row as well and both scalar carries fire (tile_walk, WALK_CARRY_MAPS).
WALK_MAPS = [(18, 70), (20, 72), (36, 140), (40, 144)]
WALK_CARRY_MAPS = WALK_MAPS[2:]
MI355X_CUS = 256

# the exact operands of the host-path tests (tests/test_conv_edges_gpu.py: the two batch splits and the channel slices)
WINO_SPLIT = (5, 16, 64, 9, 11, 2)                    # (N, Ci, Co, H, W, dil), with scale
TILE_SPLIT = (5, 3, 40, 19, 37, 5, 2, 2)              # (N, Ci, Co, H, W, k, stride, pad)
CLIP_SLICES = {"rgb": slice(0, 3), "depth": slice(3, 4)}


def out_size(H, W, kh, kw, stride, pad, dil):
    return (H + 2 * pad - (kh - 1) * dil - 1) // stride + 1, (W + 2 * pad - (kw - 1) * dil - 1) // stride + 1


def walk_images(cus, H, W, k, stride, pad):
    """images so that the tile kernel has at least 2.5 x 4 x ``cus`` tiles (8 x 32 output pixels each): with at most 4
    workgroups per CU every workgroup then walks several tiles, across tile-row and image boundaries"""
    Ho, Wo = out_size(H, W, k, k, stride, pad, 1)
    per = ((Ho + 7) // 8) * ((Wo + 31) // 32)
    return -(-10 * cus // per)


def _f32(t):
    return t.float().double()


def _seed(shape, salt):
    s = salt
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


def _pack(x, weight, bias, scale, geom, act):
    kh, kw, stride, pad, dil = geom
    return {"x": x, "weight": weight, "bias": bias, "scale": scale, "kh": kh, "kw": kw, "stride": stride, "pad": pad,
            "dil": dil, "act": act}


def make_exact_case(N, Ci, Co, H, W, kh=3, kw=3, stride=1, pad=1, dil=1, act=None, bias=True, scale=False):
    """the integer operands of the module docstring; without ``scale`` the weights are multiples of 4, with it multiples of 8"""
    g = torch.Generator().manual_seed(_seed((N, Ci, Co, H, W, kh, kw, stride, pad, dil, int(bias), int(scale)), 1))
    x = torch.randint(-3, 4, (N, Ci, H, W), generator=g).double()
    if scale:
        w = 8.0 * torch.randint(-1, 2, (Co, Ci, kh, kw), generator=g).double()
        sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (Co,), generator=g)]
    else:
        w = 4.0 * torch.randint(-2, 3, (Co, Ci, kh, kw), generator=g).double()
        sc = None
    b = torch.randint(-9, 10, (Co,), generator=g).double() if bias else None
    return _pack(x, w, b, sc, (kh, kw, stride, pad, dil), act)


def make_real_case(N, Ci, Co, H, W, kh=3, kw=3, stride=1, pad=1, dil=1, act=None):
    """the realistic operands of the module docstring"""
    g = torch.Generator().manual_seed(_seed((N, Ci, Co, H, W, kh, kw, stride, pad, dil), 2))
    x = (2.0 * torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64) + 1.0).relu() \
        + torch.rand(1, Ci, 1, 1, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, kh, kw, generator=g, dtype=torch.float64) / (Ci * kh * kw) ** 0.5
    sc = torch.rand(Co, generator=g, dtype=torch.float64) + 0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    return _pack(_f32(x), _f32(w), _f32(b), _f32(sc), (kh, kw, stride, pad, dil), act)


def make_clip_case(name):
    """-> (clip [3,4,13,18] of the exact inputs, the exact 3x3/2 case whose x is the contiguous copy of the channel slice
    CLIP_SLICES[name] of it): what the stems read in place from an RGB-D clip"""
    sl = CLIP_SLICES[name]
    T, H, W, Ci = 3, 13, 18, sl.stop - sl.start
    clip = torch.randint(-3, 4, (T, 4, H, W), generator=torch.Generator().manual_seed(41)).double()
    return clip, dict(make_exact_case(T, Ci, 24, H, W, 3, 3, 2, 1, 1, act="relu"), x=clip[:, sl].contiguous())


def with_act(case, act):
    """the same operands (shared, not copied) under another activation"""
    return dict(case, act=act)


def _activate(y, act):
    if act == "relu":
        return y.relu()
    if act == "gelu":
        return F.gelu(y)
    assert act is None, act
    return y


def _scaled_weight(case, dtype):
    w = case["weight"].to(dtype)
    return w if case["scale"] is None else w * case["scale"].to(dtype).view(-1, 1, 1, 1)


def reference(case):
    """fp64 F.conv2d of weight * scale, plus the bias, then the activation"""
    y = F.conv2d(case["x"], _scaled_weight(case, torch.float64), case["bias"], case["stride"], case["pad"], case["dil"])
    return _activate(y, case["act"])


def direct_yardstick(case, dtype=torch.float32):
    """The sum in ``dtype`` on the CPU, sequentially in the kernels' K order: taps (ky, kx) major, channels minor, one
    (tap, channel) term at a time; then the bias and the activation in ``dtype``."""
    x, w = case["x"].to(dtype), _scaled_weight(case, dtype)
    kh, kw, s, p, d = (case[n] for n in ("kh", "kw", "stride", "pad", "dil"))
    N, Ci, H, W = x.shape
    Co = w.shape[0]
    Ho, Wo = out_size(H, W, kh, kw, s, p, d)
    xp = F.pad(x, (p, p, p, p))
    acc = torch.zeros(N, Co, Ho, Wo, dtype=dtype)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, :, ky * d: ky * d + (Ho - 1) * s + 1: s, kx * d: kx * d + (Wo - 1) * s + 1: s]
            for ci in range(Ci):
                acc += w[:, ci, ky, kx].view(1, Co, 1, 1) * win[:, ci].unsqueeze(1)
    if case["bias"] is not None:
        acc = acc + case["bias"].to(dtype).view(1, Co, 1, 1)
    return _activate(acc, case["act"])


def _wino_lattice(xs, U, bias, dtype):
    """F(2x2,3x3) of one dilation sub-lattice xs [N,Ci,Hs,Ws] (a plain 3x3 / padding 1 convolution on it) -> [N,Co,Hs,Ws]"""
    N, Ci, Hs, Ws = xs.shape
    Co = U.shape[0]
    TY, TX = (Hs + 1) // 2, (Ws + 1) // 2
    xp = F.pad(xs, (1, 2 * TX + 1 - Ws, 1, 2 * TY + 1 - Hs))
    # the 4x4 patch of tile (ty, tx): rows 2 ty - 1 .. 2 ty + 2, columns 2 tx - 1 .. 2 tx + 2
    dd = [[xp[:, :, i: i + 2 * TY: 2, j: j + 2 * TX: 2] for j in range(4)] for i in range(4)]
    # B^T d (rows), then (B^T d) B (columns): the kernel's expressions
    t = [[dd[0][j] - dd[2][j] for j in range(4)], [dd[1][j] + dd[2][j] for j in range(4)],
         [dd[2][j] - dd[1][j] for j in range(4)], [dd[1][j] - dd[3][j] for j in range(4)]]
    V = [[t[i][0] - t[i][2], t[i][1] + t[i][2], t[i][2] - t[i][1], t[i][1] - t[i][3]] for i in range(4)]
    V = torch.stack([torch.stack(r, 2) for r in V], 2)                 # [N,Ci,4,4,TY,TX]
    M = torch.zeros(N, Co, 4, 4, TY, TX, dtype=dtype)
    for ci in range(Ci):
        M += U[:, ci].view(1, Co, 4, 4, 1, 1) * V[:, ci].unsqueeze(1)
    m = [[M[:, :, i, j] for j in range(4)] for i in range(4)]
    t0 = [m[0][j] + m[1][j] + m[2][j] for j in range(4)]
    t1 = [m[1][j] - m[2][j] - m[3][j] for j in range(4)]
    bv = 0 if bias is None else bias.view(1, Co, 1, 1)
    y = torch.empty(N, Co, 2 * TY, 2 * TX, dtype=dtype)
    y[:, :, 0::2, 0::2] = t0[0] + t0[1] + t0[2] + bv
    y[:, :, 0::2, 1::2] = t0[1] - t0[2] - t0[3] + bv
    y[:, :, 1::2, 0::2] = t1[0] + t1[1] + t1[2] + bv
    y[:, :, 1::2, 1::2] = t1[1] - t1[2] - t1[3] + bv
    return y[:, :, :Hs, :Ws]


def wino_yardstick(case, dtype=torch.float32):
    """Winograd F(2x2,3x3) in ``dtype`` on the CPU as csrc/conv_wino.hip does it (module docstring)."""
    assert (case["kh"], case["kw"], case["stride"]) == (3, 3, 1) and case["pad"] == case["dil"]
    x, gk, d = case["x"].to(dtype), _scaled_weight(case, dtype), case["dil"]
    bias = None if case["bias"] is None else case["bias"].to(dtype)
    # U = G gk G^T: rows (G gk), then columns, 0.5 * (a + b + c) and 0.5 * (a - b + c) left to right
    t = [gk[:, :, 0], 0.5 * (gk[:, :, 0] + gk[:, :, 1] + gk[:, :, 2]), 0.5 * (gk[:, :, 0] - gk[:, :, 1] + gk[:, :, 2]), gk[:, :, 2]]
    U = torch.stack([torch.stack([r[..., 0], 0.5 * (r[..., 0] + r[..., 1] + r[..., 2]),
                                  0.5 * (r[..., 0] - r[..., 1] + r[..., 2]), r[..., 2]], -1) for r in t], 2)    # [Co,Ci,4,4]
    N, Ci, H, W = x.shape
    y = torch.empty(N, gk.shape[0], H, W, dtype=dtype)
    for a in range(min(d, H)):
        for b in range(min(d, W)):
            y[:, :, a::d, b::d] = _wino_lattice(x[:, :, a::d, b::d], U, bias, dtype)
    return _activate(y, case["act"])


# ---- mirrors of the host's launch arithmetic ---------------------------------------------------------------------------
def wino_launches(N, Ci, Co, H, W, dil, no_tail=False):
    """[(kind, logical blocks), ...] as dfx_conv3x3_wino_f32 launches them: blocks of 64 output channels x 64 tiles, rounds of
    256; a last round of at most 160 blocks runs as quarter-size workgroups unless DFX_WINO_NO_TAIL is set."""
    TY = (H + 2 * dil - 1) // (2 * dil) * dil
    TX = (W + 2 * dil - 1) // (2 * dil) * dil
    tiles = N * TY * TX
    ntb = (tiles + 63) // 64
    blocks = ntb * (Co // 64)
    rem = blocks % 256
    quarter = 0 < rem <= 160 and not no_tail
    main = blocks - rem if quarter else blocks
    return ([("full", main)] if main > 0 else []) + ([("quarter", rem)] if quarter else [])


def wino_blocks_of_record(nbytes, Ci):
    """logical blocks of a tag -3 profile record: its byte field holds 2 * 16 * 64 * Ci * 64 flops per block"""
    per = 2 * 16 * 64 * Ci * 64
    assert nbytes % per == 0, (nbytes, per)
    return nbytes // per


def tile_template(Ci, Co, k, stride):
    """"MT,NS" of the conv_tile_kernel<MT, NS> that dfx_conv2d_tile_f32 launches: MT 32-channel blocks, NS staged elements
    per thread (3 or the maximum, 9) for the (7 s + k) x (31 s + k) input rectangle of a tile"""
    IH, IW = 7 * stride + k, 31 * stride + k
    nstage = (Ci * IH * IW + 511) // 512
    assert nstage <= 9
    MT = 1 if Co <= 32 else 2
    return "1,3" if MT == 1 and nstage <= 3 else "1,9" if MT == 1 else "2,9"


def tile_walk(cus, N, Ci, Co, H, W, k, stride, pad):
    """The persistent walk of dfx_conv2d_tile_f32 / conv_tile_kernel on a device of ``cus`` CUs, mirrored: the LDS bytes, the
    workgroups per CU they allow, the grid G, its decomposition G = d_n * TY * TX + d_ty * TX + d_tx that ``advance`` adds
    with two carries, and - walking every workgroup through the steps whose target tile exists - how many workgroups take
    the tile-column carry (tx >= TX), the tile-row carry (ty >= TY), and both within their steps."""
    Ho, Wo = out_size(H, W, k, k, stride, pad, 1)
    Kpad = (Ci * k * k + 15) // 16 * 16
    MT = 1 if Co <= 32 else 2
    IH, IW = 7 * stride + k, 31 * stride + k
    PW = 2 * ((IW + 1) // 2) if stride == 2 else IW
    lds = (32 * MT * (Kpad + 4) + Kpad + 2 * Ci * IH * PW + 32 * MT) * 4
    per_cu = 4 if lds * 4 <= 160 * 1024 else 2 if lds * 2 <= 160 * 1024 else 1
    TY, TX = (Ho + 7) // 8, (Wo + 31) // 32
    tiles = N * TY * TX
    G = min(tiles, cus * per_cu)
    d_n, rest = divmod(G, TY * TX)
    d_ty, d_tx = divmod(rest, TX)
    col = row = both = 0
    for b in range(G):
        n, r = divmod(b, TY * TX)
        ty, tx = divmod(r, TX)
        t, c_col, c_row = b, 0, 0
        while t + G < tiles:                             # (the kernel advances once more; that position is never used)
            tx += d_tx
            if tx >= TX:
                tx, ty, c_col = tx - TX, ty + 1, c_col + 1
            ty += d_ty
            if ty >= TY:
                ty, n, c_row = ty - TY, n + 1, c_row + 1
            n += d_n
            t += G
            assert (n * TY + ty) * TX + tx == t          # the carries keep the position on the tile's linear index
        col, row, both = col + (c_col > 0), row + (c_row > 0), both + (c_col > 0 and c_row > 0)
    return {"lds": lds, "per_cu": per_cu, "grid": G, "tiles": tiles, "TY": TY, "TX": TX, "d_n": d_n, "d_ty": d_ty, "d_tx": d_tx,
            "column_carry": col, "row_carry": row, "both_carries": both}


# ---- evidence for a failed exact comparison ----------------------------------------------------------------------------
def describe_mismatch(got, ref, limit=12):
    """which outputs differ: count, the set of images / channels, the bounding box, and the first few (n, co, y, x: got, want)"""
    got, ref = got.double().cpu(), ref.double()
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    bad = (got != ref) | (got.isnan() != ref.isnan())
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "equal"
    head = "; ".join(f"{tuple(i.tolist())}: {got[tuple(i)].item():g} != {ref[tuple(i)].item():g}" for i in idx[:limit])
    return (f"{idx.shape[0]} of {bad.numel()} outputs differ; images {sorted(set(idx[:, 0].tolist()))[:8]}, "
            f"channels {sorted(set(idx[:, 1].tolist()))[:16]}, rows {idx[:, 2].min().item()}..{idx[:, 2].max().item()} "
            f"(parities {sorted(set((idx[:, 2] % 2).tolist()))}), columns {idx[:, 3].min().item()}..{idx[:, 3].max().item()} "
            f"(parities {sorted(set((idx[:, 3] % 2).tolist()))}); first: {head}")


# ---- cached, never modified ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)                   # the four (bias, scale) variants of the case at hand
def exact_prepared(geom, bias, scale):
    """(case without activation, its fp64 reference before the activation) of ``make_exact_case(*geom, bias=, scale=)``;
    ReLU of the reference is taken by the caller (exact in any precision)."""
    case = make_exact_case(*geom, bias=bias, scale=scale)
    return case, reference(case)


@functools.lru_cache(maxsize=None)
def real_prepared(geom, act, algo):
    """(case, fp64 reference, fp32 yardstick of ``algo``'s arithmetic) of ``make_real_case(*geom, act=act)``"""
    case = make_real_case(*geom, act=act)
    return case, reference(case), (wino_yardstick if algo == "wino" else direct_yardstick)(case)
