"""GPU: the kernels every inference run goes through - bias_act, bias_relu_maxpool, box_refine
(csrc/fused_epilogue.hip), add_layernorm (csrc/layernorm_train.hip), group_norm (csrc/groupnorm.hip) and the
DynamicConv forward (csrc/dynconv.hip) - against the
fp64 restatements of tests/_inference_kernel_cases.py.  The rule is the project's: error relative to the reference's
largest magnitude, at most 4 x the error of the same computation in fp32 on the CPU (floored at one fp32 ulp), printed
per output and case; what is exact is asserted with torch.equal.  One case per launch regime and template
instantiation; why the bound has room and teeth: tests/test_inference_kernels_cpu.py."""
import pytest
import torch

from tests import _dynconv_cases as dc
from tests import _inference_kernel_cases as ic

pytestmark = pytest.mark.gpu


def _place(t, offset=False):
    """``t`` on the GPU; with ``offset`` as a contiguous view that starts 4 bytes into its buffer."""
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _f32(args):
    return ic.cast(args, torch.float32)


# ---- bias_act --------------------------------------------------------------------------------------------------
BIAS_ACT_GRID = [(shape, offset, residual, relu) for shape, offset in ic.BIAS_ACT_CASES for residual in (False, True)
                 for relu in (False, True) if residual or offset != "residual"]


@pytest.mark.parametrize("shape,offset,residual,relu", BIAS_ACT_GRID)
def test_bias_act_is_bit_equal_to_the_same_expression_on_the_cpu(shape, offset, residual, relu):
    """(x + b) + r, then max(., 0): no multiply, nothing to contract or reorder, so the bits are the CPU's.  Vector path,
    scalar path by size and by the alignment of x or of the residual alone, chunks > 1 on both paths, HW = 1."""
    from dfx import ops
    x, b, r = ic.bias_act_inputs(shape)
    want = ic.bias_act(x, b, r if residual else None, relu)
    xg, rg = _place(x, offset == "x"), (_place(r, offset == "residual") if residual else None)
    got = ops.bias_act_(xg, b.cuda(), rg, relu=relu)
    assert got is xg and torch.equal(got.cpu(), want)
    assert rg is None or torch.equal(rg.cpu(), r)


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (2, 5, 7, 9)])
@pytest.mark.parametrize("residual", [False, True])
def test_bias_act_on_non_finite_inputs(shape, residual):
    """+-inf come out as on the CPU.  A NaN comes out as 0 under the ReLU - fmaxf returns its other operand, where
    torch.relu keeps the NaN - and as NaN without it (the docstring of ops.bias_act_ says so)."""
    from dfx import ops
    x, b, r = ic.bias_act_inputs(shape)
    flat = x.view(-1)
    flat[0::7], flat[1::11], flat[2::13] = float("inf"), float("-inf"), float("nan")
    nan = x.isnan()
    assert nan.any() and x.isposinf().any() and x.isneginf().any()
    for relu in (True, False):
        want = ic.bias_act(x, b, r if residual else None, relu)
        got = ops.bias_act_(x.cuda(), b.cuda(), r.cuda() if residual else None, relu=relu).cpu()
        assert torch.equal(got[~nan], want[~nan])
        assert got[nan].eq(0).all() if relu else got[nan].isnan().all()


# ---- bias_relu_maxpool -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", ic.POOL_H)
@pytest.mark.parametrize("W", ic.POOL_W)
def test_stem_epilogue_is_bit_equal_at_the_fast_path_switches(H, W):
    """The widths at which the 16-byte path (xl + 8 < W) switches on and off inside a row, output widths that are no
    multiple of 4, 1 to 3 input rows under a window.  The grid-stride pass beyond 2^20 workgroups is not reached by any
    test: it takes 2^20 * 256 items of four outputs, 2.7e8 outputs."""
    from dfx import ops
    x, b = ic.pool_inputs(H, W)
    got = ops.bias_relu_maxpool(x.cuda(), b.cuda())
    assert got.shape == (2, 3, (H + 1) // 2, (W + 1) // 2) and torch.equal(got.cpu(), ic.bias_relu_maxpool(x, b))


def test_stem_epilogue_of_maps_below_the_bias_and_of_minus_infinity():
    from dfx import ops
    for H in ic.POOL_H:
        for W in ic.POOL_W:
            x, b = ic.pool_inputs(H, W)
            low = -x.abs() - b.abs().max() - 1                     # every value below -bias: all zeros
            got = ops.bias_relu_maxpool(low.cuda(), b.cuda())
            assert got.eq(0).all() and got.numel() == 6 * ((H + 1) // 2) * ((W + 1) // 2), (H, W)
            x.view(-1)[0::3] = float("-inf")
            x[1, 2] = float("-inf")                                # a whole plane: windows of nothing but -inf
            assert torch.equal(ops.bias_relu_maxpool(x.cuda(), b.cuda()).cpu(), ic.bias_relu_maxpool(x, b)), (H, W)


# ---- add_layernorm ---------------------------------------------------------------------------------------------
def _layernorm(args):
    from dfx import ops
    x, r, gamma, beta = (None if a is None else a.float().cuda() for a in args)
    return ops.add_layernorm(x, r, dc.Norm(gamma, beta))


@pytest.mark.parametrize("family", ic.LN_FAMILIES)
@pytest.mark.parametrize("C", ic.LN_C)
def test_add_layernorm_matches_fp64_within_the_measured_yardstick(C, family):
    """Instantiations <1>, <2>, <4> (768: three chunks on <4>), partial last chunks (260, 1020), a partial last workgroup
    (1 and 5 rows), residual on and off; rows of mean 64 (a one-pass variance is ~50x off there) and rows scaled by
    2^(i-4) (a row that reads another row's statistics)."""
    for rows in ic.LN_ROWS:
        for residual in (False, True):
            case = ic.ln_case(C, rows, residual, family)
            ic.compare(f"add_layernorm C={C} rows={rows} res={int(residual)} {family}:", case, {"out": _layernorm(case["args"])})


@pytest.mark.parametrize("C", ic.LN_C)
def test_add_layernorm_exact_cases(C):
    """No residual = a zero residual; a row of one power of two gives beta (x - mean is exactly 0); permuted rows give
    permuted rows - all bit for bit."""
    x, r, gamma, beta = ic.ln_case(C, 8, True, "standard")["args"]
    plain = _layernorm((x, None, gamma, beta))
    assert torch.equal(plain, _layernorm((x, torch.zeros_like(x), gamma, beta)))
    flat = (2.0 ** (torch.arange(8.0) - 3)).view(-1, 1).expand(8, C).contiguous()
    want = beta.float().expand(8, C)
    assert torch.equal(_layernorm((flat, None, gamma, beta)).cpu(), want)
    assert torch.equal(_layernorm((flat * 0.5, flat * 0.5, gamma, beta)).cpu(), want)
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    assert torch.equal(_layernorm((x[perm], r[perm], gamma, beta)), _layernorm((x, r, gamma, beta))[perm.cuda()])


def test_add_layernorm_refuses_a_channel_count_that_is_no_multiple_of_4():
    from dfx import _lib, ops
    x = torch.randn(3, 6, device="cuda")
    norm = dc.Norm(torch.ones(6, device="cuda"), torch.zeros(6, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.add_layernorm(x, None, norm)
    out = torch.full((3, 6), 7.0, device="cuda")
    rc = _lib.load().dfx_add_layernorm_f32(x.data_ptr(), 0, norm.weight.data_ptr(), norm.bias.data_ptr(), out.data_ptr(), 3, 6,
                                          dc.EPS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and out.eq(7).all()


# ---- box_refine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_dim", ic.BOX_REF_DIMS)
@pytest.mark.parametrize("lead", [(rows,) for rows in ic.BOX_ROWS] + [(2, 150)])
def test_box_refine_matches_fp64_within_the_measured_yardstick(lead, ref_dim):
    """Row counts around the 256-row workgroup, a [2, 150, 4] shape, references beyond [0, 1] and at the eps floors from both
    sides, deltas that saturate the sigmoid; a delta that is not contiguous gives the same bits."""
    from dfx import ops
    case = ic.box_case(lead, ref_dim)
    delta, ref = (a.cuda() for a in _f32(case["args"]))
    got = ops.box_refine(delta, ref)
    assert got.shape == delta.shape
    ic.compare(f"box_refine {lead} ref_dim={ref_dim}:", case, {"out": got})
    strided = delta.movedim(-1, 0).contiguous().movedim(0, -1)
    assert not strided.is_contiguous() or delta.numel() == 4
    assert torch.equal(ops.box_refine(strided, ref), got)


def test_box_refine_exact_cases():
    """ref = 0.5 adds log(0.5 / 0.5) = 0: with delta = 0 the result is exactly 0.5; and with ref_dim = 2 the columns 2 and 3
    are sigmoid(delta) - what the same kernel gives for them with ref = 0.5 on all four columns."""
    from dfx import ops
    delta, ref = (a.cuda() for a in _f32(ic.box_case((257,), 2)["args"]))
    half = torch.full((257, 4), 0.5, device="cuda")
    assert ops.box_refine(torch.zeros(257, 4, device="cuda"), half).eq(0.5).all()
    assert ops.box_refine(torch.zeros(257, 4, device="cuda"), half[:, :2].contiguous()).eq(0.5).all()
    assert torch.equal(ops.box_refine(delta, ref)[:, 2:], ops.box_refine(delta, half)[:, 2:])


def test_box_refine_refuses_three_reference_columns():
    from dfx import ops
    with pytest.raises(RuntimeError, match="box_refine"):
        ops.box_refine(torch.zeros(5, 4, device="cuda"), torch.zeros(5, 3, device="cuda"))


# ---- group_norm ------------------------------------------------------------------------------------------------
class _GroupNorm:
    """The attributes dfx.ops reads of an nn.GroupNorm."""

    def __init__(self, weight, bias, groups):
        self.weight, self.bias, self.num_groups, self.eps = weight, bias, groups, ic.EPS


def _group_norm(x, gamma, beta, groups):
    """{y, mean, rstd} of the NCHW launch after checking that the token-major launch and ops.group_norm give the same bits."""
    from dfx import ops
    N, C, H, W = x.shape
    y, stats = ops._group_norm_forward(x, gamma, beta, groups, ic.EPS, False)
    yt, stats_t = ops._group_norm_forward(x, gamma, beta, groups, ic.EPS, True)
    assert y.shape == x.shape and yt.shape == (N, H * W, C) and stats.shape == (N * groups * 2,)
    assert torch.equal(yt.transpose(1, 2).reshape(x.shape), y) and torch.equal(stats_t, stats)
    with torch.no_grad():
        norm = _GroupNorm(gamma, beta, groups)
        assert torch.equal(ops.group_norm(x, norm), y)
        view = ops.group_norm(x, norm, tokens_out=True)
        assert view.shape == x.shape and torch.equal(view.contiguous(), y) and view.flatten(2).transpose(1, 2).is_contiguous()
    return {"y": y, "mean": stats.view(-1, 2)[:, 0], "rstd": stats.view(-1, 2)[:, 1]}


@pytest.mark.parametrize("family", ic.GN_FAMILIES)
@pytest.mark.parametrize("shape", ic.GN_SHAPES + [ic.GN_MISALIGNED])
def test_group_norm_and_its_statistics_match_fp64_within_the_measured_yardstick(shape, family):
    """y, mean and rstd (the backward consumes both), NCHW and token-major (bit-equal): the scalar statistics path by
    size (count = 70) and by alignment, three channels per group on a 96-channel map, HW = 1, one channel per group,
    one group, partial pixel tiles; maps of mean 16, where folding the mean into the bias costs the most."""
    case = ic.gn_case(shape, family)
    x, gamma, beta, groups = _f32(case["args"])
    got = _group_norm(_place(x, shape == ic.GN_MISALIGNED), gamma.cuda(), beta.cuda(), groups)
    ic.compare(f"group_norm {shape} {family}:", case, got)


@pytest.mark.parametrize("shape", ic.GN_SHAPES)
def test_group_norm_of_a_zero_map_is_the_channel_number(shape):
    """beta[c] = c on an all-zero map: y[n, c, p] == c exactly, in both layouts - a wrong channel at a transpose tile edge shows."""
    N, C, H, W, groups = shape
    gamma = torch.randn(C, generator=torch.Generator().manual_seed(C)).cuda()
    got = _group_norm(torch.zeros(N, C, H, W, device="cuda"), gamma, torch.arange(C, dtype=torch.float32, device="cuda"), groups)
    assert torch.equal(got["y"], torch.arange(C, dtype=torch.float32, device="cuda").view(1, C, 1, 1).expand(N, C, H, W))
    assert got["mean"].eq(0).all()


@pytest.mark.parametrize("shape", [(2, 96, 4, 4, 32), (2, 64, 9, 10, 1)])
def test_group_norm_of_alternating_signs(shape):
    """Pixels of +1 / -1, an even count: the mean is exactly 0, the variance exactly 1; y = x * (rstd * gamma) + beta from
    the rstd the kernel wrote, bit for bit (a product with +-1 is exact, fused or not), and that rstd is within the
    yardstick of 1 / sqrt(1 + eps)."""
    N, C, H, W, groups = shape
    g = torch.Generator().manual_seed(sum(shape))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    x = (1 - 2 * (torch.arange(H * W) % 2)).float().view(1, 1, H, W).expand(N, C, H, W).contiguous()
    got = _group_norm(x.cuda(), gamma.cuda(), beta.cuda(), groups)
    assert got["mean"].eq(0).all()
    rstd = got["rstd"].cpu()
    a = rstd.view(N, groups, 1).expand(N, groups, C // groups).reshape(N, C) * gamma
    assert torch.equal(got["y"].cpu(), x * a.view(N, C, 1, 1) + beta.view(1, C, 1, 1))
    ref = torch.tensor(1 + ic.EPS, dtype=torch.float64).rsqrt().expand(N * groups)
    case = {"ref": {"rstd": ref}, "cpu32": {"rstd": torch.tensor(1 + ic.EPS, dtype=torch.float32).rsqrt().expand(N * groups)}}
    ic.compare(f"group_norm {shape} alternating:", case, {"rstd": rstd})


# ---- dynamic_conv forward --------------------------------------------------------------------------------------
def _dynconv(t, feats=None, params=None):
    from dfx import ops
    with torch.no_grad():
        return ops._dynamic_conv_forward(t["feats"] if feats is None else feats, t["params"] if params is None else params,
                                         dc.Norm(t["g1"], t["b1"]), dc.Norm(t["g2"], t["b2"]))


def _dynconv_inputs(case):
    from tests.test_dynconv_backward_gpu import _gpu_inputs
    return _gpu_inputs(case["src"], requires=())


@pytest.mark.parametrize("K,R,extra,bias", ic.DYN_SMALL)
def test_dynamic_conv_forward_matches_fp64_within_the_measured_yardstick(K, R, extra, bias):
    """``out`` in full.  R = 1, 7, 33 (one row into the second 32-row MFMA tile), 49 | 50 (the two staging templates on
    either side of their switch), 64; one RoI; params rows inside a wider buffer; LayerNorm biases of +2, where the padded
    rows of the tiles are positive after both ReLUs."""
    case = ic.dyn_case(K, R, extra, bias)
    t = _dynconv_inputs(case)
    assert not extra or t["params"].stride(0) > 2 * dc.C * dc.DD
    ic.compare(f"dynamic_conv K={K} R={R} extra={extra} bias={bias}:", case, {"out": _dynconv(t)})


@pytest.mark.parametrize("R", ic.DYN_LARGE_R)
def test_dynamic_conv_forward_over_several_rois_per_workgroup(R):
    """min(K, 256) persistent workgroups: at 257 RoIs workgroup 0 alone prefetches and runs a second one, at 515 three
    workgroups run a third.  Every RoI of the 515 equals the K = 1 call on it alone, bit for bit (same kernel, same
    summation order per row): nothing is left in LDS or in the staging registers by the RoI before."""
    case = ic.dyn_case(ic.DYN_LARGE_K, R)
    t = _dynconv_inputs(case)
    full = None
    for K in ic.DYN_K_PREFIXES:
        full = _dynconv(t, t["feats"][:K], t["params"][:K])
        ic.compare(f"dynamic_conv K={K} R={R}:", ic.dyn_prefix(case, K), {"out": full})
    for i in ic.DYN_ALONE:
        assert torch.equal(_dynconv(t, t["feats"][i:i + 1], t["params"][i:i + 1])[0], full[i]), i


@pytest.mark.parametrize("R", [33, 50])
def test_dynamic_conv_forward_permuted_rows_give_permuted_rows(R):
    """Bit for bit: a padding row of the 64-row tiles that leaked into a kept one would depend on where that row lies."""
    t = _dynconv_inputs(ic.dyn_case(5, R))
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(R)).cuda()
    assert torch.equal(_dynconv(t, t["feats"][:, perm].contiguous()), _dynconv(t)[:, perm])
