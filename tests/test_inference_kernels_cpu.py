"""CPU: the restatements of tests/_inference_kernel_cases.py against torch's own functionals in fp64, and the conditions
that make the GPU bound of tests/test_inference_kernels_gpu.py mean something: every yardstick case has room under
4 x (two independent fp32 evaluations within a factor 2 of each other), the arithmetic form of gn_apply fits under it,
and wrong kernels - a one-pass variance, a skipped partial chunk / tile / row / RoI - do not."""
import pytest
import torch
import torch.nn.functional as F

from tests import _dynconv_cases as dc
from tests import _inference_kernel_cases as ic

FP64_AGREEMENT = 1e-12       # two fp64 evaluations of these short computations (relative to the largest magnitude)

LN_GRID = [(C, rows, res, fam) for fam in ic.LN_FAMILIES for C in ic.LN_C for rows in ic.LN_ROWS for res in (False, True)]
GN_GRID = [(shape, fam) for fam in ic.GN_FAMILIES for shape in ic.GN_SHAPES + [ic.GN_MISALIGNED]]
BOX_GRID = [((rows,), rd) for rows in ic.BOX_ROWS for rd in ic.BOX_REF_DIMS] + [((2, 150), 4), ((2, 150), 2)]


def _fails(bad, case, k):
    return ic.rel_err(bad, case["ref"][k]) > ic.YARDSTICK_FACTOR * ic.yardstick(case["cpu32"][k], case["ref"][k])


# ---- restatements against torch in fp64 ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,_", ic.BIAS_ACT_CASES)
def test_bias_act_restatement_is_frozen_bn_bias_residual_relu(shape, _):
    x, b, r = (t.double() for t in ic.bias_act_inputs(shape))
    bias = b.view(1, -1, *([1] * (x.dim() - 2)))
    assert torch.equal(ic.bias_act(x, b, r, True), F.relu(x + bias + r))
    assert torch.equal(ic.bias_act(x, b, None, True), F.relu(x + bias))
    assert torch.equal(ic.bias_act(x, b, r, False), x + bias + r)
    assert torch.equal(ic.bias_act(x, b, None, False), x + bias)


@pytest.mark.parametrize("H", ic.POOL_H)
@pytest.mark.parametrize("W", ic.POOL_W)
def test_pool_restatement_is_max_pool2d_of_relu(H, W):
    x, b = (t.double() for t in ic.pool_inputs(H, W))
    assert torch.equal(ic.bias_relu_maxpool(x, b), F.max_pool2d(F.relu(x + b.view(1, -1, 1, 1)), 3, 2, 1))


@pytest.mark.parametrize("C,rows,res,fam", LN_GRID)
def test_layernorm_restatement_is_layer_norm(C, rows, res, fam):
    case = ic.ln_case(C, rows, res, fam)
    want = ic.add_layernorm_functional(*case["args"])["out"]
    assert ic.rel_err(case["ref"]["out"], want) < FP64_AGREEMENT


@pytest.mark.parametrize("lead,rd", BOX_GRID)
def test_box_restatement_is_inverse_sigmoid_then_sigmoid(lead, rd):
    case = ic.box_case(lead, rd)
    want = ic.box_refine_functional(*case["args"])["out"]
    assert want.shape == (*lead, 4) and ic.rel_err(case["ref"]["out"], want) < FP64_AGREEMENT
    if lead[-1] > 35:       # the planted rows are there: every special reference met every special delta
        delta, ref = case["args"]
        seen = {(float(r), float(d)) for r, d in zip(ref.reshape(-1, rd)[:35, 0].float(), delta.reshape(-1, 4)[:35, 0])}
        assert len(seen) == len(ic.BOX_REFS) * len(ic.BOX_DELTAS)


@pytest.mark.parametrize("shape,fam", GN_GRID)
def test_group_norm_restatement_is_group_norm(shape, fam):
    case = ic.gn_case(shape, fam)
    x, gamma, beta, groups = case["args"]
    assert ic.rel_err(case["ref"]["y"], F.group_norm(x, groups, gamma, beta, ic.EPS)) < FP64_AGREEMENT
    alt = ic.group_norm_functional(*case["args"])
    for k in ("mean", "rstd"):
        assert ic.rel_err(case["ref"][k], alt[k]) < FP64_AGREEMENT, k


@pytest.mark.parametrize("K,R,extra,bias", ic.DYN_SMALL)
def test_dynconv_plain_is_bmm_layernorm_relu(K, R, extra, bias):
    src = ic.dyn_case(K, R, extra, bias)["src"]
    a64 = tuple(src[k].double() for k in dc.OUTPUTS)
    assert ic.rel_err(ic.dynconv_plain(*a64), dc.forward_stages(*a64)[2]) < FP64_AGREEMENT


# ---- room under the bound --------------------------------------------------------------------------------------
def _room(case):
    for k, ref in case["ref"].items():
        a, b = ic.yardstick(case["cpu32"][k], ref), ic.yardstick(case["alt32"][k], ref)
        print(f"  {k}: restatement {a:.3e}, torch {b:.3e} (seed {case['seed']})")
        assert max(a, b) <= 2 * min(a, b), k
    for t in case.get("args", ()):
        if torch.is_tensor(t):      # fp32-representable inputs
            assert t.dtype == torch.float64 and torch.equal(t.float().double(), t)


@pytest.mark.parametrize("C,rows,res,fam", LN_GRID)
def test_layernorm_cases_leave_room_under_the_bound(C, rows, res, fam):
    _room(ic.ln_case(C, rows, res, fam))


@pytest.mark.parametrize("lead,rd", BOX_GRID)
def test_box_cases_leave_room_under_the_bound(lead, rd):
    _room(ic.box_case(lead, rd))


@pytest.mark.parametrize("shape,fam", GN_GRID)
def test_group_norm_cases_leave_room_under_the_bound(shape, fam):
    _room(ic.gn_case(shape, fam))


@pytest.mark.parametrize("K,R,extra,bias", ic.DYN_SMALL + [(ic.DYN_LARGE_K, R, 0, None) for R in ic.DYN_LARGE_R])
def test_dynconv_cases_leave_room_under_the_bound(K, R, extra, bias):
    case = ic.dyn_case(K, R, extra, bias)
    _room(case)
    if K == ic.DYN_LARGE_K:
        for k in ic.DYN_K_PREFIXES:
            _room(dict(ic.dyn_prefix(case, k), seed=case["seed"]))


# ---- the kernel's arithmetic form ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ic.GN_SHAPES + [ic.GN_MISALIGNED])
def test_folded_mean_form_of_gn_apply_fits_under_the_bound_at_large_mean(shape):
    """x * a + (beta - mean * a) in fp32 on the CPU: its rounding error grows with |mean| / std, and at mean 16 it stays under
    4 x the yardstick of the plain form."""
    case = ic.gn_case(shape, "large_mean")
    ref = case["ref"]["y"]
    form = ic.rel_err(ic.group_norm_kernel_form(*ic.cast(case["args"], torch.float32))["y"], ref)
    yard = ic.yardstick(case["cpu32"]["y"], ref)
    print(f"  folded form {form:.3e}, plain form {yard:.3e}")
    assert form <= ic.YARDSTICK_FACTOR * yard


# ---- teeth -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,rows,res", [(C, rows, res) for C in ic.LN_C for rows in ic.LN_ROWS for res in (False, True)])
def test_one_pass_layernorm_fails_the_bound_at_large_mean(C, rows, res):
    case = ic.ln_case(C, rows, res, "large_mean")
    bad = ic.add_layernorm_one_pass(*ic.cast(case["args"], torch.float32))["out"]
    print(f"  one pass {ic.rel_err(bad, case['ref']['out']):.3e}, two pass {ic.yardstick(case['cpu32']['out'], case['ref']['out']):.3e}")
    assert _fails(bad, case, "out")


@pytest.mark.parametrize("shape", ic.GN_SHAPES + [ic.GN_MISALIGNED])
def test_one_pass_group_norm_fails_the_bound_at_large_mean(shape):
    case = ic.gn_case(shape, "large_mean")
    bad = ic.group_norm_one_pass(*ic.cast(case["args"], torch.float32))
    print(f"  one pass y {ic.rel_err(bad['y'], case['ref']['y']):.3e}, rstd {ic.rel_err(bad['rstd'], case['ref']['rstd']):.3e}")
    assert _fails(bad["y"], case, "y") and _fails(bad["rstd"], case, "rstd")


@pytest.mark.parametrize("C,rows,res,fam", LN_GRID)
def test_layernorm_without_its_partial_pieces_fails(C, rows, res, fam):
    case = ic.ln_case(C, rows, res, fam)
    bad = ic.ln_drop_partial(case["cpu32"]["out"], C, rows)
    assert (bad is None) == (rows % 4 == 0 and (C <= 256 or C % 256 == 0))
    assert bad is None or _fails(bad, case, "out")


@pytest.mark.parametrize("shape,fam", GN_GRID)
def test_group_norm_without_its_partial_tiles_fails(shape, fam):
    case = ic.gn_case(shape, fam)
    bad = ic.gn_drop_partial(case["cpu32"]["y"], shape)
    assert (bad is None) == (shape[1] % 64 == 0 and (shape[2] * shape[3]) % 64 == 0)
    assert bad is None or _fails(bad, case, "y")


@pytest.mark.parametrize("lead,rd", BOX_GRID)
def test_box_refine_without_its_last_row_fails(lead, rd):
    case = ic.box_case(lead, rd)
    bad = case["cpu32"]["out"].clone()
    bad.reshape(-1, 4)[-1] = 0
    assert _fails(bad, case, "out")


@pytest.mark.parametrize("K,R,extra,bias", ic.DYN_SMALL)
def test_dynconv_without_its_last_row_or_roi_fails(K, R, extra, bias):
    case = ic.dyn_case(K, R, extra, bias)
    for cut in ((slice(None), R - 1), (K - 1, slice(None))):
        bad = case["cpu32"]["out"].clone()
        bad[cut] = 0
        assert _fails(bad, case, "out")
