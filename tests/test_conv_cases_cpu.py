"""No GPU: the cases, yardsticks and host-arithmetic mirrors of tests/_conv_cases.py, held against fp64 F.conv2d, against the
figures the GPU tests name their cases for, and the batch ranges of dfx.ops.ConvPlan."""
import pytest
import torch

from tests import _conv_cases as cc


def _wino_geom(c):
    N, Ci, Co, H, W, dil = c
    return (N, Ci, Co, H, W, 3, 3, 1, dil, dil)


def _tile_geom(c):
    N, Ci, Co, H, W, k, stride, pad = c
    return (N, Ci, Co, H, W, k, k, stride, pad, 1)


def _walk_geoms(cus=32):
    """(the image count of a 32-CU device keeps the fp32 sums quick; test_exact_direct_cases_are_exact_in_fp32 says why the
    count does not matter)"""
    return [(cc.walk_images(cus, H, W, k, s, p), Ci, Co, H, W, k, k, s, p, 1)
            for (Ci, Co, k, s, p) in cc.WALK_CONVS for (H, W) in cc.WALK_MAPS]


# ---- the yardsticks compute the convolution ------------------------------------------------------------------------------
SMALL_WINO = [c for c in cc.WINO_EXACT if c[3] * c[4] < 1000] + [(2, 64, 64, 25, 41, 1)]


@pytest.mark.parametrize("c", SMALL_WINO)
@pytest.mark.parametrize("act", [None, "relu", "gelu"])
def test_wino_yardstick_in_fp64_is_the_convolution(c, act):
    case = cc.make_real_case(*_wino_geom(c), act=act)
    ref = cc.reference(case)
    assert cc.wino_yardstick(case, torch.float64).shape == ref.shape
    assert cc.rel_err(cc.wino_yardstick(case, torch.float64), ref) <= 1e-12
    assert cc.rel_err(cc.direct_yardstick(case, torch.float64), ref) <= 1e-12


@pytest.mark.parametrize("geom", cc.IGEMM_EXACT + [_tile_geom(c) for c, _ in cc.TILE_EXACT])
def test_direct_yardstick_in_fp64_is_the_convolution(geom):
    case = cc.make_real_case(*geom, act="gelu")
    ref = cc.reference(case)
    assert cc.direct_yardstick(case, torch.float64).shape == ref.shape
    assert cc.rel_err(cc.direct_yardstick(case, torch.float64), ref) <= 1e-12


def test_real_cases_are_fp32_representable_non_negative_and_off_centre():
    case = cc.make_real_case(2, 16, 64, 9, 11)
    for n in ("x", "weight", "bias", "scale"):
        assert torch.equal(case[n], case[n].float().double()), n
    assert case["x"].min().item() >= 0 and case["x"].mean().item() > 1.0
    assert 0.5 <= case["scale"].min().item() and case["scale"].max().item() < 1.5


# ---- the integer recipe stays exact in fp32: a condition on the inputs, not on a kernel -----------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("c", cc.WINO_EXACT + [cc.WINO_SPLIT])
def test_exact_winograd_cases_are_exact_in_fp32(c, scale):
    """fp32 Winograd - transforms, the 0.5 factors, sums over the channels - equals fp64 conv2d bit for bit, so does the
    direct fp32 sum (the implicit GEMM's arithmetic on the same operands); the batch-split case included"""
    case, ref = cc.exact_prepared(_wino_geom(c), True, scale)
    assert ref.abs().max().item() < 2 ** 24 and torch.equal(ref, ref.round())
    assert torch.equal(cc.wino_yardstick(case).double(), ref)
    assert torch.equal(cc.direct_yardstick(case).double(), ref)


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("geom", cc.IGEMM_EXACT + [_tile_geom(c) for c, _ in cc.TILE_EXACT] + [_tile_geom(cc.TILE_SPLIT)]
                         + _walk_geoms())
def test_exact_direct_cases_are_exact_in_fp32(geom, scale):
    """The persistent-walk cases run on the GPU with an image count taken from the device; here with a smaller one.  The
    count does not matter: whatever the operands of the recipe, no partial sum of an output exceeds
    kh * kw * Ci * 3 * 16 + 9 (|x| <= 3, |weight * scale| <= 16, |bias| <= 9), an integer far below 2^24 - asserted too."""
    N, Ci, Co, H, W, kh, kw, stride, pad, dil = geom
    assert kh * kw * Ci * 3 * 16 + 9 < 2 ** 24
    case, ref = cc.exact_prepared(geom, True, scale)
    assert ref.abs().max().item() <= kh * kw * Ci * 3 * 16 + 9 and torch.equal(ref, ref.round())
    assert torch.equal(cc.direct_yardstick(case).double(), ref)
    assert ref.numel() < 16 or ((ref < 0).any() and (ref > 0).any())      # a ReLU has something to clamp and to keep


@pytest.mark.parametrize("name", sorted(cc.CLIP_SLICES))
def test_exact_channel_slice_cases_are_exact_in_fp32(name):
    clip, case = cc.make_clip_case(name)
    sl = cc.CLIP_SLICES[name]
    assert set(clip.flatten().tolist()) <= set(range(-3, 4)) and torch.equal(case["x"], clip[:, sl])
    ref = cc.reference(case)
    assert torch.equal(cc.direct_yardstick(case).double(), ref) and torch.equal(ref, ref.round())


def test_exact_operands_are_the_stated_integers():
    for scale in (False, True):
        case = cc.make_exact_case(2, 8, 64, 5, 7, bias=True, scale=scale)
        assert set(case["x"].flatten().tolist()) <= set(range(-3, 4))
        assert set(case["weight"].flatten().tolist()) <= ({-8.0, 0.0, 8.0} if scale else {-8.0, -4.0, 0.0, 4.0, 8.0})
        assert torch.equal(case["bias"], case["bias"].round())
        assert (case["scale"] is None) == (not scale)
        if scale:
            assert set(case["scale"].tolist()) <= {0.5, 1.0, 2.0}
    assert cc.make_exact_case(2, 8, 64, 5, 7, bias=False)["bias"] is None
    a, b = cc.make_exact_case(2, 8, 64, 5, 7), cc.make_exact_case(2, 8, 64, 5, 7)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["weight"], b["weight"])         # seeded from the shape


def test_a_wrong_tap_changes_an_exact_result():
    """the exact comparison has teeth: one input moved by one changes an integer of the reference"""
    case, ref = cc.exact_prepared(_wino_geom((3, 72, 64, 11, 13, 1)), True, False)
    other = dict(case, x=case["x"].clone())
    other["x"][1, 40, 5, 6] += 1
    assert not torch.equal(cc.reference(other), ref)
    assert "outputs differ" in cc.describe_mismatch(cc.reference(other), ref)
    assert cc.describe_mismatch(ref, ref) == "equal"


# ---- mirrors of the host arithmetic ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cc.WINO_EXACT)
def test_wino_launches_returns_the_regime_the_case_is_named_for(c):
    assert cc.wino_launches(*c) == cc.WINO_REGIMES[c]
    if c in cc.WINO_REGIMES_NO_TAIL:
        assert cc.wino_launches(*c, no_tail=True) == cc.WINO_REGIMES_NO_TAIL[c]
    else:
        assert cc.wino_launches(*c, no_tail=True) == [("full", cc.WINO_REGIMES[c][0][1])]


def test_wino_launches_rule_edges():
    # 64 tiles per block: an N x 1 x 1 map has N tiles; Co = 64: one channel block
    def blocks(n):
        return cc.wino_launches(64 * n, 8, 64, 1, 1, 1)
    assert blocks(160) == [("quarter", 160)]
    assert blocks(161) == [("full", 161)]
    assert blocks(256) == [("full", 256)]
    assert blocks(256 + 160) == [("full", 256), ("quarter", 160)]
    assert blocks(256 + 161) == [("full", 417)]
    assert blocks(525) == [("full", 512), ("quarter", 13)]
    # the workload's cases that tests/test_conv_gpu.py names: 525 and 276 blocks
    assert cc.wino_launches(8, 64, 64, 100, 167, 1) == [("full", 512), ("quarter", 13)]
    assert cc.wino_launches(4, 256, 256, 50, 84, 2) == [("full", 256), ("quarter", 20)]
    assert cc.wino_blocks_of_record(150 * 2 * 16 * 64 * 8 * 64, 8) == 150


@pytest.mark.parametrize("c,name", cc.TILE_EXACT)
def test_tile_template_of_the_exact_cases(c, name):
    N, Ci, Co, H, W, k, stride, pad = c
    assert cc.tile_template(Ci, Co, k, stride) == name


def test_tile_template_of_the_workload_and_all_three_are_named():
    assert cc.tile_template(3, 64, 7, 2) == "2,9"           # the ResNet stem
    assert cc.tile_template(1, 16, 3, 2) == "1,3"           # the DFormer stem's first convolution
    assert cc.tile_template(3, 32, 7, 2) == "1,9"
    assert {n for _, n in cc.TILE_EXACT} == {"1,3", "1,9", "2,9"}
    for Ci, Co, k, s, p in cc.WALK_CONVS:
        assert cc.tile_template(Ci, Co, k, s) in ("1,3", "2,9")


def test_walk_cases_have_partial_tiles_on_both_axes_and_enough_of_them():
    for Ci, Co, k, s, p in cc.WALK_CONVS:
        for H, W in cc.WALK_MAPS:
            Ho, Wo = cc.out_size(H, W, k, k, s, p, 1)
            assert Ho % 8 and Wo % 32 and Ho > 8 and Wo > 32
            for cus in (256, 304, 64):
                assert cc.walk_images(cus, H, W, k, s, p) * ((Ho + 7) // 8) * ((Wo + 31) // 32) >= 2.5 * 4 * cus


@pytest.mark.parametrize("conv", cc.WALK_CONVS)
def test_walk_cases_fire_both_carries_on_a_256_cu_device(conv):
    """What makes the walk more than a step from image to image: the grid is no multiple of the tiles per image, so
    ``advance`` moves the tile column and the tile row and carries out of both.  The 2 x 2-tile maps do not (stated, so that
    nobody takes them for more than they are); the 3 x 3-tile maps do, in every workgroup for the column or the row and in
    some workgroups for both."""
    Ci, Co, k, s, p = conv
    grid = {(1, 16, 3, 2, 1): 1024, (3, 64, 7, 2, 3): 512}[conv]          # 4 and 2 workgroups per CU (11.7 and 78.2 KB of LDS)
    for H, W in cc.WALK_MAPS:
        N = cc.walk_images(cc.MI355X_CUS, H, W, k, s, p)
        w = cc.tile_walk(cc.MI355X_CUS, N, Ci, Co, H, W, k, s, p)
        assert w["grid"] == grid and w["tiles"] >= 2.5 * grid and w["lds"] * w["per_cu"] <= 160 * 1024
        assert w["grid"] == (w["d_n"] * w["TY"] + w["d_ty"]) * w["TX"] + w["d_tx"]
        if (H, W) in cc.WALK_CARRY_MAPS:
            assert (w["TY"], w["TX"]) == (3, 3) and w["d_ty"] != 0 and w["d_tx"] != 0
            assert w["column_carry"] > 0 and w["row_carry"] > 0 and w["both_carries"] > 0
            print(f"  {conv} {H}x{W}: N {N}, {w}")
        else:
            assert (w["TY"], w["TX"], w["d_ty"], w["d_tx"], w["column_carry"], w["row_carry"]) == (2, 2, 0, 0, 0, 0)
    assert cc.tile_walk(cc.MI355X_CUS, 285, 3, 64, 36, 140, 7, 2, 3)["lds"] == 78160


# ---- ConvPlan's batch ranges (dfx.ops._conv_batch_ranges: pure) -----------------------------------------------------------
def test_conv_batch_ranges():
    from dfx import ops
    r = ops._conv_batch_ranges
    wino, tile = ops.ConvPlan.WINO_MAX_ELEMENTS, ops.ConvPlan.TILE_MAX_ELEMENTS
    assert (wino, tile) == (1 << 30, (1 << 30) - 4)
    # an empty batch: no launch, whatever the algorithm (a step of 0 used to reach range())
    for algo, limit in (("wino", wino), ("tile", tile), ("igemm", None)):
        assert r(algo, 0, 8 * 5 * 7, 0, limit) == []
        assert r(algo, 3, 8 * 5 * 7, 0, limit) == [(0, 3)]
    # Winograd: whole images below the limit
    per = 8 * 9 * 10
    assert r("wino", 5, per, 0, 2 * per + 1) == [(0, 2), (2, 4), (4, 5)]
    assert r("wino", 5, per, 0, 5 * per + 1) == [(0, 5)]
    assert r("wino", 5, per, 0, 5 * per) == [(0, 4), (4, 5)]
    assert r("wino", 2, per, 0, per) == [(0, 1), (1, 2)]            # an image larger than the limit still goes alone
    assert r("wino", 4, 1 << 28, 0, wino) == [(0, 3), (3, 4)]
    # tile: the image stride of a channel slice counts
    assert r("tile", 5, per, 0, 2 * per) == [(0, 2), (2, 4), (4, 5)]
    assert r("tile", 5, per, 4 * per // 3, 2 * per) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert r("tile", 5, per, 4 * per // 3, 3 * per) == [(0, 2), (2, 4), (4, 5)]
    assert r("tile", 3, per, 0, 1) == [(0, 1), (1, 2), (2, 3)]
    assert r("tile", 4, 3 * 800 * 1333, 4 * 800 * 1333, tile) == [(0, 4)]
    # the implicit GEMM never splits
    assert r("igemm", 70000, per, 0, None) == [(0, 70000)]
