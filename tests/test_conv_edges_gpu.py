"""GPU: the three hand-written convolutions behind dfx.ops.ConvPlan at the launch regimes, templates and geometry edges that
the workload's shapes (tests/test_conv_gpu.py) do not reach - tests/_conv_cases.py has the cases and says why.

  exact      integer-valued operands: the result must EQUAL fp64 F.conv2d (torch.equal, no tolerance); which kernel ran is
             read from the launch records (ops.profile_start / profile_stop), so a case that silently takes another route fails
  realistic  non-negative inputs with non-zero means against the CPU's own fp32 error in the kernel's order of summation
             (YARDSTICK_FACTOR x), both figures printed
  host       empty batches and the two batch splits of ConvPlan.__call__
A failed exact comparison reports which outputs differ (images, channels, rows / columns and their parities: the position in
the 2x2 Winograd tile), under the switch named in the test id."""
import itertools

import pytest
import torch

from tests import _conv_cases as cc

pytestmark = pytest.mark.gpu

FLAGS = list(itertools.product((True, False), (False, True)))         # (bias, scale)


def _gpu(t):
    return None if t is None else t.float().cuda()


def _plan(case, algo=None):
    from dfx import ops
    return ops.ConvPlan(_gpu(case["weight"]), _gpu(case["bias"]), case["stride"], case["pad"], case["dil"], case["act"],
                        scale=_gpu(case["scale"]), algo=algo)


def _assert_exact(got, want, what):
    assert tuple(got.shape) == tuple(want.shape), what
    g = got.double().cpu()
    if not torch.equal(g, want):
        pytest.fail(f"{what}: {cc.describe_mismatch(g, want)}")


def _recorded(plan, x):
    """(result, launch records) of one call"""
    from dfx import ops
    torch.cuda.synchronize()
    ops.profile_start()
    try:
        got = plan(x)
        torch.cuda.synchronize()
    finally:
        recs = ops.profile_stop()
    return got, recs


def _wino_geom(c):
    N, Ci, Co, H, W, dil = c
    return (N, Ci, Co, H, W, 3, 3, 1, dil, dil)


def _tile_geom(c):
    N, Ci, Co, H, W, k, stride, pad = c
    return (N, Ci, Co, H, W, k, k, stride, pad, 1)


def _wino_blocks(recs, Ci):
    return [cc.wino_blocks_of_record(r[1], Ci) for r in recs if r[2] == -3]


# ---- 2.1 Winograd, exact -------------------------------------------------------------------------------------------------
def _wino_id(c, phase, no_tail):
    regime = "+".join(f"{k}{n}" for k, n in cc.wino_launches(*c, no_tail=no_tail))
    switch = {None: "rule", "0": "phased", "1": "unphased"}[phase]
    return f"{'x'.join(map(str, c))}-{c[1] // 8}chunks-{regime}-{switch}{'-notail' if no_tail else ''}"


WINO_RUNS = []
for _c in cc.WINO_EXACT:                                    # case-major: the cached references of a case serve its runs
    WINO_RUNS += [(_c, ph, False) for ph in (None, "0", "1")]
    if _c in cc.WINO_MULTI_ROUND:
        WINO_RUNS.append((_c, None, True))


@pytest.mark.parametrize("c,phase,no_tail", WINO_RUNS, ids=[_wino_id(*r) for r in WINO_RUNS])
def test_winograd_exact(c, phase, no_tail, dfx_env):
    """Both workgroup sizes (full = <2,2>, quarter = <1,1>), the K loop with and without the phase shift of waves 4-7 at 1, 2,
    3 and 9 chunks, remainders 0, 150 and 163 of the 256 / 160 launch rule, DFX_WINO_NO_TAIL, maps of one pixel and smaller
    than the dilation; each with and without bias and scale, with and without ReLU.
    What the records pin: the number of launches and the logical blocks of each.  The two kernels differ in nothing else a
    record holds, so a single launch of 163 (or of 1) block is told apart from the other workgroup size only by the host rule
    mirrored in cc.wino_launches; the 256 + 150 case, two launches, is the one whose records show both kinds at work."""
    N, Ci, Co, H, W, dil = c
    dfx_env("DFX_WINO_NO_PHASE", phase)
    dfx_env("DFX_WINO_NO_TAIL", "1" if no_tail else None)
    want_launches = cc.wino_launches(*c, no_tail=no_tail)
    assert want_launches == (cc.WINO_REGIMES_NO_TAIL if no_tail else cc.WINO_REGIMES)[c]
    for bias, scale in FLAGS:
        case, ref = cc.exact_prepared(_wino_geom(c), bias, scale)
        x = _gpu(case["x"])
        for act in (None, "relu"):
            plan = _plan(cc.with_act(case, act))
            assert plan.algo == "wino"
            got, recs = _recorded(plan, x)
            what = f"wino {c} bias={bias} scale={scale} act={act}"
            assert _wino_blocks(recs, Ci) == [n for _, n in want_launches], what
            assert len(recs) == len(want_launches), what
            _assert_exact(got, ref.relu() if act else ref, what)


# ---- 2.2 implicit GEMM, exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", cc.IGEMM_EXACT, ids=["x".join(map(str, g)) for g in cc.IGEMM_EXACT])
def test_igemm_exact(geom):
    """kh != kw, 64 taps, padding beyond the kernel's reach, stride 3 with dilation 2 through the uniform-tap (Ci = 16) and the
    general (Ci = 17) template, a single K-step, the float4 and the scalar epilogue"""
    N, Ci, Co, H, W, kh, kw, stride, pad, dil = geom
    for bias, scale in FLAGS:
        case, ref = cc.exact_prepared(geom, bias, scale)
        x = _gpu(case["x"])
        for act in (None, "relu"):
            plan = _plan(cc.with_act(case, act), algo="igemm")
            assert plan.algo == "igemm"
            got, recs = _recorded(plan, x)
            what = f"igemm {geom} bias={bias} scale={scale} act={act}"
            assert [(r[2], r[1]) for r in recs] == [(-4, 2 * Co * plan.Kpad * ref.shape[2] * ref.shape[3] * N)], what
            _assert_exact(got, ref.relu() if act else ref, what)


def test_igemm_border_outputs_beyond_the_kernels_reach_are_the_bias():
    geom = (1, 16, 64, 5, 6, 3, 3, 1, 3, 1)
    case, ref = cc.exact_prepared(geom, True, False)
    got = _plan(case, algo="igemm")(_gpu(case["x"])).cpu()
    assert tuple(got.shape) == (1, 64, 9, 10)
    border = torch.ones(9, 10, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert torch.equal(got[0][:, border].double(), case["bias"].view(-1, 1).expand(-1, int(border.sum())))


@pytest.mark.parametrize("name", sorted(cc.CLIP_SLICES))
def test_igemm_exact_on_a_channel_slice_read_in_place(name):
    clip, case = cc.make_clip_case(name)
    sl = cc.CLIP_SLICES[name]
    x = _gpu(clip)[:, sl]
    assert not x.is_contiguous()
    _assert_exact(_plan(case, algo="igemm")(x), cc.reference(case), f"igemm on clip[:, {sl}]")


# ---- 2.3 tile kernel, exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,template", cc.TILE_EXACT, ids=[f"{'x'.join(map(str, c))}-MT{t[0]}-NS{t[2]}" for c, t in cc.TILE_EXACT])
def test_tile_exact_on_every_template(c, template):
    """conv_tile_kernel<1,3>, <1,9> (Co <= 32 with more than three staged elements per thread) and <2,9>"""
    N, Ci, Co, H, W, k, stride, pad = c
    assert cc.tile_template(Ci, Co, k, stride) == template
    for bias, scale in FLAGS:
        case, ref = cc.exact_prepared(_tile_geom(c), bias, scale)
        x = _gpu(case["x"])
        for act in (None, "relu"):
            plan = _plan(cc.with_act(case, act))
            assert plan.algo == "tile"
            got, recs = _recorded(plan, x)
            what = f"tile {c} <{template}> bias={bias} scale={scale} act={act}"
            assert [(r[2], r[3]) for r in recs] == [(-4, 16)], what
            _assert_exact(got, ref.relu() if act else ref, what)
            assert torch.equal(got, _plan(cc.with_act(case, act), algo="igemm")(x)), what


WALKS = [(conv, hw) for conv in cc.WALK_CONVS for hw in cc.WALK_MAPS]


@pytest.mark.parametrize("conv,hw", WALKS, ids=[f"{c[0]}to{c[1]}-{c[2]}x{c[2]}s{c[3]}-map{h}x{w}" for c, (h, w) in WALKS])
def test_tile_persistent_walk_exact(conv, hw):
    """Many small images: at least 2.5 tiles per workgroup of the largest grid the kernel takes (4 per CU), so every workgroup
    walks several tiles and stages the next one while it computes; partial tiles on both axes.  On the 2 x 2-tile maps the
    grid of a 256-CU device is a multiple of the tiles per image: a workgroup only moves from image to image on one tile.
    On the 3 x 3-tile maps (cc.WALK_CARRY_MAPS) every step also moves the tile column and the tile row, and both scalar
    carries of ``advance`` fire (cc.tile_walk mirrors the kernel's walk; asserted for the device at hand)."""
    (Ci, Co, k, stride, pad), (H, W) = conv, hw
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = cc.walk_images(cus, H, W, k, stride, pad)
    if hw in cc.WALK_CARRY_MAPS:
        w = cc.tile_walk(cus, N, Ci, Co, H, W, k, stride, pad)
        assert w["d_tx"] != 0 and w["d_ty"] != 0 and w["column_carry"] > 0 and w["row_carry"] > 0 and w["both_carries"] > 0, w
    geom = (N, Ci, Co, H, W, k, k, stride, pad, 1)
    case, ref = cc.exact_prepared(geom, True, False)
    Ho, Wo = ref.shape[2:]
    assert N * ((Ho + 7) // 8) * ((Wo + 31) // 32) >= 2.5 * 4 * cus and Ho % 8 and Wo % 32
    x = _gpu(case["x"])
    for act in (None, "relu"):
        plan = _plan(cc.with_act(case, act))
        assert plan.algo == "tile"
        got, recs = _recorded(plan, x)
        what = f"tile walk {geom} act={act}"
        assert [(r[2], r[3]) for r in recs] == [(-4, 16)], what
        _assert_exact(got, ref.relu() if act else ref, what)
        assert torch.equal(got, _plan(cc.with_act(case, act), algo="igemm")(x)), what


# ---- 2.4 realistic values against the measured yardstick -------------------------------------------------------------
REAL = [  # algo, geometry (N, Ci, Co, H, W, kh, kw, stride, pad, dil), activation
    ("wino", (3, 72, 64, 11, 13, 3, 3, 1, 1, 1), "gelu"),
    ("wino", (1, 24, 128, 9, 10, 3, 3, 1, 2, 2), "relu"),
    ("wino", (2, 64, 64, 25, 41, 3, 3, 1, 1, 1), None),
    ("igemm", (2, 16, 40, 17, 19, 3, 3, 3, 2, 2), "gelu"),
    ("igemm", (2, 5, 24, 14, 9, 5, 2, 2, 1, 1), "relu"),
    ("tile", (2, 3, 32, 30, 45, 7, 7, 2, 3, 1), "gelu"),
]


@pytest.mark.parametrize("algo,geom,act", REAL, ids=[f"{a}-{'x'.join(map(str, g))}-{t}" for a, g, t in REAL])
def test_realistic_values_within_the_cpu_fp32_yardstick(algo, geom, act):
    case, ref, yard = cc.real_prepared(geom, act, algo)
    plan = _plan(case, algo=algo)
    assert plan.algo == algo
    got = plan(_gpu(case["x"])).cpu()
    assert tuple(got.shape) == tuple(ref.shape)
    y, err = cc.rel_err(yard, ref), cc.rel_err(got, ref)
    print(f"  {algo} {geom} {act}: cpu fp32 yardstick {y:.3e}, gpu {err:.3e}, ratio {err / y if y else float('nan'):.2f}, "
          f"max |ref| {ref.abs().max().item():.3e}")
    assert err <= cc.YARDSTICK_FACTOR * y, f"{algo} {geom} {act}: gpu {err:.3e} > {cc.YARDSTICK_FACTOR} x {y:.3e}"


# ---- 2.5 host paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,wshape,stride,pad", [("wino", (64, 8, 3, 3), 1, 1), ("igemm", (8, 5, 3, 3), 2, 1),
                                                    ("tile", (16, 1, 3, 3), 2, 1)], ids=["wino", "igemm", "tile"])
def test_an_empty_batch_gives_an_empty_result_and_no_launch(algo, wshape, stride, pad):
    from dfx import ops
    w = torch.ones(wshape).cuda()
    plan = ops.ConvPlan(w, torch.ones(wshape[0]).cuda(), stride, pad, 1, "relu", algo=algo)
    assert plan.algo == algo
    x = torch.ones(2, wshape[1], 9, 12).cuda()
    got, recs = _recorded(plan, x[:0])
    Ho, Wo = cc.out_size(9, 12, 3, 3, stride, pad, 1)
    assert tuple(got.shape) == (0, wshape[0], Ho, Wo) and got.dtype == torch.float32 and got.is_cuda
    assert recs == []
    assert tuple(plan(x).shape) == (2, wshape[0], Ho, Wo)


def test_winograd_batch_split_at_the_element_limit(monkeypatch):
    """ConvPlan.WINO_MAX_ELEMENTS lowered to two images and one element: five images go as 2 + 2 + 1"""
    from dfx import ops
    c = cc.WINO_SPLIT
    N, Ci, Co, H, W, dil = c
    case, ref = cc.exact_prepared(_wino_geom(c), True, True)
    plan, x = _plan(case), _gpu(case["x"])
    assert plan.algo == "wino"
    whole, recs = _recorded(plan, x)
    assert _wino_blocks(recs, Ci) == [n for _, n in cc.wino_launches(*c)]
    monkeypatch.setattr(ops.ConvPlan, "WINO_MAX_ELEMENTS", 2 * Ci * H * W + 1)
    split, recs = _recorded(plan, x)
    want = [n for imgs in (2, 2, 1) for _, n in cc.wino_launches(imgs, Ci, Co, H, W, dil)]
    assert _wino_blocks(recs, Ci) == want and len(want) == 3
    _assert_exact(split, ref, "wino in three image ranges")
    assert torch.equal(split, whole)


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "channel-slice"])
def test_tile_batch_split_at_the_element_limit(monkeypatch, sliced):
    """ConvPlan.TILE_MAX_ELEMENTS lowered to two image strides: five images go as 2 + 2 + 1, also when the images are the RGB
    planes of a wider clip (the image stride exceeds Ci * H * W and is what counts)"""
    from dfx import ops
    N, Ci, Co, H, W, k, stride, pad = cc.TILE_SPLIT
    case, ref = cc.exact_prepared((N, Ci, Co, H, W, k, k, stride, pad, 1), True, False)
    if sliced:
        clip = torch.full((N, 4, H, W), 7.0).cuda()
        clip[:, :3] = _gpu(case["x"])
        x = clip[:, :3]
        assert not x.is_contiguous() and x.stride(0) == 4 * H * W
    else:
        x = _gpu(case["x"])
    plan = _plan(case)
    assert plan.algo == "tile"
    whole, recs = _recorded(plan, x)
    per_image = 2 * Co * plan.Kpad * ref.shape[2] * ref.shape[3]
    assert [(r[2], r[3], r[1]) for r in recs] == [(-4, 16, N * per_image)]
    monkeypatch.setattr(ops.ConvPlan, "TILE_MAX_ELEMENTS", 2 * x.stride(0))
    split, recs = _recorded(plan, x)
    assert [(r[2], r[3], r[1]) for r in recs] == [(-4, 16, n * per_image) for n in (2, 2, 1)]
    _assert_exact(split, ref, "tile in three image ranges")
    assert torch.equal(split, whole)
    if sliced:                                   # a limit between Ci * H * W and the stride: one image per launch
        monkeypatch.setattr(ops.ConvPlan, "TILE_MAX_ELEMENTS", x.stride(0) + Ci * H * W)
        single, recs = _recorded(plan, x)
        assert [r[1] for r in recs] == [per_image] * N
        assert torch.equal(single, whole)
