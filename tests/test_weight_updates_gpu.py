"""GPU: a weight changes after a fused inference route has run, and the route follows - per site that keeps tensors DERIVED
from weights (models.fused.DERIVED_ATTRIBUTES, util.memo's "lvl_pos"), every source tensor on its own, by every way user code
changes a tensor (tests/_lifecycle.py).  The reference is the same route on a module that has never run, loaded with the edited
state: same kernels, same data, so the comparison is bitwise and no tolerance appears."""
import copy
import functools

import pytest
import torch
from torch import nn

from tests import _lifecycle as L

pytestmark = pytest.mark.gpu


def _seeded(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _cpu_template(make):
    """``make`` -> a filled module on the CPU, built once per process; every ``build()`` is a copy of it on the GPU."""
    cached = functools.lru_cache(maxsize=None)(make)
    return lambda: copy.deepcopy(cached()).cuda().eval()


def _params(cases):
    return pytest.mark.parametrize("owner,name,kind", cases, ids=[L.case_id(c) for c in cases])


# ---- Bottleneck: _folded (ConvPlan of conv2, the pair product), _plans1x1 -------------------------------------------------------
def _bottleneck(inplanes, planes, stride, down):
    from models.backbone_scratch import FrozenBatchNorm2d
    from models.resnet import Bottleneck
    from tests._param_fill import fill_params_by_name
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), FrozenBatchNorm2d(planes * 4)) if down else None
    return fill_params_by_name(Bottleneck(inplanes, planes, stride, 1, ds, FrozenBatchNorm2d), seed=3)


# name: (inplanes, planes, stride, downsample, input H x W, conv2's algorithm, pair product, slots of _plans1x1)
BLOCKS = {"wino_pair": (64, 64, 1, True, (8, 12), "wino", True, None),
          "igemm_strided_shortcut": (256, 128, 2, True, (8, 12), "igemm", False, {1}),
          "unaligned_rows": (256, 64, 1, False, (7, 9), "wino", False, {0, 2})}
BLOCK_CASES = [(b,) + c for b in BLOCKS
               for c in L.case_list(L.sources(_bottleneck(*BLOCKS[b][:4])), ("conv2", "weight"))]


def test_bottleneck_cases_cover_every_tensor():
    assert [len(L.sources(_bottleneck(*BLOCKS[b][:4]))) for b in BLOCKS] == [20, 20, 15]        # 3 or 4 x (conv weight + 4 BN buffers)


@pytest.mark.parametrize("block,owner,name,kind", BLOCK_CASES, ids=[c[0] + "-" + L.case_id(c[1:]) for c in BLOCK_CASES])
def test_bottleneck_follows_a_weight_update(block, owner, name, kind):
    inplanes, planes, stride, down, (H, W), algo, pair, slots = BLOCKS[block]
    build = _cpu_template(lambda: _bottleneck(inplanes, planes, stride, down))
    x = _seeded(2, inplanes, H, W, seed=1)

    def route(m):                                   # the case keeps meaning what its name says
        plan2, had_pair = m._folded[1][1], m._folded[1][4] is not None
        assert plan2.algo == algo and had_pair == pair
        assert (set(m.__dict__["_plans1x1"]) if "_plans1x1" in m.__dict__ else None) == slots

    L.assert_follows(build, lambda m: m.forward_fused(x), owner, name, kind, after_first_runs=route)


# ---- the 1x1 chain: a block's launch consumes the NEXT block's folded conv1; the stem -------------------------------------------
def _resnet_body():
    from models.backbone_scratch import build_backbone_fromscratch
    from models.config import single_args
    from tests._param_fill import fill_params_by_name
    args = single_args("Baseline")
    args.depth_type = "Baseline_rgb"
    return fill_params_by_name(build_backbone_fromscratch(args), seed=3)[0].body          # (test_resnet_layers_agree_with_the_chain_on_and_off)


_body = _cpu_template(_resnet_body)
CHAIN_CASES = L.case_list([("layer1.1.conv1", "weight", False), ("layer1.1.bn1", "bias", True),
                           ("layer2.0.conv1", "weight", False), ("layer2.0.bn1", "running_var", True)], ("layer1.1.conv1", "weight"))


@_params(CHAIN_CASES)
def test_conv1x1_chain_follows_the_next_blocks_conv1(monkeypatch, owner, name, kind):
    import models.resnet as resnet
    from dfx import ops
    monkeypatch.setattr(resnet, "_CONV_CHAIN", True)
    monkeypatch.setattr(resnet, "_CONV_CHAIN_MAX_C1", 256)          # all seven producers of layer1 and layer2, as that test counts them
    calls, chain = [], ops.conv1x1_chain
    monkeypatch.setattr(ops, "conv1x1_chain", lambda *a, **k: (calls.append(a[0].shape), chain(*a, **k))[1])
    x = _seeded(2, 3, 64, 96, seed=1)

    def run(body):
        del calls[:]
        a = body.run_stage(body.layer1, body.stem(x, True), True)
        b = body.run_stage(body.layer2, a, True)
        assert len(calls) == 7
        return [a, b, body.__dict__["_chain_carry"][1]]             # ... the last one leaves layer3[0]'s conv1 waiting

    L.assert_follows(_body, run, owner, name, kind)


STEM_SOURCES = [("conv1", "weight", False)] + [("bn1", n, True) for n in ("weight", "bias", "running_mean", "running_var")]
STEM_CASES = L.case_list(STEM_SOURCES, ("conv1", "weight"))


def test_stem_cases_cover_every_tensor_and_the_exclusions_are_the_classifier():
    body = _resnet_body()
    assert L.sources(body, only=lambda n: n.startswith(("conv1.", "bn1."))) == STEM_SOURCES
    everything = L.sources(body)
    left_out = {n for n, _ in list(body.named_parameters()) + list(body.named_buffers())} - {f"{o}.{n}" for o, n, _ in everything}
    assert left_out == {"fc.weight", "fc.bias"}


@_params(STEM_CASES)
def test_stem_follows_a_weight_update(owner, name, kind):
    x = _seeded(2, 3, 64, 96, seed=1)
    L.assert_follows(_body, lambda body: body.stem(x, True), owner, name, kind,
                     after_first_runs=lambda body: body.__dict__["_stem_folded"])


# ---- DFormer depth stages: every BatchNorm folded into the convolution in front of it -------------------------------------------
def _dformer():
    from models.dformer_backbone import DFormerBackbone
    from tests._param_fill import fill_params_by_name
    return fill_params_by_name(DFormerBackbone(train_backbone=False, freeze_batchnorm=True), seed=2)


_RUN_STAGES = tuple(f"depth_backbone.downsample_layers_e.{i}." for i in range(3))
DFORMER_CASES = L.case_list(L.sources(_dformer()), ("depth_backbone.downsample_layers_e.1.1", "weight"))


def test_dformer_cases_cover_the_three_run_stages():
    srcs = L.sources(_dformer())
    assert len(srcs) == 4 * 2 + 4 * 4 and all(f"{o}.{n}".startswith(_RUN_STAGES) for o, n, _ in srcs)       # 4 convolutions, 4 BatchNorms
    names = {n for n, _ in list(_dformer().named_parameters()) + list(_dformer().named_buffers())}
    left_out = names - {f"{o}.{n}" for o, n, _ in srcs}
    assert all(n.endswith("num_batches_tracked") or n.startswith("depth_backbone.downsample_layers_e.3.") for n in left_out)


def _run_dformer(bb, d):
    from util.misc import NestedTensor
    return bb(NestedTensor(d, torch.zeros(d.shape[0], *d.shape[2:], dtype=torch.bool, device="cuda")))["0"].tensors


@_params(DFORMER_CASES)
def test_dformer_folded_route_follows_a_weight_update(monkeypatch, owner, name, kind):
    from models.dformer_backbone import DFormerBackbone
    folded, real = [], DFormerBackbone._forward_folded
    monkeypatch.setattr(DFormerBackbone, "_forward_folded", lambda self, stages, x: (folded.append(1), real(self, stages, x))[1])
    d = torch.rand(2, 1, 64, 96, generator=torch.Generator().manual_seed(5)).cuda()
    L.assert_follows(_cpu_template(_dformer), lambda bb: _run_dformer(bb, d), owner, name, kind)
    assert len(folded) == 4                        # two first runs, the run after the edit, the fresh module


def test_dformer_folded_route_follows_running_statistics_moved_by_a_train_mode_pass():
    build = _cpu_template(_dformer)
    d = torch.rand(2, 1, 64, 96, generator=torch.Generator().manual_seed(5)).cuda()
    run = lambda bb: _run_dformer(bb, d)          # noqa: E731
    a = build()
    y0 = L.run_twice(run, a)
    before = {k: v.clone() for k, v in a.state_dict().items()}
    a.train()
    with torch.no_grad():
        _run_dformer(a, d * 2 + 1)                 # batch statistics; every BatchNorm of the run stages moves its running ones
    a.eval()
    moved = [k for k, v in a.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == 4 * 3 and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in moved)
    with torch.no_grad():
        y1 = [run(a).clone()]
    L.assert_same(y1, L.fresh_reference(build, run, a), "after a train-mode pass")
    assert L.differs(y1, y0)


# ---- _ConvGN: the input projections that go through a ConvPlan -------------------------------------------------------------------
CONVGN = {"3x3_stride2": (dict(kernel_size=3, stride=2, padding=1), (9, 13)), "1x1_unaligned_rows": (dict(kernel_size=1), (7, 9))}


def _convgn(which):
    from models.detector_common import _conv_gn
    from tests._param_fill import fill_params_by_name
    return fill_params_by_name(_conv_gn(64, 256, **CONVGN[which][0]), seed=4)


CONVGN_CASES = [(w,) + c for w in CONVGN for c in L.case_list(L.sources(_convgn(w)), ("0", "bias"))]


@pytest.mark.parametrize("which,owner,name,kind", CONVGN_CASES, ids=[c[0] + "-" + L.case_id(c[1:]) for c in CONVGN_CASES])
def test_input_projection_follows_a_weight_update(which, owner, name, kind):
    assert len(L.sources(_convgn(which))) == 4                       # conv weight and bias, norm weight and bias
    x = _seeded(2, 64, *CONVGN[which][1], seed=6)
    L.assert_follows(_cpu_template(lambda: _convgn(which)), lambda m: m(x), owner, name, kind,
                     after_first_runs=lambda m: m.__dict__["_plan"])


# ---- MSDeformAttn: the joint [offsets | logits] projection, row-major and regrouped per head ------------------------------------
MSDA = {"fused_4_levels": (4, [(6, 8), (3, 4), (2, 2), (1, 1)], 37, "_qproj_cache"),
        "level_in_lds": (1, [(6, 8)], 1024, "_qproj_head")}          # dfx.ops.LEVEL_MIN_QUERIES queries: the route's own threshold


def _msda(which):
    from models.ops.modules import MSDeformAttn
    from tests._param_fill import fill_params_by_name
    return fill_params_by_name(MSDeformAttn(256, MSDA[which][0], 8, 4), seed=1)


MSDA_CASES = [(w,) + c for w in MSDA for c in L.case_list(L.sources(_msda(w)), ("sampling_offsets", "bias"))]


@pytest.mark.parametrize("which,owner,name,kind", MSDA_CASES, ids=[c[0] + "-" + L.case_id(c[1:]) for c in MSDA_CASES])
def test_msdeformattn_follows_a_weight_update(monkeypatch, which, owner, name, kind):
    from dfx import ops
    from models.transformer_layers import make_level_tensors
    n_levels, shp, Lq, cache = MSDA[which]
    assert len(L.sources(_msda(which))) == 8
    shapes, lsi = make_level_tensors(shp, torch.device("cuda"))
    S = sum(h * w for h, w in shp)
    q, x = _seeded(2, Lq, 256, seed=1), _seeded(2, S, 256, seed=2)
    ref = torch.rand(2, Lq, n_levels, 2, generator=torch.Generator().manual_seed(3)).cuda()
    mask = (torch.rand(2, S, generator=torch.Generator().manual_seed(4)) > 0.85).cuda()
    routes = []
    for fn in ("msda_level_forward", "msda_fused_forward"):
        monkeypatch.setattr(ops, fn, lambda *a, _real=getattr(ops, fn), _fn=fn, **k: (routes.append(_fn), _real(*a, **k))[1])
    if which == "level_in_lds":
        assert ops.level_supported(x, *shp[0], Lq, 8, 32, 1, 4, 1)

    def took(m):
        assert set(routes) == {"msda_level_forward" if which == "level_in_lds" else "msda_fused_forward"} and cache in m.__dict__

    L.assert_follows(_cpu_template(lambda: _msda(which)), lambda m: m(q, ref, x, shapes, lsi, mask), owner, name, kind,
                     after_first_runs=took)


# ---- stacked projections (_value_stack, _kv_stack) and util.memo's "lvl_pos" -----------------------------------------------------
T_FRAMES, Q_TPP = 4, 80       # 3 reference frames; 80 queries: all three rounds of the temporal stage pick more rows (4 * k * 3, k = 80, 50,
                              # 30) than the pool of 4 * 80 has, so all three query encoders project the pool - in one stacked launch


class _Clip(nn.Module):
    """The smallest TransVOD++ transformer tests/_cases.py builds, with 3 reference frames, and the heads its stages are handed."""

    def __init__(self):
        super().__init__()
        from models import deformable_transformer_multi_plusplus as tpp
        from models.detector_common import MLP
        self.tr = tpp.DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=1024,
                                            dropout=0.1, activation="relu", return_intermediate_dec=True, num_feature_levels=1,
                                            dec_n_points=4, enc_n_points=4, two_stage=False, two_stage_num_proposals=Q_TPP,
                                            num_query=Q_TPP, n_temporal_decoder_layers=1, num_ref_frames=T_FRAMES - 1,
                                            fixed_pretrained_model=False, args=None, use_depth=False, depth_type="Baseline_rgb",
                                            dpth_n_points=4)
        self.tr.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(2)])
        self.cls = nn.Linear(256, 3)
        self.tcls = nn.ModuleList([nn.Linear(256, 3) for _ in range(3)])
        self.tbox = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(3)])


def _clip_model():
    from tests._param_fill import fill_params_by_name
    m = fill_params_by_name(_Clip(), seed=21)
    with torch.no_grad():
        for h in list(m.tr.decoder.bbox_embed) + list(m.tbox):         # keep refined boxes well inside (0, 1)
            h.layers[-1].weight.mul_(0.2)
    return m


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    from models.position_encoding import PositionEmbeddingSine
    from util.misc import NestedTensor
    src = _seeded(T_FRAMES, 256, 6, 8, seed=70)
    mask = torch.zeros(T_FRAMES, 6, 8, dtype=torch.bool, device="cuda")
    pos = PositionEmbeddingSine(128, normalize=True)(NestedTensor(src, mask))
    whwh = torch.as_tensor((128, 96, 128, 96), dtype=torch.long, device="cuda").repeat(1, Q_TPP, 1)
    others = torch.as_tensor([[j for j in range(T_FRAMES) if j != i] for i in range(T_FRAMES)], dtype=torch.long, device="cuda")
    return src, mask, pos, _seeded(Q_TPP, 512, seed=90), whwh, others


def _run_clip(m):
    """Every frame as the current frame, as models.clip_inference.ClipRunner drives the stages."""
    src, mask, pos, qe, whwh, others = _clip_inputs()
    tr = m.tr
    st = tr._spatial_stage([src], [mask], [pos], [], [], [], qe, [])
    fs = tr.frame_stage(st["hs"][-1], st["inter_references"][-1], st["memory"], st["lvl_pos_embed_flatten"], st["last_hw"], whwh,
                        m.cls, tr.decoder.bbox_embed[-1], roles=("cur", "ref"))
    final_hs, final_refs, aux, _ = tr.temporal_stage(fs["cur"], st["inter_references"][-1], st["memory"], fs["ref"], fs["logits"], others,
                                                     st["spatial_shapes"], st["level_start_index"], st["valid_ratios"], m.tcls, m.tbox)
    return [st["hs"], st["memory"], final_hs, final_refs, aux[0]["pred_logits"], aux[1]["pred_boxes"]]


STACK_CASES = (L.case_list([("tr.decoder.layers.1.cross_attn.value_proj", "weight", False), ("tr.decoder.layers.1.cross_attn.value_proj", "bias", False)],
                           ("tr.decoder.layers.1.cross_attn.value_proj", "bias"))
               + L.case_list([("tr.temporal_decoder2.layers.0.cross_attn.value_proj", "bias", False)],
                             ("tr.temporal_decoder2.layers.0.cross_attn.value_proj", "bias"))[:2]
               + L.case_list([("tr.temporal_query_layer3.cross_attn", "in_proj_weight", False), ("tr.temporal_query_layer3.cross_attn", "in_proj_bias", False)],
                             ("tr.temporal_query_layer3.cross_attn", "in_proj_bias"))
               + L.case_list([("tr", "level_embed", False)], ("tr", "level_embed")))


@_params(STACK_CASES)
def test_stacked_projections_and_level_positions_follow_a_weight_update(owner, name, kind):
    """The stacked matrices live on the FIRST module of each group; the edited one is the second (value_proj of the decoder
    layers, of the three temporal decoders) or the third (in_proj of the temporal query encoders)."""
    from util import memo

    def stacked(m):
        tr = m.tr
        assert tr.decoder.layers[0].cross_attn.__dict__["_value_stack"][1].shape == (2 * 256, 256)
        assert tr.temporal_decoder1.layers[0].cross_attn.__dict__["_value_stack"][1].shape == (3 * 256, 256)
        assert tr.temporal_query_layer1.cross_attn.__dict__["_kv_stack"][1].shape == (3 * 512, 256)
        assert any(tag[0] == "lvl_pos" for _, tag in memo._MEMO if isinstance(tag, tuple))

    L.assert_follows(_cpu_template(_clip_model), _run_clip, owner, name, kind, after_first_runs=stacked)


def _single_l4():
    from models import deformable_transformer_single as ts
    from models.detector_common import MLP
    from tests._param_fill import fill_params_by_name
    tr = ts.DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=1024, dropout=0.1,
                                  activation="relu", return_intermediate_dec=True, num_feature_levels=4, dec_n_points=4, enc_n_points=4,
                                  two_stage=False, two_stage_num_proposals=30, use_depth=False, depth_type="Baseline_rgb", dpth_n_points=4)
    tr.decoder.bbox_embed = nn.ModuleList([MLP(256, 256, 4, 3) for _ in range(2)])
    fill_params_by_name(tr, seed=11)
    with torch.no_grad():
        for h in tr.decoder.bbox_embed:
            h.layers[-1].weight.mul_(0.2)
    return tr


@_params(L.case_list([("", "level_embed", False)], ("", "level_embed")))
def test_level_positions_follow_level_embed_on_four_levels(owner, name, kind):
    """tests/_cases.py's single_baseline_l4: four levels with padded frames, the positional tensors the same objects on every call
    (what the detector's memoised positional encoding hands over), so util.memo serves "lvl_pos" on the second run."""
    import tests._cases as C
    from models.position_encoding import PositionEmbeddingSine
    from util import memo
    from util.misc import NestedTensor
    C._DEVICE = "cuda"
    shp = [(8, 10), (4, 5), (2, 3), (1, 2)]
    srcs = [C.rnd(40 + i, 2, 256, h, w) for i, (h, w) in enumerate(shp)]
    masks = [C.pad_masks(50 + i, 2, h, w) for i, (h, w) in enumerate(shp)]
    C._DEVICE = "cpu"
    pe = PositionEmbeddingSine(128, normalize=True)
    poss = [pe(NestedTensor(s, m)) for s, m in zip(srcs, masks)]
    qe = _seeded(30, 512, seed=60)

    def run(tr):
        hs, init_ref, inter, _, _ = tr(srcs, masks, poss, [], [], [], qe, [])
        return [hs, init_ref, inter]

    def memoised(tr):
        assert sum(tag[0] == "lvl_pos" for _, tag in memo._MEMO if isinstance(tag, tuple)) == 4

    L.assert_follows(_cpu_template(_single_l4), run, owner, name, kind, after_first_runs=memoised)


# ---- the whole detector: one real training step between two evaluations -----------------------------------------------------------
def _detector_outputs(out):
    return [out["pred_logits"], out["pred_boxes"]] + list(out["topk"])


def test_detector_follows_one_training_step_and_drop_derived_is_complete():
    """Notices a site that keeps derived tensors and is missing from models.fused.DERIVED_ATTRIBUTES' keyed sites: every
    parameter that received a gradient moves at once, and so do the DFormer running statistics (a train-mode pass)."""
    from models.clip_inference import ClipRunner
    from models.fused import drop_derived
    from tests.test_clip_shard_gpu import _build, _clip
    from util.misc import NestedTensor
    model, clip = _build(), _clip().cuda()
    runner = ClipRunner(model, micro_batch=4)
    y0 = L.run_twice(lambda r: _detector_outputs(r(clip)), runner)

    model.train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out = model(NestedTensor(clip, torch.zeros(4, 64, 96, dtype=torch.bool, device="cuda")))
    (out["pred_logits"].sum() + out["pred_boxes"].sum()).backward()
    torch.optim.SGD(model.parameters(), lr=1e-3).step()
    model.zero_grad(set_to_none=True)
    model.eval()
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) > 100 and any("backbone" in k for k in moved) and any("temporal" in k for k in moved), len(moved)

    with torch.no_grad():
        y1 = [t.clone() for t in _detector_outputs(runner(clip))]
    fresh = _build()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        y_ref = _detector_outputs(ClipRunner(fresh, micro_batch=4)(clip))
    L.assert_same(y1, y_ref, "after a training step: the model that had run before against a fresh one")
    assert L.differs(y1, y0)

    assert drop_derived(model) > 0
    assert drop_derived(model) == 0
    with torch.no_grad():
        L.assert_same(_detector_outputs(runner(clip)), y1, "after drop_derived")
    assert drop_derived(model) > 0
