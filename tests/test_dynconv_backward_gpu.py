"""GPU: the fused DynamicConv backward (csrc/dynconv_backward.hip) against the fp64 restatement of tests/_dynconv_cases.py,
the autograd surface of ``dfx.ops.dynamic_conv``, the ``DynamicConv`` module and ``frame_stage`` on the fused route in grad
mode, and the unchanged inference path.  How the cases stay clear of the ReLU kinks: tests/_dynconv_cases.py."""
import copy

import pytest
import torch

from tests import _dynconv_cases as dc

pytestmark = pytest.mark.gpu

YARDSTICK_FACTOR = 4      # the GPU may be this many times the CPU's own fp32 error (the project's factor: test_roi_backward_gpu)


def _gpu_inputs(case, requires=dc.OUTPUTS):
    t = {k: case[k].detach().cuda() for k in dc.OUTPUTS}
    if case["params"].shape[1] > 2 * dc.C * dc.DD:       # rows strided inside a wider buffer: p_stride > row length
        wide = torch.zeros(case["params"].shape[0], case["params"].shape[1] + 64, device="cuda")
        wide[:, : case["params"].shape[1]] = t["params"]
        t["params"] = wide[:, : case["params"].shape[1]]
        assert t["params"].stride(0) > t["params"].shape[1]
    for k in requires:
        t[k].requires_grad_()
    return t


def _run(case, requires=dc.OUTPUTS):
    """(out, {name: gradient or None}) of ops.dynamic_conv in grad mode on the GPU."""
    from dfx import ops
    t = _gpu_inputs(case, requires)
    out = ops.dynamic_conv(t["feats"], t["params"], dc.Norm(t["g1"], t["b1"]), dc.Norm(t["g2"], t["b2"]))
    assert out.grad_fn is not None
    out.backward(case["grad_out"].cuda())
    torch.cuda.synchronize()
    return out.detach(), {k: t[k].grad for k in dc.OUTPUTS}


def _assert_no_flip(out, case):
    keep = ~case["unclear"]
    flips = (((out.cpu() > 0) != case["p2_positive"]) & keep[..., None]).sum().item()
    assert flips == 0, f"{flips} ReLU units of kept rows changed sign on the GPU: the gradients are not comparable"


def _compare(case, grads, names=dc.OUTPUTS):
    ref = dc.restated_backward(case)
    cpu32 = dc.autograd_backward(case, torch.float32)
    worst = []
    for k in names:
        yard, got = dc.rel_err(cpu32[k], ref[k]), dc.rel_err(grads[k].cpu(), ref[k])
        print(f"  d{k}: cpu fp32 {yard:.3e}, gpu {got:.3e}, max |ref| {ref[k].abs().max().item():.3e}")
        if got > YARDSTICK_FACTOR * yard:
            worst.append(f"d{k}: gpu {got:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}")
    assert not worst, "; ".join(worst)


# ---- 4. operator against fp64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,R,extra", dc.OPERATOR_CASES)
def test_operator_matches_fp64_within_the_measured_yardstick(K, R, extra):
    """Every gradient, in full, against the fp64 CPU result, error relative to that gradient's largest magnitude.  No bound
    can be derived through two LayerNorms, so the yardstick is measured here: the same computation on the CPU in fp32
    against fp64; the GPU may be at most 4x that per output (two fp32 evaluations of one computation that differ in
    summation order)."""
    case = dc.make_case(K, R, extra)
    print(f"case ({K},{R}): noise {case['noise']:.2e}, {case['fraction']:.2%} of the rows zeroed in grad_out")
    out, grads = _run(case)
    _assert_no_flip(out, case)
    assert grads["params"].shape == case["params"].shape
    if extra:
        assert grads["params"][:, 2 * dc.C * dc.DD:].abs().max() == 0
    _compare(case, grads)


# ---- 5. autograd surface ---------------------------------------------------------------------------------------
def test_grad_mode_makes_a_node_and_every_input_gets_its_gradient():
    case = dc.make_case(37, 49, 64)
    out, grads = _run(case)
    for k in dc.OUTPUTS:
        assert grads[k] is not None and grads[k].shape == case[k].shape and grads[k].abs().max() > 0, k


def test_no_node_without_a_gradient_to_carry():
    from dfx import _lib, ops
    case = dc.make_case(37, 49, 64)
    t = _gpu_inputs(case, requires=())
    n1, n2 = dc.Norm(t["g1"], t["b1"]), dc.Norm(t["g2"], t["b2"])
    raw = torch.empty_like(t["feats"])
    code = _lib.load().dfx_dynamic_conv_f32(t["feats"].data_ptr(), t["params"].data_ptr(), t["params"].stride(0),
                                            t["g1"].data_ptr(), t["b1"].data_ptr(), t["g2"].data_ptr(), t["b2"].data_ptr(),
                                            raw.data_ptr(), 37, 49, 256, 64, dc.EPS, torch.cuda.current_stream().cuda_stream)
    assert code == 0
    plain = ops.dynamic_conv(t["feats"], t["params"], n1, n2)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, raw)
    tg = _gpu_inputs(case)
    with torch.no_grad():
        quiet = ops.dynamic_conv(tg["feats"], tg["params"], dc.Norm(tg["g1"], tg["b1"]), dc.Norm(tg["g2"], tg["b2"]))
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, raw)
    tracked = ops.dynamic_conv(tg["feats"], tg["params"], dc.Norm(tg["g1"], tg["b1"]), dc.Norm(tg["g2"], tg["b2"]))
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), raw)


def test_unrequested_gradients_are_skipped_and_the_others_unchanged():
    case = dc.make_case(37, 49, 64)
    _, full = _run(case)
    _, no_feats = _run(case, requires=tuple(k for k in dc.OUTPUTS if k != "feats"))
    _, no_params = _run(case, requires=tuple(k for k in dc.OUTPUTS if k != "params"))
    _, ln_only = _run(case, requires=("g1", "b1", "g2", "b2"))
    assert no_feats["feats"] is None and no_params["params"] is None and ln_only["feats"] is None and ln_only["params"] is None
    for run, skipped in ((no_feats, {"feats"}), (no_params, {"params"}), (ln_only, {"feats", "params"})):
        for k in dc.OUTPUTS:
            if k not in skipped:
                assert torch.equal(run[k], full[k]), k


def test_backward_entry_reports_what_it_was_asked_for():
    from dfx import ops
    case = dc.make_case(5, 7)
    t = _gpu_inputs(case, requires=())
    n1, n2 = dc.Norm(t["g1"], t["b1"]), dc.Norm(t["g2"], t["b2"])
    res = ops.dynamic_conv_backward(case["grad_out"].cuda(), t["feats"], t["params"], n1, n2, need_feats=False, need_params=False)
    assert res[0] is None and res[1] is None and [tuple(r.shape) for r in res[2:]] == [(64,), (64,), (256,), (256,)]
    empty = ops.dynamic_conv_backward(torch.zeros(0, 7, 256, device="cuda"), torch.zeros(0, 7, 256, device="cuda"),
                                      torch.zeros(0, 2 * 256 * 64, device="cuda"), n1, n2)
    assert empty[0].shape == (0, 7, 256) and all(r.abs().max() == 0 for r in empty[2:])


def test_params_rows_of_any_width_get_a_gradient_of_their_shape():
    """params [K, 2*C*dd + 2] as a column slice of a wider buffer (row stride a multiple of 4, as the forward asks): the
    gradient has params' shape, zeros in the extra columns, and equals the gradient of the exact-width call."""
    from dfx import ops
    case = dc.make_case(5, 7)
    t = _gpu_inputs(case, requires=())
    n1, n2 = dc.Norm(t["g1"], t["b1"]), dc.Norm(t["g2"], t["b2"])
    width = 2 * dc.C * dc.DD
    wide = torch.zeros(5, width + 8, device="cuda")
    wide[:, :width] = t["params"]
    odd = wide[:, : width + 2]
    go = case["grad_out"].cuda()
    want = ops.dynamic_conv_backward(go, t["feats"], t["params"], n1, n2)
    got = ops.dynamic_conv_backward(go, t["feats"], odd, n1, n2)
    assert got[1].shape == odd.shape and got[1][:, width:].abs().max() == 0
    assert torch.equal(got[1][:, :width], want[1]) and torch.equal(got[0], want[0])


# ---- 6. bit-reproducible ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [600, 1200])
def test_two_calls_give_the_same_bits(K):
    """No atomics, a fixed grid and fixed summation orders: every workgroup walks several RoIs here."""
    case = dc.make_case(K, 49)
    _, a = _run(case)
    _, b = _run(case)
    for k in dc.OUTPUTS:
        assert torch.equal(a[k], b[k]), k


# ---- 7. padding rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,R,extra", dc.PADDING_CASES)
def test_padding_rows_contribute_nothing(K, R, extra):
    """LayerNorm biases of +2: rows R..63 of the 64-row tiles (zero rows of X, whose LayerNorm is the bias) are +2 in A1
    and positive in P2.  They may only ever meet zero rows of dZ2 / dZ1: a padded row of dZ that is not zero leaks
    through A1^T dZ2 into dK2 and through the row sums into dg, db, far beyond the yardstick.  (dY itself is read as
    zero on those rows, so this is about what the kernel does with the padded rows of its LDS tiles, not about a mask
    on dY.)"""
    case = dc.make_case(K, R, extra, bias=2.0)
    out, grads = _run(case)
    _assert_no_flip(out, case)
    _compare(case, grads)


# ---- 8. the module ---------------------------------------------------------------------------------------------
MOD_K = 24


def _module_case():
    from models.sparse_roi_head.head import DynamicConv
    from tests._param_fill import fill_params_by_name
    cfg = {"MODEL": {"SparseRCNN": {"HIDDEN_DIM": 256, "DIM_DYNAMIC": 64, "NUM_DYNAMIC": 2},
                     "ROI_BOX_HEAD": {"POOLER_RESOLUTION": 7}}}
    m = fill_params_by_name(DynamicConv(cfg), seed=31, prefix="inst_interact.").train()
    g = torch.Generator().manual_seed(32)
    return m, torch.randn(1, MOD_K, 256, generator=g), torch.randn(MOD_K, 49, 256, generator=g), torch.randn(MOD_K, 256, generator=g)


def _module_run(m, pro, feats, device, dtype, row_mask=None, weight=None, fused=False):
    """Output, the three ReLU pre-activations and (with ``weight``) the gradients of loss = sum(out * weight).  ``row_mask``
    [K,49] multiplies the output of the second ReLU - the operator boundary - on every route: through a forward hook
    on the activation where the modules run, around dfx.ops.dynamic_conv on the fused route (which calls no module)."""
    from dfx import ops
    m = copy.deepcopy(m).to(device=device, dtype=dtype)
    pro = pro.to(device=device, dtype=dtype).requires_grad_()
    feats = feats.to(device=device, dtype=dtype).requires_grad_()
    mask = None if row_mask is None else row_mask.to(device=device, dtype=dtype)[..., None]
    pre, calls, hooks, saved = [], [0], [], ops.dynamic_conv
    if fused:
        ops.dynamic_conv = lambda f, p, n1, n2: saved(f, p, n1, n2) if mask is None else saved(f, p, n1, n2) * mask
    else:
        def after(mod, args, out):
            calls[0] += 1
            return out * mask if (calls[0] == 2 and mask is not None) else None
        hooks = [m.activation.register_forward_pre_hook(lambda mod, args: pre.append(args[0].detach().clone().cpu().double())),
                 m.activation.register_forward_hook(after)]
    try:
        out = m(pro, feats.permute(1, 0, 2))
        grads = None
        if weight is not None:
            leaves = dict(pro_features=pro, roi_features=feats, **dict(m.named_parameters()))
            got = torch.autograd.grad((out * weight.to(device=device, dtype=dtype)).sum(), list(leaves.values()))
            grads = {k: v.detach().cpu().double() for k, v in zip(leaves, got)}
    finally:
        ops.dynamic_conv = saved
        for h in hooks:
            h.remove()
    return out.detach().cpu().double(), pre, grads


@pytest.fixture(scope="module")
def module_runs():
    m, pro, feats, weight = _module_case()
    a64, a32 = _module_run(m, pro, feats, "cpu", torch.float64), _module_run(m, pro, feats, "cpu", torch.float32)
    noise = max((a32[1][i] - a64[1][i]).abs().max().item() for i in (0, 1))
    unclear = (a64[1][0].abs().min(-1).values < dc.KINK_FACTOR * noise) | (a64[1][1].abs().min(-1).values < dc.KINK_FACTOR * noise)
    assert unclear.float().mean().item() <= dc.MAX_UNCLEAR
    keep = ~unclear
    b64, b32 = (_module_run(m, pro, feats, "cpu", dt, keep) for dt in (torch.float64, torch.float32))
    noise3 = (b32[1][2] - b64[1][2]).abs().max().item()
    clear3 = b64[1][2].abs() >= dc.KINK_FACTOR * noise3            # the third ReLU is elementwise: unit by unit
    assert clear3.float().mean().item() >= 1 - dc.MAX_UNCLEAR
    weight = weight * clear3
    ref = _module_run(m, pro, feats, "cpu", torch.float64, keep, weight)
    cpu32 = _module_run(m, pro, feats, "cpu", torch.float32, keep, weight)
    return m, pro, feats, keep, weight, ref, cpu32


def test_module_trains_on_the_fused_route(module_runs, monkeypatch):
    """DynamicConv in train mode: the fused route against the same module with DFX_DYNCONV_TRAIN off (output, the
    forward test's tolerance) and against the fp64 CPU module (every gradient, 4x the CPU fp32 figure); torch.bmm is
    not called on the fused route."""
    from models.sparse_roi_head import head
    m, pro, feats, keep, weight, ref, cpu32 = module_runs
    bmm_calls, real_bmm = [0], torch.bmm

    def spy(*a, **k):
        bmm_calls[0] += 1
        return real_bmm(*a, **k)

    monkeypatch.setattr(torch, "bmm", spy)
    assert head.DYNCONV_TRAIN
    fused = _module_run(m, pro, feats, "cuda", torch.float32, keep, weight, fused=True)
    assert bmm_calls[0] == 0, "grad mode still ran the library route"
    monkeypatch.setattr(head, "DYNCONV_TRAIN", False)
    library = _module_run(m, pro, feats, "cuda", torch.float32, keep, weight)
    assert bmm_calls[0] == 2
    assert torch.allclose(fused[0], library[0], rtol=2e-4, atol=2e-4), (fused[0] - library[0]).abs().max().item()
    bad = []
    for k in ref[2]:
        yard, got, lib = dc.rel_err(cpu32[2][k], ref[2][k]), dc.rel_err(fused[2][k], ref[2][k]), dc.rel_err(library[2][k], ref[2][k])
        print(f"  d{k}: cpu fp32 {yard:.3e}, gpu fused {got:.3e}, gpu library {lib:.3e}")
        if got > YARDSTICK_FACTOR * yard:
            bad.append(f"d{k}: gpu {got:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}")
    assert not bad, "; ".join(bad)


# ---- 9. frame_stage end to end ---------------------------------------------------------------------------------
def _frame_stage_fused(tr, heads, inputs, detach_memory, monkeypatch):
    """frame_stage on the GPU with no hook on the head's activation, so that DynamicConv takes the fused route:
    (memory.grad or None, head parameter gradients, need_feats of every fused backward, number of RoIAlign backwards)."""
    from dfx import ops
    from tests.test_roi_backward_gpu import HW
    tr, heads = copy.deepcopy(tr).cuda(), copy.deepcopy(heads).cuda()
    t = {k: v.detach().cuda() for k, v in inputs.items()}      # detach: an earlier CPU fp32 run may have marked the inputs
    memory = t["memory"] if detach_memory else t["memory"].requires_grad_()
    seen, roi_backwards = [], [0]
    real_dc, real_roi = ops.dynamic_conv_backward, ops.roi_align_backward

    def dc_backward(grad_out, feats, params, n1, n2, need_feats=True, need_params=True):
        seen.append(need_feats)
        return real_dc(grad_out, feats, params, n1, n2, need_feats=need_feats, need_params=need_params)

    def roi_backward(*a, **k):
        roi_backwards[0] += 1
        return real_roi(*a, **k)

    monkeypatch.setattr(ops, "dynamic_conv_backward", dc_backward)
    monkeypatch.setattr(ops, "roi_align_backward", roi_backward)
    head = tr.dynamic_layer_for_current_query1
    out = tr.frame_stage(t["hs_last"], t["ref_last"], memory, t["pos_embed"], HW, t["whwh"], heads["cls"], heads["box"],
                         roles=("cur", "ref"))
    loss = (out["cur"] * t["p_cur"]).sum() + (out["ref"] * t["p_ref"]).sum()
    params = dict(head.named_parameters())
    grads = torch.autograd.grad(loss, ([] if detach_memory else [memory]) + list(params.values()), allow_unused=True)
    cpu64 = lambda v: None if v is None else v.detach().cpu().double()
    gm = None if detach_memory else cpu64(grads[0])
    return gm, {k: cpu64(v) for k, v in zip(params, grads[0 if detach_memory else 1:])}, seen, roi_backwards[0]


@pytest.fixture(scope="module")
def frame_stage_case():
    """The case of tests/test_roi_backward_gpu.py with its seed rule: the first seed whose fp64 run keeps every ReLU
    pre-activation further from zero than KINK_MARGIN x the CPU fp32 run's worst pre-activation error."""
    from tests import _roi_cases as rc
    from tests.test_roi_backward_gpu import KINK_MARGIN, SEEDS, _frame_stage_case, _frame_stage_grads
    for seed in SEEDS:
        tr, heads, inputs = _frame_stage_case(seed)
        ref = _frame_stage_grads(tr, heads, inputs, "cpu", torch.float64, rc.roi_align_like_ops)
        cpu32 = _frame_stage_grads(tr, heads, inputs, "cpu", torch.float32, rc.roi_align_like_ops)
        if ref[2].abs().min().item() > KINK_MARGIN * (cpu32[2] - ref[2]).abs().max().item():
            return tr, heads, inputs, ref, cpu32
    raise AssertionError("no seed keeps every ReLU pre-activation clear of zero")


@pytest.mark.parametrize("detach_memory", [False, True])
def test_frame_stage_trains_on_the_fused_route(frame_stage_case, detach_memory, monkeypatch):
    """memory.grad and the gradients of dynamic_layer_for_current_query1's parameters against the fp64 CPU run within
    4x the CPU fp32 figure; both the fused DynamicConv backward and roi_align_backward ran.  With the memory detached
    (fixed_pretrained_model) grad_feats is not computed and the head's parameter gradients keep the same bound."""
    from tests.test_roi_backward_gpu import _errors, _rel
    tr, heads, inputs, ref, cpu32 = frame_stage_case
    gm, gp, seen, roi_backwards = _frame_stage_fused(tr, heads, inputs, detach_memory, monkeypatch)
    ym, yp = _errors(cpu32, ref)
    used = [k for k, v in ref[1].items() if v is not None and v.abs().max() > 0]
    assert used and all(gp[k] is not None for k in used)
    worst = max(_rel(gp[k], ref[1][k]) for k in used)
    assert len(seen) == 2, f"the fused DynamicConv backward ran {len(seen)} times for the two roles"
    if detach_memory:
        assert seen == [False, False] and roi_backwards == 0
        print(f"frame_stage, memory detached: head parameters (worst): cpu fp32 {yp:.3e}, gpu {worst:.3e}")
    else:
        assert seen == [True, True] and roi_backwards == 2
        err = _rel(gm, ref[0])
        print(f"frame_stage memory.grad: cpu fp32 {ym:.3e}, gpu {err:.3e}; head parameters (worst): cpu fp32 {yp:.3e}, gpu {worst:.3e}")
        assert err <= YARDSTICK_FACTOR * ym, f"memory.grad: gpu {err:.3e} against 4 x cpu fp32 {ym:.3e}"
    assert worst <= YARDSTICK_FACTOR * yp, f"head parameter gradients: gpu {worst:.3e} against 4 x cpu fp32 {yp:.3e}"


# ---- 10. inference unchanged -----------------------------------------------------------------------------------
def test_inference_is_bit_equal_to_the_raw_forward_entry():
    """ClipRunner under no_grad with ops.dynamic_conv as shipped against the same run with ops.dynamic_conv forced onto
    the forward entry point of the library (no autograd wrapper in between)."""
    from dfx import _lib, ops
    from models.clip_inference import ClipRunner
    from tests.test_models_gpu import _build, _clip
    calls = [0]

    def raw(feats, params, norm1, norm2):
        calls[0] += 1
        K, R, C = feats.shape
        assert feats.is_contiguous() and not torch.is_grad_enabled()
        out = torch.empty_like(feats)
        code = _lib.load().dfx_dynamic_conv_f32(feats.data_ptr(), params.data_ptr(), params.stride(0), norm1.weight.data_ptr(),
                                                norm1.bias.data_ptr(), norm2.weight.data_ptr(), norm2.bias.data_ptr(),
                                                out.data_ptr(), K, R, C, 64, float(norm1.eps),
                                                torch.cuda.current_stream().cuda_stream)
        assert code == 0
        return out

    clip = _clip(4, 21).cuda()
    model, _ = _build("cuda")
    model = model.cuda()
    with torch.no_grad():
        got = ClipRunner(model, micro_batch=2)(clip)
        saved = ops.dynamic_conv
        ops.dynamic_conv = raw
        try:
            want = ClipRunner(model, micro_batch=2)(clip)
        finally:
            ops.dynamic_conv = saved
    assert calls[0] > 0
    assert torch.equal(got["pred_logits"], want["pred_logits"]) and torch.equal(got["pred_boxes"], want["pred_boxes"])
