"""GPU: the fused MSDA backward (csrc/msda_fused_backward.hip) against the fp64 statements of tests/_msda_fused_cases.py,
the autograd surface of ``dfx.ops.msda_fused``, ``MSDeformAttn`` and a decoder layer on the fused route in grad mode, and
the routes that must stay as they were.  How the operator cases stay clear of the bilinear kinks: tests/_msda_fused_cases.py;
the module tests, whose offsets come out of a Linear, zero the rows of grad_out of the queries that are not clear."""
import copy

import pytest
import torch

from tests import _msda_fused_cases as fc

pytestmark = pytest.mark.gpu

YARDSTICK_FACTOR = 4      # the GPU may be this many times the CPU's own fp32 error (the project's factor: test_roi_backward_gpu)
KINK_FACTOR, MAX_UNCLEAR = 8, 0.05
FWD_TOL = dict(rtol=1e-4, atol=5e-5)      # fused against unfused forward (tests/test_msda_gpu.py)


def _gpu_inputs(case, requires=fc.GRADS, strided=False):
    t = {k: case[k].detach().cuda() for k in fc.GRADS}
    if strided:       # offsets and logits as column slices of one wider buffer: row stride > row length
        wo, wl = t["offsets"].shape[2], t["logits"].shape[2]
        wide = torch.zeros(*t["offsets"].shape[:2], wo + wl + 8, device="cuda")
        wide[..., :wo], wide[..., wo:wo + wl] = t["offsets"], t["logits"]
        t["offsets"], t["logits"] = wide[..., :wo], wide[..., wo:wo + wl]
        assert t["offsets"].stride(1) > wo and not t["logits"].is_contiguous()
    for k in requires:
        t[k].requires_grad_()
    return t


def _run(case, requires=fc.GRADS, strided=False, grad_out=None):
    """(out, {name: gradient or None}) of ops.msda_fused in grad mode on the GPU."""
    from dfx import ops
    t = _gpu_inputs(case, requires, strided)
    out = ops.msda_fused(t["value"], case["shapes"].cuda(), case["lsi"].cuda(), t["ref"], t["offsets"], t["logits"], case["L"], fc.P)
    assert out.grad_fn is not None
    out.backward(case["grad_out"].cuda() if grad_out is None else grad_out)
    torch.cuda.synchronize()
    return out.detach(), {k: t[k].grad for k in fc.GRADS}


def _compare(ref, cpu32, got, names, what=""):
    worst = []
    for k in names:
        yard, err = fc.rel_err(cpu32[k], ref[k]), fc.rel_err(got[k].cpu(), ref[k])
        print(f"  {what}d{k}: cpu fp32 {yard:.3e}, gpu {err:.3e}, max |ref| {ref[k].abs().max().item():.3e}")
        if err > YARDSTICK_FACTOR * yard:
            worst.append(f"d{k}: gpu {err:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}")
    assert not worst, "; ".join(worst)


# ---- 1. operator against fp64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,ref_dim,N,Lq,strided", fc.OPERATOR_CASES)
def test_operator_matches_fp64_within_the_measured_yardstick(levels, ref_dim, N, Lq, strided):
    """Every gradient, in full, against the fp64 CPU restatement (which the CPU file checks against autograd), error
    relative to that gradient's largest magnitude.  The yardstick is the same statement on the CPU in fp32 against fp64;
    the GPU may be at most 4x that per gradient (two fp32 evaluations of one computation that differ in summation order)."""
    case = fc.make_case(levels, ref_dim, N, Lq)
    print(f"case ({levels},{ref_dim},{N},{Lq}): coordinate noise {case['noise']:.2e}")
    out, grads = _run(case, strided=strided)
    want = fc.reference_forward(*(case[k].double() for k in ("value", "ref", "offsets", "logits")), case["sizes"])
    assert torch.allclose(out.cpu().double(), want, **FWD_TOL)
    for k in fc.GRADS:
        assert grads[k].shape == case[k].shape, k
    _compare(fc.restated_backward(case), fc.autograd_backward(case, torch.float32), grads, fc.GRADS)


# ---- 2. forward unchanged --------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,ref_dim,N,Lq,strided", [(4, 2, 2, 300, False), (1, 4, 2, 300, False), (2, 2, 3, 37, True)])
def test_forward_is_bit_equal_to_the_inference_entry(levels, ref_dim, N, Lq, strided):
    from dfx import ops
    case = fc.make_case(levels, ref_dim, N, Lq)
    t = _gpu_inputs(case, requires=(), strided=strided)
    shapes, lsi = case["shapes"].cuda(), case["lsi"].cuda()
    want = ops.msda_fused_forward(t["value"], shapes, lsi, t["ref"], torch.cat([t["offsets"], t["logits"]], -1).contiguous(),
                                  case["L"], fc.P)
    plain = ops.msda_fused(t["value"], shapes, lsi, t["ref"], t["offsets"], t["logits"], case["L"], fc.P)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, want)
    tg = _gpu_inputs(case, strided=strided)
    tracked = ops.msda_fused(tg["value"], shapes, lsi, tg["ref"], tg["offsets"], tg["logits"], case["L"], fc.P)
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), want)


# ---- 3. autograd surface ---------------------------------------------------------------------------------------
def test_a_node_only_when_there_is_a_gradient_to_carry():
    from dfx import ops
    case = fc.make_case(2, 4, 3, 37)
    shapes, lsi = case["shapes"].cuda(), case["lsi"].cuda()
    for name in fc.GRADS:
        t = _gpu_inputs(case, requires=(name,))
        out = ops.msda_fused(t["value"], shapes, lsi, t["ref"], t["offsets"], t["logits"], 2, fc.P)
        assert out.grad_fn is not None, name
        with torch.no_grad():
            quiet = ops.msda_fused(t["value"], shapes, lsi, t["ref"], t["offsets"], t["logits"], 2, fc.P)
        assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, out.detach())


def test_unrequested_gradients_are_skipped_and_the_others_unchanged(monkeypatch):
    """value detached: need_value is False, grad_value is None and no [N,S,M,D] buffer exists; need_ref likewise."""
    from dfx import ops
    case = fc.make_case(4, 4, 3, 37)
    seen, real = [], ops.msda_fused_backward

    def spy(*a, need_value=True, need_ref=False):
        res = real(*a, need_value=need_value, need_ref=need_ref)
        seen.append((need_value, need_ref, res[0] is None, res[3] is None))
        return res

    monkeypatch.setattr(ops, "msda_fused_backward", spy)
    _, full = _run(case)
    _, no_value = _run(case, requires=("offsets", "logits", "ref"))
    _, no_ref = _run(case, requires=("value", "offsets", "logits"))
    _, neither = _run(case, requires=("offsets", "logits"))
    assert seen == [(True, True, False, False), (False, True, True, False), (True, False, False, True), (False, False, True, True)]
    assert no_value["value"] is None and no_ref["ref"] is None and neither["value"] is None and neither["ref"] is None
    for run, names in ((no_value, ("offsets", "logits", "ref")), (no_ref, ("offsets", "logits")), (neither, ("offsets", "logits"))):
        for k in names:
            assert torch.equal(run[k], full[k]), k
    assert fc.rel_err(no_ref["value"], full["value"]) < 1e-5          # float atomics: order-dependent last bits


# ---- 4. determinism --------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_in_the_small_gradients():
    case = fc.make_case(4, 4, 2, 1100)
    _, a = _run(case)
    _, b = _run(case)
    for k in ("offsets", "logits", "ref"):
        assert torch.equal(a[k], b[k]), k


# ---- 5. exact cases --------------------------------------------------------------------------------------------
def test_zero_grad_out_gives_exact_zeros():
    case = fc.make_case(3, 4, 3, 37)
    _, grads = _run(case, grad_out=torch.zeros(3, 37, 256, device="cuda"))
    for k in fc.GRADS:
        assert grads[k].abs().max() == 0, k


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_samples_outside_the_map_give_exact_zeros(ref_dim):
    from dfx import ops
    case = fc.make_case(2, ref_dim, 3, 37)
    t = _gpu_inputs(case, requires=())
    far = (t["offsets"].abs() + 1) * 1000           # every location far beyond the map, on the positive side
    res = ops.msda_fused_backward(case["grad_out"].cuda(), t["value"], case["shapes"].cuda(), case["lsi"].cuda(), t["ref"],
                                  far, t["logits"], need_value=True, need_ref=True)
    for g in res:
        assert g.abs().max() == 0


def test_no_queries_give_empty_results():
    from dfx import ops
    case = fc.make_case(2, 2, 3, 37)
    v, shapes, lsi = case["value"].cuda(), case["shapes"].cuda(), case["lsi"].cuda()
    z = lambda *s: torch.zeros(*s, device="cuda")
    gv, go, gl, gr = ops.msda_fused_backward(z(3, 0, 256), v, shapes, lsi, z(3, 0, 2, 2), z(3, 0, 128), z(3, 0, 64),
                                             need_value=True, need_ref=True)
    assert gv.shape == v.shape and gv.abs().max() == 0
    assert go.shape == (3, 0, 128) and gl.shape == (3, 0, 64) and gr.shape == (3, 0, 2, 2)
    assert ops.msda_fused(v, shapes, lsi, z(3, 0, 2, 2), z(3, 0, 128), z(3, 0, 64), 2, 4).shape == (3, 0, 256)


def test_strided_rows_give_gradients_of_the_inputs_shape_equal_to_the_contiguous_call():
    case = fc.make_case(4, 4, 3, 37)
    _, want = _run(case)
    _, got = _run(case, strided=True)
    for k in ("offsets", "logits", "ref"):
        assert got[k].shape == case[k].shape and torch.equal(got[k], want[k]), k


def _raw_backward(case, t, S, value_ptr, pad):
    """dfx_msda_fused_backward_f32 itself, gradient rows `pad` floats wider than the row, the buffers pre-filled with 7:
    -> (return code, grad_off, grad_logits, grad_ref) with the padded columns still in place."""
    from dfx import _lib
    N, Lq, L = case["ref"].shape[:3]
    wo, wl = t["offsets"].shape[2], t["logits"].shape[2]
    go = torch.full((N, Lq, wo + pad), 7.0, device="cuda")
    gl = torch.full((N, Lq, wl + pad), 7.0, device="cuda")
    gr = torch.full((N, Lq, L, case["ref"].shape[3]), 7.0, device="cuda")
    shapes, lsi, grad_out = case["shapes"].cuda(), case["lsi"].cuda(), case["grad_out"].cuda()      # alive across the call
    rc = _lib.load().dfx_msda_fused_backward_f32(
        value_ptr, shapes.data_ptr(), lsi.data_ptr(), t["ref"].data_ptr(), case["ref"].shape[3],
        t["offsets"].data_ptr(), wo, t["logits"].data_ptr(), wl, grad_out.data_ptr(), N, S, fc.M, fc.D, L, Lq, fc.P,
        None, go.data_ptr(), wo + pad, gl.data_ptr(), wl + pad, gr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, go, gl, gr


def test_entry_point_writes_padded_gradient_rows_and_zeros_for_an_empty_map():
    """The C entry with grad_off / grad_logits row strides larger than the row: the row part equals the packed call of
    dfx.ops, the padding is not touched.  S == 0 writes zeros to the three small gradients (and, like the forward
    entry, still refuses a null value pointer)."""
    from dfx import _lib, ops
    case = fc.make_case(3, 4, 3, 37)
    t = _gpu_inputs(case, requires=())
    wo, wl = t["offsets"].shape[2], t["logits"].shape[2]
    S = case["value"].shape[1]
    want = ops.msda_fused_backward(case["grad_out"].cuda(), t["value"], case["shapes"].cuda(), case["lsi"].cuda(), t["ref"],
                                   t["offsets"], t["logits"], need_value=False, need_ref=True)
    rc, go, gl, gr = _raw_backward(case, t, S, t["value"].data_ptr(), 12)
    assert rc == 0
    assert torch.equal(go[..., :wo], want[1]) and torch.equal(gl[..., :wl], want[2]) and torch.equal(gr, want[3])
    assert (go[..., wo:] == 7).all() and (gl[..., wl:] == 7).all()
    rc, go, gl, gr = _raw_backward(case, t, 0, t["value"].data_ptr(), 12)
    assert rc == 0
    assert go[..., :wo].abs().max() == 0 and gl[..., :wl].abs().max() == 0 and gr.abs().max() == 0
    assert (go[..., wo:] == 7).all() and (gl[..., wl:] == 7).all()
    rc, *_ = _raw_backward(case, t, 0, None, 0)
    assert rc != 0 and b"null pointer" in _lib.load().dfx_last_error()
    rc, *_ = _raw_backward(case, t, S, t["value"].data_ptr(), 2)          # stride not a multiple of 4
    assert rc != 0 and b"strides" in _lib.load().dfx_last_error()


# ---- 6. the module ---------------------------------------------------------------------------------------------
class _CoreOp:
    """Stand-in for MSDeformAttnFunction on CPU tensors: the differentiable plain-tensor statement; records the locations."""

    def __init__(self, sizes):
        self.sizes, self.locs = sizes, []

    def apply(self, value, shapes, lsi, loc, aw, step):
        self.locs.append(loc.detach().double())
        return fc.ms_deform_attn_core_pytorch(value, self.sizes, loc, aw)


class _Forbidden:
    def apply(self, *a):
        raise AssertionError("MSDeformAttnFunction called on the fused training route")


class _Counting:
    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def apply(self, *a):
        self.calls += 1
        return self.inner.apply(*a)


def _unclear_queries(loc64, loc32, sizes):
    """[N,Lq] mask of the queries with a pixel coordinate within KINK_FACTOR x (worst fp32 - fp64 coordinate difference)
    of an integer in the fp64 run, and that difference."""
    wh = torch.as_tensor([(w, h) for h, w in sizes], dtype=torch.float64)[None, None, None, :, None, :]
    p64, p32 = loc64 * wh - 0.5, loc32 * wh - 0.5
    noise = (p32 - p64).abs().max().item()
    near = (p64 - torch.round(p64)).abs() < KINK_FACTOR * noise
    return near.flatten(2).any(-1), noise


def _leaves_run(fn, leaves, params, gout, device, dtype):
    """Run fn(leaves on device) -> out; (out, {name: gradient}) of sum(out * gout) for every leaf and parameter."""
    t = {k: v.detach().to(device=device, dtype=dtype).requires_grad_() for k, v in leaves.items()}
    out = fn(t)
    if gout is None:
        return out.detach().cpu().double(), None
    named = dict(t, **params)
    grads = torch.autograd.grad((out * gout.to(device=device, dtype=dtype)).sum(), list(named.values()), allow_unused=True)
    return out.detach().cpu().double(), {k: g.detach().cpu().double() for k, g in zip(named, grads) if g is not None}


MODULE_SIZES = {1: [(20, 31)], 4: [(16, 20), (8, 10), (4, 5), (2, 3)]}


def _module_case(L, ref_dim):
    from models.ops.modules import MSDeformAttn
    torch.manual_seed(10 * L + ref_dim)
    m = MSDeformAttn(256, L, 8, 4).train()
    with torch.no_grad():     # the initialisation zeroes these; give the sampling something to differentiate
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    sizes = MODULE_SIZES[L]
    shapes, lsi = fc.level_tensors(sizes)
    N, Lq, S = 2, 50, int((shapes[:, 0] * shapes[:, 1]).sum())
    g = torch.Generator().manual_seed(100 + 10 * L + ref_dim)
    ref = 0.1 + 0.8 * torch.rand(N, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = 0.2 + 0.4 * torch.rand(N, Lq, L, 2, generator=g)
    leaves = {"query": torch.randn(N, Lq, 256, generator=g), "reference_points": ref, "input_flatten": torch.randn(N, S, 256, generator=g)}
    return m, leaves, torch.randn(N, Lq, 256, generator=g), sizes, shapes, lsi


def _module_on(m, shapes, lsi, device, dtype):
    mod = copy.deepcopy(m).to(device=device, dtype=dtype)
    sh, ls = shapes.to(device), lsi.to(device)
    return mod, (lambda t: mod(t["query"], t["reference_points"], t["input_flatten"], sh, ls))


def _cpu_yardsticks(run_on, sizes, leaves, gout, monkeypatch):
    """fp64 and fp32 CPU runs with the rows of grad_out of the unclear queries zeroed -> (keep mask, ref grads, cpu32 grads)."""
    import models.ops.functions.ms_deform_attn_func as f
    locs = {}
    for dt in (torch.float64, torch.float32):
        op = _CoreOp(sizes)
        monkeypatch.setattr(f, "MSDeformAttnFunction", op)
        _, fn, _ = run_on("cpu", dt)
        _leaves_run(fn, leaves, {}, None, "cpu", dt)
        locs[dt] = op.locs[-1]
    unclear, noise = _unclear_queries(locs[torch.float64], locs[torch.float32], sizes)
    fraction = unclear.float().mean().item()
    print(f"  coordinate noise {noise:.2e}, {fraction:.2%} of the queries unclear")
    assert fraction <= MAX_UNCLEAR
    masked = gout * (~unclear)[..., None]
    res = {}
    for dt in (torch.float64, torch.float32):
        monkeypatch.setattr(f, "MSDeformAttnFunction", _CoreOp(sizes))
        mod, fn, _ = run_on("cpu", dt)
        res[dt] = _leaves_run(fn, leaves, dict(mod.named_parameters()), masked, "cpu", dt)[1]
    return masked, res[torch.float64], res[torch.float32]


@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("L", [1, 4])
def test_module_trains_on_the_fused_route(L, ref_dim, monkeypatch):
    """MSDeformAttn(256, L, 8, 4).train(): gradients of every parameter, the query, input_flatten and reference_points
    against the fp64 CPU module within 4x the CPU fp32 figure; the fused backward ran and MSDeformAttnFunction did not.
    With MSDA_TRAIN off the opposite, the sampled values within the forward tests' tolerance of each other."""
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    from models.ops.modules import ms_deform_attn as mod_file
    m, leaves, gout, sizes, shapes, lsi = _module_case(L, ref_dim)
    real = f.MSDeformAttnFunction

    def run_on(device, dt):
        mod, fn = _module_on(m, shapes, lsi, device, dt)
        return mod, fn, None

    masked, ref, cpu32 = _cpu_yardsticks(run_on, sizes, leaves, gout, monkeypatch)

    calls, real_bwd = [0], ops.msda_fused_backward

    def bwd_spy(*a, **k):
        calls[0] += 1
        return real_bwd(*a, **k)

    def gpu_run():
        mod, fn = _module_on(m, shapes, lsi, "cuda", torch.float32)
        sampled = []
        mod.output_proj.register_forward_pre_hook(lambda _, args: sampled.append(args[0].detach()))
        out, grads = _leaves_run(fn, leaves, dict(mod.named_parameters()), masked, "cuda", torch.float32)
        return out, grads, sampled[0]

    monkeypatch.setattr(ops, "msda_fused_backward", bwd_spy)
    monkeypatch.setattr(f, "MSDeformAttnFunction", _Forbidden())
    assert mod_file.MSDA_TRAIN
    fused_out, fused, fused_sampled = gpu_run()
    assert calls[0] == 1
    assert set(fused) == set(ref), set(ref) ^ set(fused)
    _compare(ref, cpu32, fused, sorted(ref), what="fused ")

    counting = _Counting(real)
    monkeypatch.setattr(f, "MSDeformAttnFunction", counting)
    monkeypatch.setattr(mod_file, "MSDA_TRAIN", False)
    unfused_out, unfused, unfused_sampled = gpu_run()
    assert calls[0] == 1 and counting.calls == 1
    assert torch.allclose(fused_out, unfused_out, **FWD_TOL), (fused_out - unfused_out).abs().max().item()
    assert torch.allclose(fused_sampled, unfused_sampled, **FWD_TOL), (fused_sampled - unfused_sampled).abs().max().item()


# ---- 7. routes left alone --------------------------------------------------------------------------------------
def test_autocast_fp64_and_the_flat_read_stay_on_the_operator(monkeypatch):
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    from models.ops.modules import MSDeformAttn

    def never(*a, **k):
        raise AssertionError("dfx.ops.msda_fused on a route it does not cover")

    monkeypatch.setattr(ops, "msda_fused", never)
    counting = _Counting(f.MSDeformAttnFunction)
    monkeypatch.setattr(f, "MSDeformAttnFunction", counting)
    m, leaves, gout, sizes, shapes, lsi = _module_case(1, 2)
    shapes, lsi = shapes.cuda(), lsi.cuda()
    q, r, x = (leaves[k].cuda() for k in ("query", "reference_points", "input_flatten"))
    mc = copy.deepcopy(m).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = mc(q.clone().requires_grad_(), r, x, shapes, lsi)
    out.float().sum().backward()
    assert counting.calls == 1
    md = copy.deepcopy(m).cuda().double()
    md(q.double().requires_grad_(), r.double(), x.double(), shapes, lsi).sum().backward()
    assert counting.calls == 2
    flat = torch.rand(1, 50, 3, 2, device="cuda")           # Lr = 3 != L = 1: the temporal decoder's flat read
    mc(q[:1].clone().requires_grad_(), flat, x[:1], shapes, lsi).sum().backward()
    assert counting.calls == 3


@pytest.mark.parametrize("L", [1, 4])
def test_no_grad_is_bit_equal_to_the_inference_route(L, monkeypatch):
    """Under no_grad the module's output equals its own output with dfx.ops.msda_fused removed (nothing of the new route
    runs) and the sampled values are those of ops.msda_fused_forward on the joint projection."""
    from dfx import ops
    m, leaves, gout, sizes, shapes, lsi = _module_case(L, 2)
    mc = copy.deepcopy(m).cuda()
    shapes, lsi = shapes.cuda(), lsi.cuda()
    q, r, x = (leaves[k].cuda().requires_grad_() for k in ("query", "reference_points", "input_flatten"))
    seen, real = [], ops.msda_fused_forward

    def spy(*a):
        seen.append(real(*a))
        return seen[-1]

    monkeypatch.setattr(ops, "msda_fused_forward", spy)
    with torch.no_grad():
        got = mc(q, r, x, shapes, lsi)
        monkeypatch.delattr(ops, "msda_fused")
        monkeypatch.delattr(ops, "msda_fused_backward")
        want = mc(q, r, x, shapes, lsi)
        assert len(seen) == 2 and torch.equal(seen[0], seen[1])
        assert torch.equal(mc.output_proj(seen[0]), got)
    assert got.grad_fn is None and torch.equal(got, want)


# ---- 8. a decoder layer ----------------------------------------------------------------------------------------
def test_decoder_layer_trains_on_the_fused_route(monkeypatch):
    """DeformableTransformerDecoderLayer in train mode with dropout 0, two frames, Lq = 30: parameter gradients through
    self-attention, the fused cross-attention route and the FFN against fp64 within 4x the CPU fp32 figure.  A row of
    the layer's grad_out reaches cross_attn's output row of the same query only (LayerNorm and FFN work per row), so
    zeroing the rows of the unclear queries keeps their samples out of every gradient."""
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    from models.transformer_layers import DeformableTransformerDecoderLayer
    torch.manual_seed(5)
    layer = DeformableTransformerDecoderLayer(256, 1024, 0.0, "relu", 4, 8, 4).train()
    with torch.no_grad():
        layer.cross_attn.sampling_offsets.weight.normal_(0, 0.02)
        layer.cross_attn.attention_weights.weight.normal_(0, 0.02)
    sizes = MODULE_SIZES[4]
    shapes, lsi = fc.level_tensors(sizes)
    N, Lq, S = 2, 30, int((shapes[:, 0] * shapes[:, 1]).sum())
    g = torch.Generator().manual_seed(6)
    leaves = {"tgt": torch.randn(N, Lq, 256, generator=g), "query_pos": torch.randn(N, Lq, 256, generator=g),
              "src": torch.randn(N, S, 256, generator=g)}
    ref_points = 0.1 + 0.8 * torch.rand(N, Lq, 4, 2, generator=g)
    gout = torch.randn(N, Lq, 256, generator=g)

    def run_on(device, dt):
        mod = copy.deepcopy(layer).to(device=device, dtype=dt)
        rp, sh, ls = ref_points.to(device=device, dtype=dt), shapes.to(device), lsi.to(device)
        return mod, (lambda t: mod(t["tgt"], t["query_pos"], rp, t["src"], sh, ls)), None

    masked, ref, cpu32 = _cpu_yardsticks(run_on, sizes, leaves, gout, monkeypatch)
    calls, real_bwd = [0], ops.msda_fused_backward

    def bwd_spy(*a, **k):
        calls[0] += 1
        return real_bwd(*a, **k)

    monkeypatch.setattr(ops, "msda_fused_backward", bwd_spy)
    monkeypatch.setattr(f, "MSDeformAttnFunction", _Forbidden())
    mod, fn, _ = run_on("cuda", torch.float32)
    _, got = _leaves_run(fn, leaves, dict(mod.named_parameters()), masked, "cuda", torch.float32)
    assert calls[0] == 1
    assert set(got) == set(ref), set(ref) ^ set(got)
    _compare(ref, cpu32, got, sorted(ref), what="layer ")
