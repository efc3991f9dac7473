"""GPU: the deterministic training mode (csrc/fixed_sum.h) - grad_value of the fused MSDA backward in its
level (LDS) and global form and grad_input of the channels-last RoIAlign summed in 64-bit fixed point.

What is asserted.  Accuracy: the bounds the float routes are held to (tests/test_msda_level_backward_gpu.py: at most
YARDSTICK_FACTOR x the CPU's own fp32 error against fp64, ATOMIC_TOL of the float route; tests/_roi_cases.py: the exact
family bit for bit, the random family inside random_bound).  Reproducibility: the same bits twice, the same bits under a
permutation of the queries / RoIs, exact scaling by a power of two, the edges (zeros, one writer, NaN for a non-finite
grad_out, argument checks before any launch), the routes the mode selects and the routes that have no twin.
The float routes are never asserted to DIFFER between calls: that would be a flaky test."""
import warnings

import pytest
import torch

from tests import _msda_fused_cases as fc
from tests import _msda_level_bwd_cases as lc
from tests import _roi_cases as rc
from tests import test_msda_level_backward_gpu as lt

pytestmark = pytest.mark.gpu

YARDSTICK_FACTOR, ATOMIC_TOL = lt.YARDSTICK_FACTOR, lt.ATOMIC_TOL
LEVEL_FIXED, FUSED_FIXED, ROI_FIXED = ("dfx_msda_level_grad_value_fixed_f32", "dfx_msda_fused_backward_fixed_f32",
                                       "dfx_roi_align_backward_nhwc_fixed_f32")
LEVEL_FLOAT, FUSED_FLOAT, ROI_FLOAT = ("dfx_msda_level_grad_value_f32", "dfx_msda_fused_backward_f32",
                                       "dfx_roi_align_backward_nhwc_f32")
COLLIDE = (20, 31, 1, 1100)
SMALL = (5, 7, 3, 37)
SIZE, SCALE = 7, 1 / 32


@pytest.fixture()
def flag(monkeypatch):
    """``flag(on, warn_only)`` sets torch's deterministic flag; restored at teardown."""
    from dfx import ops
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setenv("CUBLAS_WORKSPACE_CONFIG", ":4096:8")      # what torch asks of its own GEMMs under the flag
    monkeypatch.setattr(ops, "_ALERTED", set())
    yield lambda on=True, warn_only=False: torch.use_deterministic_algorithms(on, warn_only=warn_only)
    torch.use_deterministic_algorithms(was[0], warn_only=was[1])


def _level(t, N, H, W, deterministic=True):
    from dfx import ops
    out = ops.msda_level_grad_value(t["grad_out"], t["ref"], t["offsets"], t["logits"], N, H, W, deterministic=deterministic)
    torch.cuda.synchronize()
    return out


def _global(case, t=None, deterministic=True, **kw):
    """ops.msda_fused_backward below the level threshold: the global form (asserted by the route tests below)."""
    from dfx import ops
    t = t or lt._gpu_rows(case)
    assert case["value"].shape[0] * t["ref"].shape[1] < ops.LEVEL_BWD_MIN_QUERIES
    res = ops.msda_fused_backward(t["grad_out"], case["value"].cuda(), case["shapes"].cuda(), case["lsi"].cuda(), t["ref"],
                                  t["offsets"], t["logits"], need_value=True, need_ref=True, deterministic=deterministic, **kw)
    torch.cuda.synchronize()
    return res


def _permuted(t, seed):
    """One random permutation of the queries of each frame, applied to the rows of grad_out, ref, offsets and logits."""
    g = torch.Generator().manual_seed(seed)
    N, Lq = t["ref"].shape[:2]
    perms = [torch.randperm(Lq, generator=g).cuda() for _ in range(N)]
    assert any(not torch.equal(p, torch.arange(Lq, device="cuda")) for p in perms)
    return {k: torch.stack([v[n][perms[n]] for n in range(N)]).contiguous() for k, v in t.items()}


def _roi_case(sr=2, aligned=True, seed=5, C=64, H=13, W=21):
    rois = rc.random_family(H, W, aligned, sr, seed=seed, per_image=60)
    go = torch.randn(rois.shape[0], C, SIZE, SIZE, generator=torch.Generator().manual_seed(11))
    return rois, go, (2, C, H, W)


def _roi_fixed(go_nchw, rois, shape, sr=2, aligned=True, deterministic=True):
    """grad_input [N,C,H,W] on the CPU from the channels-last entry."""
    from dfx import ops
    N, C, H, W = shape
    tok = go_nchw.flatten(2).transpose(1, 2).contiguous().cuda()
    got = ops.roi_align_backward(tok, rois.cuda(), (N, H, W, C), SIZE, SCALE, sr, aligned, channels_last=True,
                                 deterministic=deterministic)
    torch.cuda.synchronize()
    return got.permute(0, 3, 1, 2).cpu()


# ---- 1. accuracy of the level form -----------------------------------------------------------------------------
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("H,W,N,Lq,strided", lc.KERNEL_CASES)
def test_level_form_matches_fp64_and_the_float_route(H, W, N, Lq, strided, ref_dim):
    case = lc.make_level_case(H, W, ref_dim, N, Lq)
    want, cpu32 = lc.references(H, W, ref_dim, N, Lq)
    t = lt._gpu_rows(case, strided)
    got = _level(t, N, H, W)
    assert got.shape == (N, H * W, 8, 32) and got.is_contiguous()
    flt = _level(t, N, H, W, deterministic=False)
    lt._within_yardstick(f"fixed ({H}x{W}, N {N}, Lq {Lq}, ref_dim {ref_dim})", got, want, cpu32, flt)
    diff = fc.rel_err(got, flt)
    print(f"  against the float route {diff:.3e}")
    assert diff < ATOMIC_TOL


def test_level_form_with_every_query_adding_into_the_same_tokens():
    """The case that tests the bound n: 1100 queries x 4 points meet in the same few accumulators."""
    H, W, N, Lq = COLLIDE
    case = lc.make_level_case(H, W, 2, N, Lq, True)
    want, cpu32 = lc.references(H, W, 2, N, Lq, True)
    t = lt._gpu_rows(case)
    got, flt = _level(t, N, H, W), _level(t, N, H, W, deterministic=False)
    lt._within_yardstick("fixed, collisions", got, want, cpu32, flt)
    assert fc.rel_err(got, flt) < ATOMIC_TOL


# ---- 2. accuracy of the global form ----------------------------------------------------------------------------
def _global_cases():
    two = fc.make_case(2, 2, 3, 37)
    one = lc.make_level_case(*SMALL[:2], 2, *SMALL[2:])
    return (("two levels", two, fc.restated_backward(two)["value"], fc.autograd_backward(two, torch.float32)["value"]),
            ("one level below the threshold", one, *lc.references(*SMALL[:2], 2, *SMALL[2:])))


def test_global_form_matches_fp64_and_the_float_route():
    for what, case, want, cpu32 in _global_cases():
        fixed, flt = _global(case), _global(case, deterministic=False)
        lt._within_yardstick(f"fixed, global, {what}", fixed[0], want, cpu32, flt[0])
        assert fc.rel_err(fixed[0], flt[0]) < ATOMIC_TOL
        for name, a, b in zip(("grad_off", "grad_logits", "grad_ref"), fixed[1:], flt[1:]):
            assert torch.equal(a, b), f"{what}: {name} changed with the mode"


# ---- 3. the same bits twice ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N,Lq,collide", [COLLIDE + (True,), (50, 84, 1, 1100, False)])
def test_two_calls_give_the_same_bits(H, W, N, Lq, collide):
    case = lc.make_level_case(H, W, 2, N, Lq, collide)
    t = lt._gpu_rows(case)
    assert torch.equal(_level(t, N, H, W), _level(t, N, H, W)), "level form"
    assert torch.equal(_global(case, t)[0], _global(case, t)[0]), "global form"


def test_two_roi_calls_give_the_same_bits():
    rois, go, shape = _roi_case()
    assert torch.equal(_roi_fixed(go, rois, shape), _roi_fixed(go, rois, shape))


# ---- 4. order independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N,Lq,collide", [(20, 31, 2, 1100, False), COLLIDE + (True,)])
def test_level_form_does_not_depend_on_the_query_order(H, W, N, Lq, collide):
    t = lt._gpu_rows(lc.make_level_case(H, W, 2, N, Lq, collide))
    if collide:     # the builder gives every query the same sample points; the rows still differ in logits and grad_out
        assert not torch.equal(t["grad_out"][:, 0], t["grad_out"][:, 1])
    assert torch.equal(_level(t, N, H, W), _level(_permuted(t, 1), N, H, W))


def test_global_form_does_not_depend_on_the_query_order():
    for case in (fc.make_case(2, 2, 3, 37), lc.make_level_case(20, 31, 2, 2, 1100)):
        t = lt._gpu_rows(case)
        assert torch.equal(_global(case, t)[0], _global(case, _permuted(t, 2))[0])


def test_roi_sum_does_not_depend_on_the_roi_order():
    rois, go, shape = _roi_case()
    perm = torch.randperm(rois.shape[0], generator=torch.Generator().manual_seed(3))
    assert torch.equal(_roi_fixed(go, rois, shape), _roi_fixed(go[perm], rois[perm], shape))


# ---- 5. scaling by a power of two is exact ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, -40])
def test_scaling_grad_out_by_a_power_of_two_scales_the_result_exactly(k):
    H, W, N, Lq = SMALL
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = lt._gpu_rows(case)
    scaled = dict(t, grad_out=t["grad_out"] * 2.0 ** k)
    base = _level(t, N, H, W)
    assert base.abs().max() > 0
    assert torch.equal(_level(scaled, N, H, W), base * 2.0 ** k), "level form"
    assert torch.equal(_global(case, scaled)[0], _global(case, t)[0] * 2.0 ** k), "global form"
    x, rois, go = rc.exact_family()
    assert torch.equal(_roi_fixed(go * 2.0 ** k, rois, tuple(x.shape)), _roi_fixed(go, rois, tuple(x.shape)) * 2.0 ** k), "RoIAlign"


# ---- 6. edges --------------------------------------------------------------------------------------------------
def _raw_level(t, ref_dim, N, H, W, Lq, grad_value_ptr, scratch_ptr, off_pitch=None, logit_pitch=None):
    from dfx import _lib
    rc_ = _lib.load().dfx_msda_level_grad_value_fixed_f32(
        t["ref"].data_ptr(), ref_dim, t["offsets"].data_ptr(), t["offsets"].stride(1) if off_pitch is None else off_pitch,
        t["logits"].data_ptr(), t["logits"].stride(1) if logit_pitch is None else logit_pitch, t["grad_out"].data_ptr(),
        N, H, W, Lq, grad_value_ptr, scratch_ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc_


def _scratch():
    return torch.full((4,), 0x55555555, dtype=torch.int32, device="cuda")     # the entry clears it itself


def _untouched(buf):
    return bool((buf[:64] == 7).all() and (buf[-64:] == 7).all())


def test_level_entry_writes_every_element_once_and_nothing_else():
    H, W, N, Lq = 5, 7, 9, 37
    t = lt._gpu_rows(lc.make_level_case(H, W, 2, N, Lq))
    buf, inside = lt._embedded(N, H * W)
    assert _raw_level(t, 2, N, H, W, Lq, inside.data_ptr(), _scratch().data_ptr()) == 0
    assert _untouched(buf) and not (inside == 7).any()
    assert torch.equal(inside, _level(t, N, H, W))


def test_edges_give_exact_zeros():
    H, W, N, Lq = SMALL
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = lt._gpu_rows(case)
    zero = dict(t, grad_out=torch.zeros_like(t["grad_out"]))
    empty = {k: v[:, :0].contiguous() for k, v in t.items()}
    far = dict(t, offsets=(t["offsets"].abs() + 1) * 1000)         # every location thousands of pixels beyond the map
    for what, rows, lq in (("zero grad_out", zero, Lq), ("no queries", empty, 0), ("far outside", far, Lq)):
        buf, inside = lt._embedded(N, H * W)
        assert _raw_level(rows, 2, N, H, W, lq, inside.data_ptr(), _scratch().data_ptr(), 64, 32) == 0, what
        assert inside.abs().max() == 0 and _untouched(buf), f"level form, {what}"
        got = _global(case, rows)
        assert got[0].shape == case["value"].shape and got[0].abs().max() == 0, f"global form, {what}"
    assert _level(far, N, H, W).abs().max() == 0 and _level(dict(far, offsets=-far["offsets"]), N, H, W).abs().max() == 0


def test_one_inf_in_grad_out_makes_every_element_nan():
    H, W, N, Lq = SMALL
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = lt._gpu_rows(case)
    for bad in (float("inf"), float("nan")):
        go = t["grad_out"].clone()
        go[1, 5, 77] = bad
        rows = dict(t, grad_out=go)
        assert torch.isnan(_level(rows, N, H, W)).all(), "level form"
        assert torch.isnan(_global(case, rows)[0]).all(), "global form"
    rois, go, shape = _roi_case()
    go = go.clone()
    go[3, 2, 1, 1] = float("inf")
    assert torch.isnan(_roi_fixed(go, rois, shape)).all(), "RoIAlign"


def test_fixed_entries_reject_bad_arguments_before_any_launch():
    from dfx import _lib
    lib = _lib.load()
    H, W, N, Lq = SMALL
    case = lc.make_level_case(H, W, 2, N, Lq)
    t = lt._gpu_rows(case)
    buf = torch.full((N * 60 * 100 * 256,), 7.0, device="cuda")         # large enough for the level that is refused
    sc = _scratch()
    err = lib.dfx_last_error
    assert _raw_level(t, 2, N, 60, 100, Lq, buf.data_ptr(), sc.data_ptr()) != 0 and b"does not fit" in err()
    assert _raw_level(t, 3, N, H, W, Lq, buf.data_ptr(), sc.data_ptr()) != 0 and b"ref_dim" in err()
    assert _raw_level(t, 2, N, H, W, Lq, buf.data_ptr(), sc.data_ptr(), off_pitch=66) != 0 and b"pitches" in err()
    assert _raw_level(t, 2, N, H, W, Lq, buf.data_ptr(), sc.data_ptr(), logit_pitch=30) != 0 and b"pitches" in err()
    assert _raw_level(t, 2, N, H, W, Lq, None, sc.data_ptr()) != 0 and b"null pointer" in err()
    assert _raw_level(t, 2, N, H, W, Lq, buf.data_ptr(), None) != 0 and b"scratch" in err()
    # the global form: a null workspace, a null scratch word, a null grad_value
    v, sh, ls = case["value"].cuda(), case["shapes"].cuda(), case["lsi"].cuda()
    S = H * W
    ws = torch.zeros(N * S * 256, dtype=torch.int64, device="cuda")
    small = torch.full((N * Lq * (64 + 32 + 2),), 7.0, device="cuda")
    goff, glog, gref = small[:N * Lq * 64], small[N * Lq * 64:N * Lq * 96], small[N * Lq * 96:]

    def fused(grad_value, workspace, scratch):
        r = lib.dfx_msda_fused_backward_fixed_f32(
            v.data_ptr(), sh.data_ptr(), ls.data_ptr(), t["ref"].data_ptr(), 2, t["offsets"].data_ptr(), 64,
            t["logits"].data_ptr(), 32, t["grad_out"].data_ptr(), N, S, 8, 32, 1, Lq, 4, grad_value, workspace, scratch,
            goff.data_ptr(), 64, glog.data_ptr(), 32, gref.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return r

    assert fused(buf.data_ptr(), None, sc.data_ptr()) != 0 and b"workspace" in err()
    assert fused(buf.data_ptr(), ws.data_ptr(), None) != 0 and b"scratch" in err()
    assert fused(None, ws.data_ptr(), sc.data_ptr()) != 0 and b"grad_value" in err()
    assert fused(buf.data_ptr(), ws.data_ptr() + 8, sc.data_ptr()) != 0 and b"aligned" in err()
    # RoIAlign: a null workspace
    rois, go, (n, C, h, w) = _roi_case()
    tok, r = go.flatten(2).transpose(1, 2).contiguous().cuda(), rois.cuda()
    rc_ = lib.dfx_roi_align_backward_nhwc_fixed_f32(tok.data_ptr(), r.data_ptr(), n, C, h, w, r.shape[0], SIZE, SIZE, SCALE, 2, 1,
                                                    buf.data_ptr(), None, sc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc_ != 0 and b"workspace" in err()
    rc_ = lib.dfx_roi_align_backward_nhwc_fixed_f32(tok.data_ptr(), r.data_ptr(), n, C, h, w, r.shape[0], SIZE, SIZE, SCALE, 0, 1,
                                                    buf.data_ptr(), ws.data_ptr(), sc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc_ != 0 and b"sampling_ratio" in err()
    torch.cuda.synchronize()
    assert (buf == 7).all() and (small == 7).all() and (ws == 0).all() and (sc == 0x55555555).all()


# ---- 7. RoIAlign -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
def test_roi_exact_family_is_bit_equal_to_fp64(plain, dfx_env):
    if plain:
        dfx_env("DFX_ROI_BWD_PLAIN", 1)
    x, rois, go = rc.exact_family()
    ref = rc.reference_backward(x.shape, rois, go, rc.EXACT_SIZE, rc.EXACT_SCALE, rc.EXACT_SR, True)
    assert ref.abs().max() > 0
    assert torch.equal(_roi_fixed(go, rois, tuple(x.shape)).double(), ref)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("sr", [2, 3])
def test_roi_random_family_within_the_derived_bound(sr, aligned):
    """The float route's elementwise bound (tests/_roi_cases.py:random_bound): the fixed-point sum adds at most half a
    unit of 2^(e-F) <= 2^-37 gmax per term to terms the bound already charges 2^-24 each."""
    H, W, C = 13, 21, 256
    rois = rc.random_family(H, W, aligned, sr, seed=100 + sr)
    go = torch.randn(rois.shape[0], C, SIZE, SIZE, generator=torch.Generator().manual_seed(11))
    shape = (2, C, H, W)
    ref, bound = rc.random_bound(shape, rois, go, SIZE, SCALE, sr, aligned)
    err = (_roi_fixed(go, rois, shape, sr, aligned).double() - ref).abs()
    worst = (err / bound.clamp(min=1e-300))[bound > 0].max().item()
    print(f"fixed, sr={sr} aligned={aligned}: max err {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert (err <= bound).all(), f"err / bound up to {worst:.3f}"


def test_roi_no_rois_give_zeros_and_the_adaptive_ratio_raises():
    from dfx import ops
    go = torch.zeros(0, 49, 64, device="cuda")
    got = ops.roi_align_backward(go, torch.zeros(0, 5, device="cuda"), (2, 13, 21, 64), SIZE, SCALE, 2, True,
                                 channels_last=True, deterministic=True)
    assert got.shape == (2, 13, 21, 64) and got.abs().max() == 0
    rois, go, (N, C, H, W) = _roi_case()
    tok = go.flatten(2).transpose(1, 2).contiguous().cuda()
    with pytest.raises(RuntimeError, match="adaptive sampling_ratio"):
        ops.roi_align_backward(tok, rois.cuda(), (N, H, W, C), SIZE, SCALE, 0, True, channels_last=True, deterministic=True)


# ---- 8. routes -------------------------------------------------------------------------------------------------
def _fused_backward_names(monkeypatch, case, **kw):
    names = lt._spy_on_calls(monkeypatch)
    res = lt._fused_backward(case, **kw)
    return res, list(names)


def test_the_flag_selects_the_fixed_entries(flag, monkeypatch):
    from dfx import ops
    case = lc.make_level_case(5, 7, 4, 3, 37)
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", True)
    flag(True)
    assert ops.deterministic_mode()
    with monkeypatch.context() as mp:
        _, names = _fused_backward_names(mp, case, need_value=True, need_ref=True)
    assert names == [FUSED_FIXED]
    with monkeypatch.context() as mp:
        _, names = _fused_backward_names(mp, fc.make_case(2, 2, 3, 37), need_value=True)
    assert names == [FUSED_FIXED]
    with monkeypatch.context() as mp:
        res, names = _fused_backward_names(mp, case, need_value=False, need_ref=True)
    assert names == [FUSED_FLOAT] and res[0] is None
    with monkeypatch.context() as mp:
        mp.setattr(ops, "LEVEL_BWD_MIN_QUERIES", 0)
        on, names = _fused_backward_names(mp, case, need_value=True, need_ref=True)
        assert names == [FUSED_FLOAT, LEVEL_FIXED]
        assert torch.equal(on[0], lt._fused_backward(case, need_value=True)[0])
    # the library opted out: the float entries, whatever torch's flag says
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_DETERMINISTIC_ENV", "0")
        assert not ops.deterministic_mode()
        _, names = _fused_backward_names(mp, case, need_value=True)
        assert names == [FUSED_FLOAT]
        mp.setattr(ops, "LEVEL_BWD_MIN_QUERIES", 0)
        del names[:]
        _, names = _fused_backward_names(mp, case, need_value=True)
        assert names[-2:] == [FUSED_FLOAT, LEVEL_FLOAT]
    # without the flag, DFX_DETERMINISTIC=1 alone turns the mode on
    flag(False)
    assert not ops.deterministic_mode()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_DETERMINISTIC_ENV", "1")
        _, names = _fused_backward_names(mp, case, need_value=True)
        assert names == [FUSED_FIXED]


def test_the_flag_selects_the_fixed_roi_entry(flag, monkeypatch):
    from dfx import ops
    rois, go, (N, C, H, W) = _roi_case()
    tok = go.flatten(2).transpose(1, 2).contiguous().cuda()

    def backward_names():
        with monkeypatch.context() as mp:
            names = lt._spy_on_calls(mp)
            x = torch.zeros(N, H, W, C, device="cuda", requires_grad=True)
            ops.roi_align(x, rois.cuda(), SIZE, SCALE, 2, True, channels_last=True).backward(tok)
            torch.cuda.synchronize()
            return x.grad, [n for n in names if "backward" in n]

    flag(True)
    a, names = backward_names()
    assert names == [ROI_FIXED]
    b, _ = backward_names()
    assert torch.equal(a, b)
    monkeypatch.setattr(ops, "_DETERMINISTIC_ENV", "0")
    c, names = backward_names()
    assert names == [ROI_FLOAT] and fc.rel_err(c, a) < ATOMIC_TOL


@pytest.mark.parametrize("form", ["level", "global"])
def test_module_gradients_are_bit_identical_under_the_flag(form, flag, monkeypatch):
    """MSDeformAttn(256, 1, 8, 4).train() on a 5 x 7 level, N 2, Lq 37: two forward and backward passes under the flag give
    torch.equal gradients for every parameter, the query and the memory."""
    import models.ops.functions.ms_deform_attn_func as f
    from dfx import ops
    from models.ops.modules import MSDeformAttn
    torch.manual_seed(16)
    m = MSDeformAttn(256, 1, 8, 4).train().cuda()
    with torch.no_grad():     # the initialisation zeroes these; give the sampling something to differentiate
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    H, W, N, Lq = 5, 7, 2, 37
    shapes, lsi = fc.level_tensors([(H, W)])
    g = torch.Generator().manual_seed(160)
    ref = (0.1 + 0.8 * torch.rand(N, Lq, 1, 2, generator=g)).cuda()
    leaves = {"query": torch.randn(N, Lq, 256, generator=g), "memory": torch.randn(N, H * W, 256, generator=g)}
    gout = torch.randn(N, Lq, 256, generator=g).cuda()
    monkeypatch.setattr(f, "MSDeformAttnFunction", lt._Forbidden())
    monkeypatch.setattr(ops, "USE_LEVEL_BWD", True)
    if form == "level":
        monkeypatch.setattr(ops, "LEVEL_BWD_MIN_QUERIES", 0)
    names = lt._spy_on_calls(monkeypatch)
    flag(True)

    def once():
        t = {k: v.clone().cuda().requires_grad_() for k, v in leaves.items()}
        out = m(t["query"], ref, t["memory"], shapes.cuda(), lsi.cuda())
        named = dict(t, **dict(m.named_parameters()))
        grads = torch.autograd.grad((out * gout).sum(), list(named.values()))
        torch.cuda.synchronize()
        return dict(zip(named, grads))

    first, second = once(), once()
    want = [FUSED_FLOAT, LEVEL_FIXED] if form == "level" else [FUSED_FIXED]
    assert [n for n in names if n in (FUSED_FLOAT, FUSED_FIXED, LEVEL_FLOAT, LEVEL_FIXED)] == want * 2
    assert set(first) == {"query", "memory"} | set(dict(m.named_parameters()))
    for k in first:
        assert first[k].abs().max() > 0, k
        assert torch.equal(first[k], second[k]), f"d{k} differs between two passes"


# ---- 9. routes without a twin ----------------------------------------------------------------------------------
def _plain_operator_args():
    case = fc.make_case(2, 2, 3, 37)
    N, Lq, L = case["ref"].shape[:3]
    loc = fc.locations(case["ref"], case["offsets"].view(N, Lq, 8, L, 4, 2), case["sizes"]).contiguous()
    aw = torch.softmax(case["logits"].view(N, Lq, 8, L * 4), -1).view(N, Lq, 8, L, 4).contiguous()
    return [case["value"].cuda(), case["shapes"].cuda(), case["lsi"].cuda(), loc.cuda(), aw.cuda(), case["grad_out"].cuda()]


def test_routes_without_a_twin_raise_under_the_flag(flag):
    from dfx import ops
    args = _plain_operator_args()
    rois, go, shape = _roi_case()
    today = [t.clone() for t in ops.msda_backward(*args)], ops.roi_align_backward(go.cuda(), rois.cuda(), shape, SIZE, SCALE, 2)
    flag(True)
    with pytest.raises(RuntimeError, match="ms_deform_attn_backward does not have a deterministic implementation"):
        ops.msda_backward(*args)
    with pytest.raises(RuntimeError, match=r"roi_align_backward \(NCHW\) does not have a deterministic implementation"):
        ops.roi_align_backward(go.cuda(), rois.cuda(), shape, SIZE, SCALE, 2)
    flag(True, warn_only=True)
    with pytest.warns(UserWarning, match="ms_deform_attn_backward does not have a deterministic"):
        got = ops.msda_backward(*args)
    for a, b in zip(got, today[0]):
        assert a.shape == b.shape and fc.rel_err(a, b) < ATOMIC_TOL
    with pytest.warns(UserWarning, match="NCHW"):
        got = ops.roi_align_backward(go.cuda(), rois.cuda(), shape, SIZE, SCALE, 2)
    assert fc.rel_err(got, today[1]) < ATOMIC_TOL
    with warnings.catch_warnings():         # once per operation
        warnings.simplefilter("error")
        ops.msda_backward(*args)
    torch.cuda.synchronize()
