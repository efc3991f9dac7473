"""GPU: the host path behind the fused MSDA front end (dfx/ops.py, models/ops/modules/ms_deform_attn.py).  The joint and the
split form of the fused forward are one launch, the temporal decoder's flat read belongs to the forward alone, both forms
reject the same malformed operands before any launch, the level-in-LDS kernel on the reference layouts is an explicit call,
and MSDeformAttn takes one of its four routes per input - the dfx.ops entries each route calls, in order.

Shapes are the smallest that reach the edges: Lq = 5 (odd: a wave's second query slot is empty at the tail), levels of a
few pixels, N = 2.  Launch counts come from the library's own profile drain (dfx_profile_*)."""
import pytest
import torch

from tests import _msda_fused_cases as fc
from tests.test_msda_gpu import _level_case, _run_level_blocked, lsi_of

pytestmark = pytest.mark.gpu

M, D, P = 8, 32, 4
SIZES = {1: [(3, 4)], 3: [(3, 4), (2, 2), (1, 3)]}


@pytest.fixture(scope="module")
def ops():
    from dfx import _lib, ops
    _lib.load()  # fail loudly if the HIP library is missing
    return ops


def front_end_case(L, Lr, ref_dim, N=2, Lq=5, seed=0):
    """CPU tensors value [N,S,M,D], shapes, lsi, ref [N,Lq,Lr,ref_dim], qproj [N,Lq,3*M*L*P]."""
    g = torch.Generator().manual_seed(1000 * L + 10 * Lr + ref_dim + seed)
    shapes = torch.as_tensor(SIZES[L], dtype=torch.long)
    S = int(shapes.prod(1).sum())
    value = torch.randn(N, S, M, D, generator=g)
    qproj = torch.randn(N, Lq, 3 * M * L * P, generator=g) * 2.0
    ref = torch.rand(N, Lq, Lr, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] *= 0.3
    return value, shapes, lsi_of(shapes), ref, qproj


def launches(ops, fn):
    """(result or raised exception, number of fused MSDA launches `fn` made)."""
    torch.cuda.synchronize()
    ops.profile_start()
    try:
        got = fn()
    except RuntimeError as e:
        got = e
    finally:
        torch.cuda.synchronize()
        n = len(ops.profile_stop())
    return got, n


# ---- 1. joint form and split form are the same launch ------------------------------------------------------------
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("L", [1, 3])
def test_joint_and_split_form_are_the_same_launch(ops, L, ref_dim):
    value, shapes, lsi, ref, qproj = (t.cuda() for t in front_end_case(L, L, ref_dim))
    N, Lq, mlp = 2, 5, M * L * P
    with torch.no_grad():
        joint = ops.msda_fused_forward(value, shapes, lsi, ref, qproj, L, P)
        assert torch.isfinite(joint).all() and joint.abs().max() > 0
        # column slices of the joint row: read in place, rows one joint pitch apart
        off, logits = qproj[..., : 2 * mlp], qproj[..., 2 * mlp:]
        for t, width in ((off, 2 * mlp), (logits, mlp)):
            kept, pitch = ops._pitched_rows(t, N, Lq, width)
            assert kept is t and pitch == 3 * mlp
        assert torch.equal(joint, ops.msda_fused(value, shapes, lsi, ref, off, logits, L, P))
        # two tensors of their own
        off_c, logits_c = off.contiguous(), logits.contiguous()
        assert off_c.data_ptr() != off.data_ptr()
        assert torch.equal(joint, ops.msda_fused(value, shapes, lsi, ref, off_c, logits_c, L, P))
        # a slice that starts 4 bytes off a 16-byte boundary: _pitched_rows hands the kernel a copy
        wide = torch.zeros(N, Lq, 2 * mlp + 4, device="cuda")
        wide[..., 1:1 + 2 * mlp] = off
        skewed = wide[..., 1:1 + 2 * mlp]
        assert skewed.data_ptr() % 16 == 4
        copied, pitch = ops._pitched_rows(skewed, N, Lq, 2 * mlp)
        assert copied.data_ptr() != skewed.data_ptr() and pitch == 2 * mlp
        assert torch.equal(joint, ops.msda_fused(value, shapes, lsi, ref, skewed, logits, L, P))


# ---- 2. the temporal decoder's flat read ------------------------------------------------------------------------------
def test_flat_read_is_the_forwards_alone(ops, oracle):
    """L = 1 value level under Lr = 3 reference levels: msda_fused_forward reads the module's [Lq,M,Lr,P,2] locations flat
    per batch element (csrc/msda_fused.hip header) - the oracle at the tolerance of test_fused_front_end_temporal_quirk;
    msda_fused and msda_fused_backward want one reference level per value level and raise before any launch."""
    L, Lr, N, Lq = 1, 3, 2, 5
    value, shapes, lsi, ref, qproj = front_end_case(L, Lr, 4)
    off = qproj[..., : 2 * M * P].reshape(N, Lq, M, 1, P, 2)
    aw = torch.softmax(qproj[..., 2 * M * P:].reshape(N, Lq, M, P), -1).view(N, Lq, M, 1, P)
    loc = (ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5).contiguous()
    assert loc.shape == (N, Lq, M, Lr, P, 2)
    expect = torch.cat([oracle.msda_forward(value[b:b + 1], shapes, lsi, loc[b:b + 1].contiguous(), aw[b:b + 1].contiguous())
                        for b in range(N)], 0)
    v, s, l, r, q = (t.cuda() for t in (value, shapes, lsi, ref, qproj))
    got, n = launches(ops, lambda: ops.msda_fused_forward(v, s, l, r, q, L, P))
    assert n == 1
    assert torch.allclose(got.cpu(), expect, rtol=1e-4, atol=5e-5)
    o, lg = q[..., : 2 * M * P], q[..., 2 * M * P:]
    for call in (lambda: ops.msda_fused(v, s, l, r, o, lg, L, P),
                 lambda: ops.msda_fused(v, s, l, r, o.clone().requires_grad_(), lg, L, P),
                 lambda: ops.msda_fused_backward(torch.ones(N, Lq, M * D, device="cuda"), v, s, l, r, o, lg)):
        err, n = launches(ops, call)
        assert isinstance(err, RuntimeError) and "one reference level per value level" in str(err) and n == 0


# ---- 3. validation parity -----------------------------------------------------------------------------------------
def malformed(args):
    """name -> (value, shapes, lsi, ref, offsets, logits) with one operand broken; the split form rejects every one."""
    value, shapes, lsi, ref, offsets, logits = args
    return {
        "level_start_index length": (value, shapes, torch.cat([lsi, lsi[-1:]]), ref, offsets, logits),
        "fp64 value": (value.double(), shapes, lsi, ref, offsets, logits),
        "int32 spatial_shapes": (value, shapes.int(), lsi, ref, offsets, logits),
        "3-d reference_points": (value, shapes, lsi, ref[:, :, 0], offsets, logits),
    }


@pytest.mark.parametrize("what", ["level_start_index length", "fp64 value", "int32 spatial_shapes", "3-d reference_points"])
def test_joint_and_split_form_reject_the_same_operands(ops, what):
    L = 3
    value, shapes, lsi, ref, qproj = (t.cuda() for t in front_end_case(L, L, 2))
    mlp = M * L * P
    good = (value, shapes, lsi, ref, qproj[..., : 2 * mlp], qproj[..., 2 * mlp:])
    with torch.no_grad():
        out, n = launches(ops, lambda: ops.msda_fused(*good, L, P))
        assert isinstance(out, torch.Tensor) and n == 1
        v, s, l, r, o, lg = malformed(good)[what]
        for call in (lambda: ops.msda_fused(v, s, l, r, o, lg, L, P),
                     lambda: ops.msda_fused_forward(v, s, l, r, qproj, L, P),
                     lambda: ops.msda_fused_backward(torch.ones(2, 5, M * D, device="cuda"), v, s, l, r, o, lg)):
            err, n = launches(ops, call)
            assert isinstance(err, RuntimeError) and n == 0, (what, err)


# ---- 4. the level-in-LDS kernel on the reference layouts --------------------------------------------------------------
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_level_kernel_on_reference_layouts_is_the_block_major_launch(ops, ref_dim):
    H, W, N = 6, 7, 2
    value, qproj, ref = _level_case(900 + ref_dim, H, W, N, H * W, ref_dim, 2.0, ref_dim == 2)
    got = ops.msda_level_forward_reference(value.cuda(), ref.cuda(), qproj.cuda(), H, W)
    assert got.shape == (N, H * W, 256) and got.abs().max() > 0
    assert torch.equal(got, _run_level_blocked(value, qproj, ref, H, W))


def test_level_kernel_on_reference_layouts_refuses_what_does_not_fit(ops):
    from dfx import _lib
    fits = _lib.load().dfx_msda_fused_level_fits
    W = 84
    H = next(h for h in range(1, 4096) if not fits(h, W))          # the first height the library itself refuses
    assert H > 1 and fits(H - 1, W)
    q, r = torch.zeros(1, 3, 96, device="cuda"), torch.zeros(1, 3, 1, 2, device="cuda")
    ok, n = launches(ops, lambda: ops.msda_level_forward_reference(torch.zeros(1, (H - 1) * W, 8, 32, device="cuda"), r, q, H - 1, W))
    assert isinstance(ok, torch.Tensor) and n == 1
    err, n = launches(ops, lambda: ops.msda_level_forward_reference(torch.zeros(1, H * W, 8, 32, device="cuda"), r, q, H, W))
    assert isinstance(err, RuntimeError) and "does not fit" in str(err) and n == 0


# ---- 5. the module's route table -----------------------------------------------------------------------------------------
SPIED = ("linear", "add_layernorm", "msda_level_forward", "msda_fused_forward", "msda_fused", "msda_fused_backward")

# case -> the dfx.ops entries (and the operator's two) MSDeformAttn(256, L, 8, 4) calls, in order, forward then backward;
# recorded on the commit before MSDeformAttn.forward selected its route in one place.  linear[...] names the keywords that
# carry an operand layout or a fused neighbour.
_LEVEL = ["linear[row_mask,col_block=4]", "linear[col_block=12]", "msda_level_forward"]
_NORM = ["linear[]", "add_layernorm"]                       # what linear(norm=...) itself goes on to call
ROUTES = {
    "level": _LEVEL + ["linear[x_blocked]"],
    "level, pair, value=, post=": ["linear[row_mask,col_block=4]", "linear[add,col_block=12]", "msda_level_forward",
                                   "linear[x_blocked,residual,norm]", "linear[x_blocked]", "add_layernorm"],
    "fused": ["linear[row_mask]", "linear[]", "msda_fused_forward", "linear[]"],
    "fused, pair, value=": ["linear[add]", "msda_fused_forward", "linear[]"],
    "fused, post=": ["linear[row_mask]", "linear[]", "msda_fused_forward", "linear[residual,norm]"] + _NORM,
    "fused, value=, post=": ["linear[]", "msda_fused_forward", "linear[residual,norm]"] + _NORM,
    "train": ["msda_fused", "msda_fused_backward"],
    "train, post=": ["msda_fused", "msda_fused_backward"],
    "operator: fp64": ["operator forward", "operator backward"],
    "operator: autocast": ["operator forward", "operator backward"],
    "operator: MSDA_TRAIN off": ["operator forward", "operator backward"],
    "flat read in grad mode": ["operator forward"] * 2 + ["operator backward"] * 2,
}


def route_calls(case, monkeypatch):
    """Run one input of the table through the module -> the recorded entry names."""
    import copy

    import MultiScaleDeformableAttention as MSDA
    from dfx import ops
    from models.ops.modules import MSDeformAttn
    from models.ops.modules import ms_deform_attn as mod_file
    from models.transformer_layers import make_level_tensors
    calls = []

    def spy(owner, name, label):
        real = getattr(owner, name)

        def wrapper(*a, **k):
            tag = label
            if name == "linear":
                keys = [f"{n}={k[n]}" if n == "col_block" else n for n in ("add", "row_mask", "col_block", "x_blocked", "residual", "norm")
                        if k.get(n) is not None and not (isinstance(k[n], (bool, int)) and not k[n])]
                tag = f"linear[{','.join(keys)}]"
            calls.append(tag)
            return real(*a, **k)

        monkeypatch.setattr(owner, name, wrapper)

    for name in SPIED:
        spy(ops, name, name)
    spy(MSDA, "ms_deform_attn_forward", "operator forward")
    spy(MSDA, "ms_deform_attn_backward", "operator backward")

    L = 1 if case.startswith(("level", "flat")) else 2
    sizes = [(5, 6)] if L == 1 else [(3, 4), (2, 2)]
    Lr = 3 if case.startswith("flat") else L
    N, Lq, S = 2, 30, sum(h * w for h, w in sizes)
    torch.manual_seed(3)
    m = MSDeformAttn(256, L, 8, 4).cuda().eval()
    if case.startswith("level"):
        shapes, lsi = make_level_tensors(sizes, torch.device("cuda"))       # the host sizes ride on the shapes tensor
        monkeypatch.setattr(ops, "LEVEL_MIN_QUERIES", 0)
    else:
        shapes, lsi = (t.cuda() for t in fc.level_tensors(sizes))
    g = torch.Generator().manual_seed(4)
    query, pos = torch.randn(N, Lq, 256, generator=g).cuda(), torch.randn(N, Lq, 256, generator=g).cuda()
    src = torch.randn(N, S, 256, generator=g).cuda()
    ref = torch.rand(N, Lq, Lr, 2, generator=g).cuda()
    mask = torch.zeros(N, S, dtype=torch.bool, device="cuda")
    mask[:, -1] = True
    kw = {}
    if "value=" in case:
        kw["value"] = torch.randn(N, S, 256, generator=g).cuda()
    if "post=" in case:
        kw["post"] = (torch.randn(N, Lq, 256, generator=g).cuda(), torch.nn.LayerNorm(256).cuda())
    if case.startswith(("level", "fused")):
        with torch.no_grad():
            out = m((query, pos) if "pair" in case else query, ref, src, shapes, lsi, mask, **kw)
        assert out.shape == (N, Lq, 256) and out.grad_fn is None
        return calls
    if case == "operator: MSDA_TRAIN off":
        monkeypatch.setattr(mod_file, "MSDA_TRAIN", False)
    query.requires_grad_()
    if case == "operator: fp64":
        m, query, src, ref = copy.deepcopy(m).double(), query.detach().double().requires_grad_(), src.double(), ref.double()
    if case == "operator: autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(query, ref, src, shapes, lsi, mask, **kw)
    else:
        out = m(query, ref, src, shapes, lsi, mask, **kw)
    out.float().sum().backward()
    assert query.grad is not None
    return calls


@pytest.mark.parametrize("case", [
    "level", "level, pair, value=, post=", "fused", "fused, pair, value=", "fused, post=", "fused, value=, post=",
    "train", "train, post=", "operator: fp64", "operator: autocast", "operator: MSDA_TRAIN off", "flat read in grad mode",
])
def test_module_route_table(case, monkeypatch):
    calls = route_calls(case, monkeypatch)
    print(f'    "{case}": {calls},')
    assert calls == ROUTES[case]
