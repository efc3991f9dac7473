"""Shared builders of the inference kernel tests (csrc/fused_epilogue.hip, add_layernorm of csrc/layernorm_train.hip,
csrc/groupnorm.hip, the forward of csrc/dynconv.hip): seeded fp64 CPU inputs of fp32-representable values and a plain
restatement of each operator in the
dtype of its arguments.  The restatement is used twice: in fp64 it is the reference, in fp32 on the CPU it is the
yardstick - the GPU tests allow ``YARDSTICK_FACTOR`` x its error, error relative to the reference's largest magnitude,
the yardstick floored at one fp32 ulp (``yardstick``).

The seed rule.  A factor of 4 over one fp32 evaluation only means something when that evaluation is typical: every
yardstick case is built from the first seed (counting up from the case's base seed, at most ``MAX_SEEDS``) for which
two independent fp32 evaluations on the CPU - the restatement and torch's own functional - are within a factor 2 of
each other's error against fp64, per output (``roomy``).  tests/test_inference_kernels_cpu.py asserts that every case
finds such a seed.  DynamicConv reuses ``forward_stages`` (bmm + layer_norm + relu: torch's functional is the
restatement there) and ``make_case`` of tests/_dynconv_cases.py; its second evaluation is ``dynconv_plain``.
"""
import functools
import itertools

import torch
import torch.nn.functional as F

from tests import _dynconv_cases as dc

YARDSTICK_FACTOR = 4
ULP = 2.0 ** -23
MAX_SEEDS = 64
EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # what the C entries receive: the fp32 nearest to 1e-5


def rel_err(got, ref):
    """max |got - ref| relative to the reference's largest magnitude."""
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp(min=1e-300)).item()


def yardstick(cpu32, ref):
    """The CPU fp32 figure, at least one fp32 ulp (the CPU may happen to be exact; no other order has to be)."""
    return max(rel_err(cpu32, ref), ULP)


def cast(args, dtype):
    return tuple(a.to(dtype) if torch.is_tensor(a) and a.is_floating_point() else a for a in args)


def roomy(case):
    """Both fp32 evaluations within a factor 2 of each other's (floored) error, for every output."""
    for k, ref in case["ref"].items():
        a, b = yardstick(case["cpu32"][k], ref), yardstick(case["alt32"][k], ref)
        if max(a, b) > 2 * min(a, b):
            return False
    return True


def build_case(make_inputs, restate, functional, base_seed):
    """{args (fp64), ref, cpu32, alt32, seed}: the first seed from ``base_seed`` that is ``roomy``."""
    for seed in range(base_seed, base_seed + MAX_SEEDS):
        args = make_inputs(seed)
        a32 = cast(args, torch.float32)
        case = {"args": args, "seed": seed, "ref": restate(*args), "cpu32": restate(*a32), "alt32": functional(*a32)}
        if roomy(case):
            return case
    raise AssertionError(f"no seed in {base_seed}..{base_seed + MAX_SEEDS - 1} leaves room under the bound")


def compare(label, case, got, names=None):
    """The project's rule (tests/test_mha_backward_gpu.py::_compare): per output, error relative to the reference's
    largest magnitude, at most 4 x the (floored) CPU fp32 figure; prints ``cpu fp32 / gpu / max |ref|``."""
    worst = []
    for k in names or case["ref"]:
        ref = case["ref"][k]
        yard, err = yardstick(case["cpu32"][k], ref), rel_err(got[k].detach().cpu(), ref)
        print(f"  {label} {k}: cpu fp32 {yard:.3e}, gpu {err:.3e}, max |ref| {ref.abs().max().item():.3e}")
        if err > YARDSTICK_FACTOR * yard:
            worst.append(f"{label} {k}: {err:.3e} against {YARDSTICK_FACTOR} x cpu fp32 {yard:.3e}")
    assert not worst, "; ".join(worst)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- bias_act ----------------------------------------------------------------------------------------------------
# (shape, which operand starts 4 bytes into its buffer): vector path, scalar path, scalar by alignment of x / of the
# residual alone, chunks > 1 on both paths (few planes of >= 4096 elements), HW = 1
BIAS_ACT_CASES = [((2, 8, 8, 8), None), ((2, 5, 7, 9), None), ((2, 4, 4, 4), "x"), ((2, 4, 4, 4), "residual"),
                  ((1, 2, 64, 64), None), ((1, 3, 4099), None), ((2, 3, 1, 1), None)]


def bias_act(x, bias, residual, relu):
    """(x + b) + r, then max(., 0): the kernel's expression, no multiply in it."""
    v = x + bias.view(1, -1, *([1] * (x.dim() - 2)))
    if residual is not None:
        v = v + residual
    return torch.relu(v) if relu else v


def bias_act_inputs(shape):
    g = torch.Generator().manual_seed(sum(shape))
    return _randn(g, *shape), _randn(g, shape[1]), _randn(g, *shape)


# ---- bias_relu_maxpool -------------------------------------------------------------------------------------------
# the 16-byte fast path (xl + 8 < W) switches on and off inside a row at these widths; Wo = 1, 1, 4, 4, 5, 5, 8, 9
POOL_W, POOL_H = (1, 2, 7, 8, 9, 10, 16, 17), (1, 2, 3, 6)


def bias_relu_maxpool(x, bias):
    """relu(max over the 3x3 / stride 2 / pad 1 window + b): the window spelled out as nine shifted slices."""
    N, C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pad = torch.full((N, C, 2 * Ho + 1, 2 * Wo + 1), float("-inf"), dtype=x.dtype)
    pad[:, :, 1:H + 1, 1:W + 1] = x
    m = torch.full((N, C, Ho, Wo), float("-inf"), dtype=x.dtype)
    for dy, dx in itertools.product(range(3), range(3)):
        m = torch.maximum(m, pad[:, :, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])
    return torch.relu(m + bias.view(1, -1, 1, 1))


def pool_inputs(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    return _randn(g, 2, 3, H, W), _randn(g, 3)


# ---- add_layernorm -----------------------------------------------------------------------------------------------
LN_C = (4, 64, 256, 260, 512, 768, 1020, 1024)      # instantiations <1>, <2>, <4>; 768 = three chunks on <4>; partial last chunks
LN_ROWS = (1, 5, 8)                                   # four rows per workgroup: the last one is partial at 1 and 5
LN_FAMILIES = ("standard", "large_mean", "row_scales")


def add_layernorm(x, residual, gamma, beta, eps=EPS):
    s = x if residual is None else x + residual
    d = s - s.mean(-1, keepdim=True)
    return {"out": d * ((d * d).mean(-1, keepdim=True) + eps).rsqrt() * gamma + beta}


def add_layernorm_functional(x, residual, gamma, beta, eps=EPS):
    s = x if residual is None else x + residual
    return {"out": F.layer_norm(s, (s.shape[-1],), gamma, beta, eps)}


def add_layernorm_one_pass(x, residual, gamma, beta, eps=EPS):
    """What the kernel must not become: var = E[x^2] - mean^2."""
    s = x if residual is None else x + residual
    mean = s.mean(-1, keepdim=True)
    var = (s * s).mean(-1, keepdim=True) - mean * mean
    return {"out": (s - mean) * (var + eps).rsqrt() * gamma + beta}


def _ln_inputs(C, rows, residual, family, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "large_mean":
        x, r = _randn(g, rows, C) + 64, _randn(g, rows, C) * 0.25
    else:
        x, r = _randn(g, rows, C) * 3 + 1, _randn(g, rows, C)
    if family == "row_scales":           # LayerNorm is scale invariant up to eps: a row that reads another row's statistics shows
        scale = (2.0 ** (torch.arange(rows) - 4)).view(-1, 1)
        x, r = x * scale, r * scale
    return x.double(), (r.double() if residual else None), _randn(g, C).double(), _randn(g, C).double()


@functools.lru_cache(maxsize=None)
def ln_case(C, rows, residual, family):
    base = 1000 * C + 10 * rows + residual + 100000 * LN_FAMILIES.index(family)
    return build_case(lambda s: _ln_inputs(C, rows, residual, family, s), add_layernorm, add_layernorm_functional, base)


def ln_drop_partial(out, C, rows):
    """The result of a kernel that skips its partial pieces: the last chunk of < 256 channels, the rows of the last,
    partly filled workgroup of four.  None when the case has neither."""
    bad = out.clone()
    if C > 256 and C % 256:
        bad[:, C - C % 256:] = 0
    if rows % 4:
        bad[rows - rows % 4:] = 0
    return None if torch.equal(bad, out) else bad


# ---- box_refine --------------------------------------------------------------------------------------------------
BOX_ROWS, BOX_REF_DIMS = (1, 255, 256, 257), (2, 4)
BOX_REFS = (0.0, 1.0, 0.5, 1.2, -0.1, 1e-5, 1 - 1e-5)      # beyond [0, 1] and at the eps floors from both sides
BOX_DELTAS = (0.0, 20.0, -20.0, 100.0, -100.0)


def box_refine(delta, ref, eps=EPS):
    """sigmoid(delta + inverse_sigmoid(ref)) on the first ref.shape[-1] box columns, sigmoid(delta) on the rest."""
    v = delta.clone()
    x = ref.clamp(min=0, max=1)
    v[..., : ref.shape[-1]] += torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))
    return {"out": 1 / (1 + torch.exp(-v))}


def box_refine_functional(delta, ref, eps=EPS):
    from util.misc import inverse_sigmoid
    v = delta.clone()
    v[..., : ref.shape[-1]] += inverse_sigmoid(ref, eps)
    return {"out": v.sigmoid()}


def _box_inputs(lead, ref_dim, seed):
    """Random rows; from the front, as many as fit of the 35 rows (special reference x special delta) on every column."""
    g = torch.Generator().manual_seed(seed)
    rows = 1
    for n in lead:
        rows *= n
    delta, ref = _randn(g, rows, 4) * 2, torch.rand(rows, ref_dim, generator=g)
    grid = list(itertools.product(BOX_REFS, BOX_DELTAS))[: max(rows - 1, 0)]      # row 0 of a one-row case stays random
    for i, (r, d) in enumerate(grid):
        ref[i], delta[i] = r, d
    return delta.double().reshape(*lead, 4), ref.double().reshape(*lead, ref_dim)


@functools.lru_cache(maxsize=None)
def box_case(lead, ref_dim):
    return build_case(lambda s: _box_inputs(lead, ref_dim, s), box_refine, box_refine_functional, 10 * sum(lead) + ref_dim)


# ---- group_norm --------------------------------------------------------------------------------------------------
# (N, C, H, W, groups): count = 70 (scalar statistics path); cg = 3 and C no multiple of the 64-channel tile; HW = 1;
# one channel per group; one group; HW = 273 (partial pixel tiles)
GN_SHAPES = [(1, 64, 7, 5, 32), (2, 96, 4, 4, 32), (1, 8, 1, 1, 2), (1, 64, 5, 13, 64), (2, 64, 9, 9, 1), (3, 256, 13, 21, 32)]
GN_MISALIGNED = (2, 64, 6, 6, 32)        # count = 72, a multiple of 4: the scalar path by alignment alone
GN_FAMILIES = ("standard", "large_mean")
GN_OUTPUTS = ("y", "mean", "rstd")


def _gn_stats(x, groups, eps):
    xg = x.reshape(x.shape[0], groups, -1)
    mean = xg.mean(-1, keepdim=True)
    d = xg - mean
    return xg, mean, ((d * d).mean(-1, keepdim=True) + eps).rsqrt()


def group_norm(x, gamma, beta, groups, eps=EPS):
    """y = (x - mean) * rstd * gamma + beta and the statistics as the kernel stores them, per (image, group)."""
    N, C = x.shape[:2]
    xg, mean, rstd = _gn_stats(x, groups, eps)
    y = ((xg - mean) * rstd).reshape(N, C, -1) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    return {"y": y.reshape(x.shape), "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}


def group_norm_functional(x, gamma, beta, groups, eps=EPS):
    """y of F.group_norm; it returns no statistics, so those come from torch.var_mean over each (image, group) block."""
    var, mean = torch.var_mean(x.reshape(x.shape[0], groups, -1), -1, unbiased=False)
    return {"y": F.group_norm(x, groups, gamma, beta, eps), "mean": mean.reshape(-1), "rstd": (var + eps).rsqrt().reshape(-1)}


def group_norm_kernel_form(x, gamma, beta, groups, eps=EPS):
    """gn_apply's arithmetic: the mean folded into the bias, x * a + (beta - mean * a)."""
    N, C = x.shape[:2]
    _, mean, rstd = _gn_stats(x, groups, eps)
    cg = C // groups
    a = rstd.repeat_interleave(cg, 1) * gamma.view(1, -1, 1)
    b = beta.view(1, -1, 1) - mean.repeat_interleave(cg, 1) * a
    return {"y": (x.reshape(N, C, -1) * a + b).reshape(x.shape), "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}


def group_norm_one_pass(x, gamma, beta, groups, eps=EPS):
    N, C = x.shape[:2]
    xg = x.reshape(N, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    rstd = ((xg * xg).mean(-1, keepdim=True) - mean * mean + eps).rsqrt()
    y = ((xg - mean) * rstd).reshape(N, C, -1) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    return {"y": y.reshape(x.shape), "mean": mean.reshape(-1), "rstd": rstd.reshape(-1)}


def _gn_inputs(shape, family, seed):
    N, C, H, W, groups = shape
    g = torch.Generator().manual_seed(seed)
    x = _randn(g, N, C, H, W) + 16 if family == "large_mean" else _randn(g, N, C, H, W) * 3 + 1
    return x.double(), _randn(g, C).double(), _randn(g, C).double(), groups


@functools.lru_cache(maxsize=None)
def gn_case(shape, family):
    base = 1000 * sum(shape) + 100000 * GN_FAMILIES.index(family)
    return build_case(lambda s: _gn_inputs(shape, family, s), group_norm, group_norm_functional, base)


def gn_drop_partial(y, shape):
    """The result of a kernel that skips its partial 64 x 64 tiles (channels past the last full 64, pixels past the last
    full 64).  None when the shape has neither."""
    N, C, H, W, _ = shape
    bad = y.clone().reshape(N, C, H * W)
    bad[:, C - C % 64:] = 0
    bad[:, :, H * W - (H * W) % 64:] = 0
    bad = bad.reshape(y.shape)
    return None if torch.equal(bad, y) else bad


# ---- dynamic_conv forward ----------------------------------------------------------------------------------------
# (K, R, extra params columns, LayerNorm bias | None).  R: one row; 7; 33 = one row into the second 32-row MFMA tile; 49 / 50
# = the staging templates X_F4 / X_F4_MAX on either side of their switch; 64.  (5, 49, 64): params rows in a wider buffer.
DYN_SMALL = [(5, 1, 0, None), (5, 7, 0, None), (5, 33, 0, None), (5, 49, 0, None), (5, 50, 0, None), (5, 64, 0, None),
             (1, 49, 0, None), (1, 7, 0, None), (5, 49, 64, None)] + [(K, R, extra, 2.0) for K, R, extra in dc.PADDING_CASES]
# grid = min(K, 256) persistent workgroups: at 257 workgroup 0 alone runs a second RoI, at 515 three workgroups run a third.
# One case of 515 RoIs per R; the smaller counts are its leading RoIs (RoIs are independent: so is the reference).
DYN_LARGE_K, DYN_LARGE_R, DYN_K_PREFIXES = 515, (7, 49), (256, 257, 515)
DYN_ALONE = (0, 255, 256, 511, 514)


def dynconv_plain(feats, params, g1, b1, g2, b2):
    """The forward with both LayerNorms spelled out (the second fp32 evaluation beside ``forward_stages``)."""
    k1, k2 = dc.split_params(params, feats.shape[0])

    def ln(z, g, b):
        d = z - z.mean(-1, keepdim=True)
        return d * ((d * d).mean(-1, keepdim=True) + dc.EPS).rsqrt() * g + b

    y1 = torch.relu(ln(torch.matmul(feats, k1), g1, b1))
    return torch.relu(ln(torch.matmul(y1, k2), g2, b2))


@functools.lru_cache(maxsize=None)
def dyn_case(K, R, extra=0, bias=None):
    """``make_case`` of tests/_dynconv_cases.py under the seed rule; the case's own inputs plus ref / cpu32 / alt32 of ``out``."""
    base = 1000 * K + R
    for seed in range(base, base + MAX_SEEDS):
        try:
            src = dc.make_case(K, R, extra, bias, None if seed == base else seed)
        except AssertionError:          # make_case's own rule: too many rows near a ReLU kink for the backward tests
            continue
        a64 = tuple(src[k].double() for k in dc.OUTPUTS)
        a32 = tuple(src[k] for k in dc.OUTPUTS)
        case = {"src": src, "seed": seed, "ref": {"out": dc.forward_stages(*a64)[2]},
                "cpu32": {"out": dc.forward_stages(*a32)[2]}, "alt32": {"out": dynconv_plain(*a32)}}
        if roomy(case):
            return case
    raise AssertionError(f"dynamic_conv ({K},{R}): no seed leaves room under the bound")


def dyn_prefix(case, K):
    """The leading K RoIs of a case as a case of its own."""
    return {name: {"out": case[name]["out"][:K]} for name in ("ref", "cpu32", "alt32")}
