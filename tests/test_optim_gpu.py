"""GPU: dfx.optim.AdamW / grad_norm (csrc/optim.hip) on a hand-made parameter list - every size at which the kernels take
another path (one thread, the vector body, the scalar tail, a short / a full / several chunks, no chunk, a misaligned view).

The yardstick is never the kernel: truth is torch.optim.AdamW (and clip_grad_norm_) on fp64 copies of the same tensors, and
the bound is what the fp32 torch.optim.AdamW route itself misses that truth by on these inputs, times 2 - the kernel rounds
in fp32 like that route but contracts other products into FMAs, so its error is of the same size, not the same bits.

Measured on an MI355X (profiles/r20_optim_step.txt; each test prints its pair): largest error after the three steps relative
to each tensor's largest magnitude, torch fp32 route / this kernel:
    plain     p 1.38e-07 / 1.30e-07   exp_avg 5.59e-07 / 5.59e-07   exp_avg_sq 1.87e-07 / 1.45e-07
    clipped   p 1.39e-07 / 1.07e-07   exp_avg 3.24e-07 / 1.30e-07   exp_avg_sq 2.49e-07 / 1.41e-07
    cosine    p 1.22e-07 / 1.07e-07   exp_avg 5.59e-07 / 5.59e-07   exp_avg_sq 1.87e-07 / 1.45e-07
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("p", "exp_avg", "exp_avg_sq")
STEPS = 3
MISALIGNED = 67          # elements of the parameter that starts one float into its storage


@functools.lru_cache(maxsize=None)
def numels():
    from dfx import optim
    chunk = optim.chunk_elements()
    return (1, 3, 4, 5, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 7, 0, MISALIGNED)


def scales():
    n = len(numels())
    return [10.0 ** (-6 + 9 * i / (n - 1)) for i in range(n)]          # 1e-6 .. 1e3 across the tensors


@functools.lru_cache(maxsize=None)
def initial_values():
    g = torch.Generator().manual_seed(0)
    return tuple(torch.randn(n, generator=g) for n in numels())


@functools.lru_cache(maxsize=None)
def gradient_values(step):
    g = torch.Generator().manual_seed(100 + step)
    return tuple(torch.randn(n, generator=g) * s for n, s in zip(numels(), scales()))


def make_params(dtype=torch.float32):
    """fresh leaves on the GPU holding initial_values(); the last one is a contiguous view one element into its storage"""
    out = []
    for v in initial_values()[:-1]:
        out.append(v.to("cuda", dtype).requires_grad_())
    base = torch.zeros(MISALIGNED + 1, dtype=dtype, device="cuda")
    view = base[1:]
    view.copy_(initial_values()[-1])
    assert view.is_contiguous() and view.data_ptr() % 16 == view.element_size()
    out.append(view.requires_grad_())
    return out


def set_grads(params, step):
    for p, g in zip(params, gradient_values(step)):
        p.grad = g.to(p.device, p.dtype)


def groups_of(params):
    """two groups with their own lr and weight decay, one without decay; the sizes are spread over both"""
    return [{"params": params[0::2], "lr": 1e-3, "weight_decay": 0.1}, {"params": params[1::2], "lr": 3e-2, "weight_decay": 0.0}]


def make_optimizer(route, params):
    if route == "ours":
        from dfx.optim import AdamW
        return AdamW(groups_of(params), lr=1e-3, weight_decay=1e-2)
    return torch.optim.AdamW(groups_of(params), lr=1e-3, weight_decay=1e-2)


def one_step(route, opt, params, max_norm):
    """clip_grad_norm_ + step on the torch routes, step(max_norm) on ours; -> the total norm or None"""
    if route == "ours":
        return opt.step(max_norm=max_norm)
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else None
    opt.step()
    return norm


def snapshot(opt, params):
    return {"p": [p.detach().clone() for p in params],
            "exp_avg": [opt.state[p]["exp_avg"].clone() for p in params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() for p in params]}


@functools.lru_cache(maxsize=None)
def run(route, scenario):
    """route "truth" (fp64 torch) | "torch" (fp32 torch) | "ours";  scenario "plain" | "clip" | "cosine" -> snapshot after STEPS"""
    params = make_params(torch.float64 if route == "truth" else torch.float32)
    opt = make_optimizer("ours" if route == "ours" else "torch", params)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=STEPS, eta_min=1e-5) if scenario == "cosine" else None
    for step in range(STEPS):
        set_grads(params, step)
        one_step(route, opt, params, CLIP if scenario == "clip" else 0.0)
        if sched is not None:
            sched.step()
    return snapshot(opt, params)


def total_norm64(step):
    return torch.linalg.vector_norm(torch.cat([g.double() for g in gradient_values(step)]).cuda()).item()


CLIP = 50.0          # below the norm of every step's gradients (asserted in test_clipping_below_the_norm)


def errors(got, truth):
    """per kind: the largest |got - truth| relative to the tensor's largest |truth|, over all tensors"""
    out = {}
    for k in KINDS:
        worst = 0.0
        for a, b in zip(got[k], truth[k]):
            if b.numel():
                worst = max(worst, ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)).item())
        out[k] = worst
    return out


def assert_within_torch_error(got, scenario, what):
    truth = run("truth", scenario)
    torch_err, our_err = errors(run("torch", scenario), truth), errors(got, truth)
    print(f"{what}: error against fp64 truth, torch fp32 route {torch_err}  this route {our_err}")
    for k in KINDS:
        assert torch_err[k] > 0, "the fp32 torch route equals fp64 truth: the inputs check nothing"
        assert our_err[k] <= 2 * torch_err[k], (what, k, our_err[k], torch_err[k])


# ---- norm ------------------------------------------------------------------------------------------------------------
def test_grad_norm_is_the_fp64_norm_rounded_once_and_repeats_bitwise():
    from dfx.optim import grad_norm
    params = make_params()
    set_grads(params, 0)
    a, b = grad_norm(params), grad_norm(params)
    assert a.shape == () and a.dtype == torch.float32 and a.is_cuda
    want = total_norm64(0)
    assert abs(a.item() - want) / want <= 2.0 ** -23
    assert torch.equal(a, b)
    params[2].grad = None                                      # skipped, like clip_grad_norm_ skips it
    rest = torch.linalg.vector_norm(torch.cat([g.double() for i, g in enumerate(gradient_values(0)) if i != 2])).item()
    assert abs(grad_norm(params).item() - rest) / rest <= 2.0 ** -23


# ---- the update ------------------------------------------------------------------------------------------------------
def test_three_steps_against_fp64_truth():
    assert_within_torch_error(run("ours", "plain"), "plain", "three steps, two groups")


def test_clipping_below_the_norm():
    assert all(total_norm64(s) > 2 * CLIP for s in range(STEPS))
    assert_within_torch_error(run("ours", "clip"), "clip", f"three steps clipped to {CLIP}")


def test_clipping_above_the_norm_changes_no_bit_and_leaves_grad_alone():
    plain, loose = make_params(), make_params()
    opt_a, opt_b = make_optimizer("ours", plain), make_optimizer("ours", loose)
    set_grads(plain, 0), set_grads(loose, 0)
    before = [p.grad.clone() for p in loose]
    assert opt_a.step() is None
    norm = opt_b.step(max_norm=4.0 * total_norm64(0))                          # coefficient exactly 1
    assert norm.shape == () and norm.dtype == torch.float32
    assert abs(norm.item() - total_norm64(0)) / total_norm64(0) <= 2.0 ** -23
    a, b = snapshot(opt_a, plain), snapshot(opt_b, loose)
    for k in KINDS:
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    for p, g in zip(loose, before):
        assert torch.equal(p.grad, g)
    tight = make_params()
    opt_c = make_optimizer("ours", tight)
    set_grads(tight, 0)
    norm_c = opt_c.step(max_norm=CLIP)                                          # clipped: the norm is the same, .grad still unscaled
    assert torch.equal(norm_c, norm)
    for p, g in zip(tight, before):
        assert torch.equal(p.grad, g)
    assert any(not torch.equal(x, y) for x, y in zip(snapshot(opt_c, tight)["exp_avg"], a["exp_avg"]))


def test_parameters_without_a_gradient_are_skipped():
    params = make_params()
    frozen = torch.randn(70, device="cuda")                    # requires_grad=False
    params.append(frozen)
    opt = make_optimizer("ours", params)
    set_grads(params[:-1], 0)
    params[4].grad = None
    untouched = (params[4], frozen)
    kept = [(t.detach().clone(), t._version) for t in untouched]
    versions = [p._version for p in params]
    opt.step(max_norm=CLIP)
    torch.cuda.synchronize()
    for t, (value, version) in zip(untouched, kept):
        assert torch.equal(t.detach(), value) and t._version == version and len(opt.state[t]) == 0
    empty = params[numels().index(0)]
    assert empty.numel() == 0 and opt.state[empty]["step"].item() == 1           # harmless: no chunk, nothing to write
    for i, p in enumerate(params):
        if all(p is not t for t in untouched):
            assert p._version > versions[i] and opt.state[p]["step"].item() == 1
    set_grads(params[:-1], 1)                                  # the skipped parameter joins later with its own step count
    opt.step()
    assert opt.state[params[4]]["step"].item() == 1 and opt.state[params[5]]["step"].item() == 2


def test_non_finite_gradients_follow_torch():
    results = {}
    for route in ("torch", "ours"):
        params = make_params()
        opt = make_optimizer(route, params)
        set_grads(params, 0)
        big = numels().index(max(numels()))
        params[big].grad[5] = float("inf")
        norm = one_step(route, opt, params, 1.0)
        assert torch.isinf(norm)
        results[route] = snapshot(opt, params)
    for k in KINDS:
        for a, b in zip(results["ours"][k], results["torch"][k]):
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isfinite(a), torch.isfinite(b)), k
    assert sum(int(torch.isnan(t).sum()) for t in results["ours"]["p"]) == 1


# ---- state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,then", [("ours", "torch"), ("torch", "ours")])
def test_state_dict_moves_between_the_classes(first, then):
    """two steps on one class, its state_dict loaded into the other over cloned parameters, one more step on both"""
    params = make_params()
    opt = make_optimizer(first, params)
    for step in range(STEPS - 1):
        set_grads(params, step)
        one_step(first, opt, params, 0.0)
    clones = [p.detach().clone().requires_grad_() for p in params]
    other = make_optimizer(then, clones)
    assert set(other.param_groups[0]) == set(opt.param_groups[0])            # the same hyper-parameter keys, before any loading
    other.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert all(other.state[c]["step"].item() == STEPS - 1 and not other.state[c]["step"].is_cuda for c in clones)
    for route, o, ps in ((first, opt, params), (then, other, clones)):
        set_grads(ps, STEPS - 1)
        one_step(route, o, ps, 0.0)
        assert_within_torch_error(snapshot(o, ps), "plain", f"{STEPS - 1} steps on {first}, the last on {route}")


def test_cosine_annealing_drives_the_learning_rate():
    assert_within_torch_error(run("ours", "cosine"), "cosine", "three epochs of one step under CosineAnnealingLR")
    assert any(not torch.equal(a, b) for a, b in zip(run("ours", "cosine")["p"], run("ours", "plain")["p"]))


# ---- versions and the cached fused routes ------------------------------------------------------------------------------
def _step_on(module, lr=0.05):
    from dfx.optim import AdamW
    from models.fused import derived_key
    params = [p for p in module.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(17)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    owners = [m for m in module.modules() if any(True for _ in m.parameters(recurse=False))]
    keys, versions = [derived_key(m) for m in owners], [p._version for p in params]
    AdamW(params, lr=lr).step(max_norm=1.0)
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(derived_key(m) != k for m, k in zip(owners, keys))
    for p in params:
        p.grad = None


def _follows(build, run_module):
    from tests import _lifecycle as L
    from util import memo
    memo.clear()
    a = build()
    y0 = L.run_twice(run_module, a)                            # the second run meets every cache
    _step_on(a)
    with torch.no_grad():
        y1 = [t.clone() for t in L.tensors_of(run_module(a))]
    L.assert_same(y1, L.fresh_reference(build, run_module, a), "after AdamW.step: the module that had run against a fresh one")
    assert L.differs(y1, y0)


def test_fused_linear_shows_the_stepped_weights():
    from models.fused import Linear
    from tests._param_fill import fill_params_by_name
    x = torch.randn(50, 64, generator=torch.Generator().manual_seed(1)).cuda()
    _follows(lambda: fill_params_by_name(Linear(64, 32), seed=3).cuda().eval(), lambda m: m(x))


def test_folded_bottleneck_shows_the_stepped_weights():
    from torch import nn
    from models.backbone_scratch import FrozenBatchNorm2d
    from models.resnet import Bottleneck
    from tests._param_fill import fill_params_by_name
    x = torch.randn(2, 64, 8, 12, generator=torch.Generator().manual_seed(1)).cuda()

    def build():
        ds = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False), FrozenBatchNorm2d(256))
        return fill_params_by_name(Bottleneck(64, 64, 1, 1, ds, FrozenBatchNorm2d), seed=3).cuda().eval()

    def run_block(m):
        y = m.forward_fused(x)
        assert "_folded" in m.__dict__                       # the route that keeps folded filters
        return y

    _follows(build, run_block)


# ---- routing -----------------------------------------------------------------------------------------------------------
def test_build_optimizer_takes_the_fused_class_for_fp32_parameters_on_the_gpu(monkeypatch):
    from types import SimpleNamespace
    import dfx.optim
    from models.optim import build_optimizer
    args = SimpleNamespace(lr=1e-4, lr_linear_proj_names=["sampling_offsets"], lr_linear_proj_mult=0.1, lr_backbone_names=["backbone.0"],
                           weight_decay=2e-5, depth_type="Baseline_rgb", sgd=False)
    model = torch.nn.ModuleDict({"sampling_offsets": torch.nn.Linear(8, 4), "head": torch.nn.Linear(4, 2)}).cuda()
    monkeypatch.delenv("DFX_OPTIM", raising=False)
    opt = build_optimizer(args, model, "main_multi.py")
    assert type(opt) is dfx.optim.AdamW
    assert [(len(g["params"]), g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(2, 1e-4, 2e-5), (2, 1e-4 * 0.1, 2e-5)]
    monkeypatch.setenv("DFX_OPTIM", "0")
    assert type(build_optimizer(args, model, "main_multi.py")) is torch.optim.AdamW
    monkeypatch.delenv("DFX_OPTIM")
    assert type(build_optimizer(args, model.half(), "main_multi.py")) is torch.optim.AdamW          # not fp32: torch's class
    args.sgd = True
    assert type(build_optimizer(args, model, "main_multi.py")) is torch.optim.SGD


# ---- rejections --------------------------------------------------------------------------------------------------------
def test_construction_refuses_what_the_kernels_cannot_take():
    from dfx.optim import AdamW
    ok = torch.zeros(8, device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="parameter 1 .*CPU"):
        AdamW([ok, torch.zeros(8, requires_grad=True)])
    with pytest.raises(ValueError, match="parameter 1 .*float16"):
        AdamW([ok, torch.zeros(8, device="cuda", dtype=torch.float16, requires_grad=True)])
    with pytest.raises(ValueError, match="parameter 2 .*contiguous"):
        AdamW([{"params": [ok, torch.zeros(8, device="cuda", requires_grad=True)]},
               {"params": [torch.zeros(4, 6, device="cuda").t().requires_grad_()]}])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            AdamW([ok], **{flag: True})
    opt = AdamW([ok])
    ok.grad = torch.zeros(8, 2, device="cuda")[:, 0]            # 8 elements, stride 2
    with pytest.raises(RuntimeError, match="not contiguous"):
        opt.step()
    ok.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (8,)).cuda()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
