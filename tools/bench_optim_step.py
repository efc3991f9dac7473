"""Time the tail of a training iteration - clip_grad_norm_ + AdamW.step over all trainable parameters of a detector - on the
torch routes and on dfx.optim.AdamW (csrc/optim.hip), and the two kernels' achieved bandwidth.

    python tools/bench_optim_step.py                       # both parameter sets, every route, host / device / wall time
    python tools/bench_optim_step.py --kernels             # the two kernels alone, back to back: bytes per second
    python tools/bench_optim_step.py --train-step          # one whole training step of the single-frame Late Fusion recipe at
                                                           # 2 x 800 x 1333 (bench_criterion.py --train-step) + the optimizer step
                                                           # (DFX_LINEAR_BF16_TRAIN=1 [--linear-bf16-min-elements 0]: DESIGN.md 4l)

Parameter sets: the trainable parameters of the single-frame Late Fusion recipe (LateFusion.sh: the RGB body frozen by the
reference's group rules) and of TransVOD++ with depth (TransVOD++_withdepth.sh), grouped by models.optim.build_param_groups
with the scripts' own lr / weight decay / max_norm, gradients seeded randn * 1e-3.
Routes, alternating in one process on the same parameters (each with its own optimizer state):
    foreach      clip_grad_norm_ + torch.optim.AdamW (its default on the GPU: _foreach_* calls)
    torch_fused  the same with fused=True, if this torch build constructs and runs it
    dfx          dfx.optim.AdamW.step(max_norm)
Per route the median over --repeats of the host clock around a step that ends in a synchronise (``wall``), of the host clock
until the step returns (``host``) and of device events around it (``device``), with min / max of the wall time.
A GPU is required: there is no CPU timing.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8e12          # the MI355X figure the README uses
# what every shipped training script passes (configs/training/*.sh through the reference's parsers: tests/golden/args.json)
TRAIN = dict(lr_linear_proj_names=["reference_points", "sampling_offsets"], lr_linear_proj_mult=0.1,
             lr_backbone_names=["backbone.0"], weight_decay=2e-5, sgd=False)
SETS = {"single_latefusion": ("main.py", dict(lr=1e-5), 0.5), "transvodpp_depth": ("main_multi.py", dict(lr=1e-4), 1.0)}


def parameter_set(name, model=None):
    """-> (args, model, script, groups, max_norm) with the model on the GPU"""
    from models import build_model
    from models.config import single_args, transvodpp_args
    from models.optim import build_param_groups
    script, extra, max_norm = SETS[name]
    make = single_args if name == "single_latefusion" else transvodpp_args
    args = make("LateFusion", device="cuda", **TRAIN, **extra)
    if model is None:
        torch.manual_seed(0)
        model = build_model(args)[0].cuda().train()
    return args, model, script, build_param_groups(args, model, script), max_norm


def seed_grads(params, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3


def make_routes(groups, args, max_norm):
    """-> {name: step function}; a route that cannot be built is reported and left out"""
    from dfx.optim import AdamW
    params = [p for g in groups for p in g["params"]]
    kw = dict(lr=args.lr, weight_decay=args.weight_decay)
    routes = {}

    def torch_route(opt):
        def step():
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
        return step

    routes["foreach"] = torch_route(torch.optim.AdamW(groups, **kw))
    try:
        fused = torch_route(torch.optim.AdamW(groups, fused=True, **kw))
        fused()
        torch.cuda.synchronize()
        routes["torch_fused"] = fused
    except Exception as e:          # noqa: BLE001 - whatever this build raises is the finding
        print(f"  torch.optim.AdamW(fused=True) does not run on this build: {type(e).__name__}: {e}")
    ours = AdamW(groups, **kw)
    routes["dfx"] = lambda: ours.step(max_norm=max_norm)
    return routes


def time_routes(name, repeats, warmup):
    args, model, script, groups, max_norm = parameter_set(name)
    params = [p for g in groups for p in g["params"]]
    n = sum(p.numel() for p in params)
    print(f"{name}: {len(params)} trainable tensors, {n} elements ({n * 28 / 1e9:.3f} GB per update pass), {len(groups)} groups, max_norm {max_norm}")
    seed_grads(params)
    routes = make_routes(groups, args, max_norm)
    times = {r: {"wall": [], "host": [], "device": []} for r in routes}
    for i in range(warmup + repeats):
        for r, step in routes.items():            # alternating: every route sees the same machine
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            step()
            stop.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= warmup:
                times[r]["wall"].append(t2 - t0)
                times[r]["host"].append(t1 - t0)
                times[r]["device"].append(start.elapsed_time(stop) * 1e-3)
    med = {r: {k: statistics.median(v) for k, v in t.items()} for r, t in times.items()}
    for r in routes:
        w = times[r]["wall"]
        print(f"  {r:11s}  wall {med[r]['wall'] * 1e3:7.3f} ms (min {min(w) * 1e3:.3f}, max {max(w) * 1e3:.3f})   host {med[r]['host'] * 1e3:7.3f} ms   "
              f"device events {med[r]['device'] * 1e3:7.3f} ms   [{repeats} repeats after {warmup}]")
    best_torch = min((r for r in routes if not r.startswith("dfx")), key=lambda r: med[r]["wall"])
    print(f"  {best_torch} / dfx wall: {med[best_torch]['wall'] / med['dfx']['wall']:.2f}x")


def time_kernels(name, launches, repeats):
    """the two kernels alone: ``launches`` launches back to back between two device events, median over ``repeats``"""
    from dfx.optim import AdamW, chunk_elements
    from dfx.ops import _call
    args, model, script, groups, max_norm = parameter_set(name)
    params = [p for g in groups for p in g["params"]]
    n = sum(p.numel() for p in params)
    seed_grads(params)
    opt = AdamW(groups, lr=args.lr, weight_decay=args.weight_decay)
    params, rec, chunks = opt._host_tables()
    dev = params[0].device
    tables, off = opt._staging.upload(dev, rec, chunks)
    tp, cp, nc = tables.data_ptr(), tables.data_ptr() + off, len(chunks)
    partials = torch.empty(nc, dtype=torch.float64, device=dev)
    norm = torch.empty((), dtype=torch.float32, device=dev)
    kernels = {
        "grad_sqnorm (4 B/element)": (4, lambda: _call("bench", "dfx_grad_sqnorm_f32", dev, tp, cp, nc, partials.data_ptr())),
        "adamw_step (28 B/element)": (28, lambda: _call("bench", "dfx_adamw_step_f32", dev, tp, cp, nc, None, 0.0, None)),
        "adamw_step with clipping (28 B/element)": (28, lambda: _call("bench", "dfx_adamw_step_f32", dev, tp, cp, nc, partials.data_ptr(),
                                                                      float(max_norm), norm.data_ptr())),
    }
    print(f"{name}: {n} elements in {len(params)} tensors, {nc} chunks of {chunk_elements()}; {launches} launches back to back, median of {repeats}")
    for what, (bytes_per, launch) in kernels.items():
        per = []
        for i in range(repeats + 2):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                launch()
            stop.record()
            torch.cuda.synchronize()
            if i >= 2:
                per.append(start.elapsed_time(stop) * 1e-3 / launches)
        t = statistics.median(per)
        rate = n * bytes_per / t
        print(f"  {what:42s} {t * 1e6:8.1f} us (min {min(per) * 1e6:.1f}, max {max(per) * 1e6:.1f})   "
              f"{rate / 1e12:.2f} TB/s = {rate / HBM_BYTES_PER_S:.2f} of 8 TB/s")


def train_step(repeats, warmup, bf16_min_elements=None):
    """bench_criterion.py --train-step with the optimizer step appended: forward, criterion, backward, clip + AdamW.
    bf16_min_elements: replaces models.fused.LINEAR_BF16_TRAIN_MIN_ELEMENTS (0: every eligible Linear takes the bf16 train route
    when DFX_LINEAR_BF16_TRAIN=1, whatever its size - the step at 2 frames lies below the rule)."""
    import bench_criterion as bc
    if bf16_min_elements is not None:
        from models import fused
        fused.LINEAR_BF16_TRAIN_MIN_ELEMENTS = bf16_min_elements
        print(f"models.fused.LINEAR_BF16_TRAIN_MIN_ELEMENTS = {bf16_min_elements}")
    from dfx.optim import AdamW
    from models import build_model
    from util.misc import NestedTensor
    name = "single_latefusion"
    script, extra, max_norm = SETS[name]
    from models.config import single_args
    args = single_args("LateFusion", device="cuda", **TRAIN, **extra)
    torch.manual_seed(0)
    model, crit, _ = build_model(args)
    model = model.cuda().train()
    from models.optim import build_param_groups
    groups = build_param_groups(args, model, script)
    params = [p for g in groups for p in g["params"]]
    g = torch.Generator().manual_seed(1)
    x = NestedTensor(torch.randn(2, 4, 800, 1333, generator=g).cuda(), torch.zeros(2, 800, 1333, dtype=torch.bool, device="cuda"))
    targets = [{"labels": torch.randint(0, 3, (T,), generator=g).cuda(), "boxes": bc.rand_boxes(g, T).cuda()} for T in (3, 5)]
    kw = dict(lr=args.lr, weight_decay=args.weight_decay)
    opts = {"none": None, "foreach": torch.optim.AdamW(groups, **kw), "dfx": AdamW(groups, **kw)}
    try:
        opts["torch_fused"] = torch.optim.AdamW(groups, fused=True, **kw)
    except Exception as e:          # noqa: BLE001
        print(f"torch.optim.AdamW(fused=True) does not construct on this build: {type(e).__name__}: {e}")
    times = {r: [] for r in opts}
    bc.set_route("fused")
    for i in range(warmup + repeats):
        for r, opt in opts.items():
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = bc.one_call(crit, model(x), targets)
            if i == 0 and r == "none":      # the first pass: initial weights, the seed's dropout masks - comparable between runs
                total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict).item()
                print(f"first pass (DFX_LINEAR_BF16_TRAIN={os.environ.get('DFX_LINEAR_BF16_TRAIN', '0')}): weighted loss {total:.6f}; "
                      + ", ".join(f"{k} {losses[k].item():.6f}" for k in ("loss_ce", "loss_bbox", "loss_giou") if k in losses))
            if r == "dfx":
                opt.step(max_norm=max_norm)
            elif opt is not None:
                torch.nn.utils.clip_grad_norm_(params, max_norm)
                opt.step()
            torch.cuda.synchronize()
            if i >= warmup:
                times[r].append(time.perf_counter() - t0)
    for r, t in times.items():
        what = "no optimizer step" if r == "none" else f"clip + AdamW on the {r} route"
        print(f"train step, single-frame Late Fusion, 2 x 800 x 1333, forward + criterion + backward, {what}: "
              f"median {statistics.median(t) * 1e3:.1f} ms (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}; {repeats} repeats after {warmup})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="all", choices=["all"] + list(SETS))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--linear-bf16-min-elements", type=int, default=None, help="with --train-step: override the bf16 train route's size rule")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim_step.py measures on the GPU; there is no CPU timing"
    if args.train_step:
        return train_step(min(args.repeats, 5), min(args.warmup, 2), args.linear_bf16_min_elements)
    for name in (SETS if args.set == "all" else [args.set]):
        if args.kernels:
            time_kernels(name, args.launches, min(args.repeats, 10))
        else:
            time_routes(name, args.repeats, args.warmup)


if __name__ == "__main__":
    main()
