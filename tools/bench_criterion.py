"""Time one criterion call (forward + backward) on the fused route and on the op-by-op torch route.

    python tools/bench_criterion.py                          # the three shapes, both routes, host and device time
    python tools/bench_criterion.py --trace fused --calls 10   # only N calls of one route at --shape: run it under
                                                             # ``rocprofv3 --kernel-trace --stats -- python ...`` for launch counts
    python tools/bench_criterion.py --train-step             # one whole training step of the single-frame Late Fusion recipe
                                                             # at 2 x 800 x 1333 (forward, criterion, backward), each route

Shapes: ``single`` B = 4, six sets of 300 (last layer + 5 aux);  ``transvodpp`` B = 1, the sets a TransVOD++ Late Fusion model
returns in train mode (query counts read from its actual output on a small clip);  ``b32`` B = 32, six sets of 300.
Targets: 1 to 8 per image, seeded.  Both routes run in the same process on the same inputs, alternating; per route the
median over --repeats of the host clock around a call that ends in a synchronise (``wall``), of the host clock until the call
returns (``host``: what the Python thread spends; the fused route's one synchronisation is inside it), and of device events
around the call (``device``).  A GPU is required: there is no CPU timing.
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

COST = dict(cost_class=2, cost_bbox=5, cost_giou=2)


def rand_boxes(g, *lead):
    return torch.cat([0.2 + 0.6 * torch.rand(*lead, 2, generator=g), 0.05 + 0.3 * torch.rand(*lead, 2, generator=g)], -1)


def make_case(B, queries, seed=0):
    """-> (outputs with leaves that require grad, targets) on cuda; queries[0] is the last layer, the rest aux sets"""
    g = torch.Generator().manual_seed(seed)
    sets = [{"pred_logits": torch.randn(B, Q, 3, generator=g).cuda().requires_grad_(True),
             "pred_boxes": rand_boxes(g, B, Q).cuda().requires_grad_(True)} for Q in queries]
    outputs = dict(sets[0], aux_outputs=sets[1:])
    counts = torch.randint(1, 9, (B,), generator=g).tolist()
    targets = [{"labels": torch.randint(0, 3, (T,), generator=g).cuda(), "boxes": rand_boxes(g, T).cuda()} for T in counts]
    return outputs, targets


def transvodpp_queries():
    """query counts of the sets a TransVOD++ Late Fusion model returns in train mode (a 64 x 96 clip: the counts do not depend on the size)"""
    from models import build_model
    from models.config import transvodpp_args
    torch.manual_seed(0)
    model, _, _ = build_model(transvodpp_args("LateFusion", num_ref_frames=2, device="cuda"))
    model = model.cuda().train()
    from util.misc_multi import NestedTensor
    with torch.no_grad():
        out = model(NestedTensor(torch.randn(3, 4, 64, 96, device="cuda"), torch.zeros(3, 64, 96, dtype=torch.bool, device="cuda")))
    return [out["pred_logits"].shape[1]] + [a["pred_logits"].shape[1] for a in out["aux_outputs"]]


def criterion_for(n_aux):
    from models.criterion import SetCriterion
    from models.matcher import HungarianMatcher
    coef = {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2}
    wd = {k + sfx: v for sfx in [""] + [f"_{i}" for i in range(n_aux)] for k, v in coef.items()}
    return SetCriterion(3, HungarianMatcher(**COST), wd, ["labels", "boxes", "cardinality"])


def one_call(crit, outputs, targets):
    losses = crit(outputs, targets)
    sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict).backward()
    return losses


def set_route(route):
    os.environ["DFX_CRITERION"] = "1" if route == "fused" else "0"


def time_routes(name, B, queries, repeats, warmup):
    outputs, targets = make_case(B, queries)
    crit = criterion_for(len(queries) - 1)
    times = {r: {"wall": [], "host": [], "device": []} for r in ("fused", "torch")}
    values = {}
    for i in range(warmup + repeats):
        for route in ("fused", "torch"):            # alternating: both see the same machine
            set_route(route)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            losses = one_call(crit, outputs, targets)
            stop.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= warmup:
                times[route]["wall"].append(t2 - t0)
                times[route]["host"].append(t1 - t0)
                times[route]["device"].append(start.elapsed_time(stop) * 1e-3)
            values[route] = {k: v.item() for k, v in losses.items()}
    worst = max(abs(values["fused"][k] - values["torch"][k]) / max(abs(values["torch"][k]), 1e-12) for k in values["torch"])
    print(f"{name}: B={B} sets={queries} targets={[len(t['labels']) for t in targets]}  largest relative loss difference between the routes {worst:.2e}")
    med = {r: {k: statistics.median(v) for k, v in t.items()} for r, t in times.items()}
    for r in ("fused", "torch"):
        spread = (min(times[r]["wall"]), max(times[r]["wall"]))
        print(f"  {r:5s}  wall {med[r]['wall'] * 1e3:8.3f} ms (min {spread[0] * 1e3:.3f}, max {spread[1] * 1e3:.3f})   host {med[r]['host'] * 1e3:8.3f} ms   "
              f"device events {med[r]['device'] * 1e3:8.3f} ms   [{repeats} repeats after {warmup}]")
    print(f"  torch / fused wall: {med['torch']['wall'] / med['fused']['wall']:.2f}x")


def train_step(repeats, warmup):
    from models import build_model
    from models.config import single_args
    torch.manual_seed(0)
    model, crit, _ = build_model(single_args("LateFusion", device="cuda"))
    model = model.cuda().train()
    g = torch.Generator().manual_seed(1)
    from util.misc import NestedTensor
    x = NestedTensor(torch.randn(2, 4, 800, 1333, generator=g).cuda(), torch.zeros(2, 800, 1333, dtype=torch.bool, device="cuda"))
    targets = [{"labels": torch.randint(0, 3, (T,), generator=g).cuda(), "boxes": rand_boxes(g, T).cuda()} for T in (3, 5)]
    times = {"fused": [], "torch": []}
    for i in range(warmup + repeats):
        for route in ("fused", "torch"):
            set_route(route)
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_call(crit, model(x), targets)
            torch.cuda.synchronize()
            if i >= warmup:
                times[route].append(time.perf_counter() - t0)
    for r, t in times.items():
        print(f"train step, single-frame Late Fusion, 2 x 800 x 1333, forward + criterion + backward, criterion on the {r} route: "
              f"median {statistics.median(t) * 1e3:.1f} ms (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}; {repeats} repeats after {warmup})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["all", "single", "transvodpp", "b32"])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", choices=["fused", "torch"], help="run only --calls calls of this route (for a profiler run)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--train-step", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_criterion.py measures on the GPU; there is no CPU timing"
    if args.train_step:
        return train_step(min(args.repeats, 5), min(args.warmup, 2))
    shapes = {"single": lambda: (4, [300] * 6), "transvodpp": lambda: (1, transvodpp_queries()), "b32": lambda: (32, [300] * 6)}
    if args.trace:
        B, queries = shapes["single" if args.shape == "all" else args.shape]()
        outputs, targets = make_case(B, queries)
        crit = criterion_for(len(queries) - 1)
        set_route(args.trace)
        for _ in range(args.calls):
            one_call(crit, outputs, targets)
        torch.cuda.synchronize()
        print(f"trace: {args.calls} calls of the {args.trace} route, B={B} sets={queries}: divide the profiler's launch counts by {args.calls}")
        return
    for name in (shapes if args.shape == "all" else [args.shape]):
        B, queries = shapes[name]()
        time_routes(name, B, queries, args.repeats, args.warmup)


if __name__ == "__main__":
    main()
