#!/usr/bin/env python
"""The DFormer depth stem under a training step (the same file times any commit of this project: --pkg names the package
directory to import):

  stem     models.dformer_backbone.DFormerBackbone(train_backbone=True, freeze_batchnorm=False) in train mode: forward +
           backward of the three stages that run, every parameter asking for a gradient, on --frames depth maps of
           800 x 1333 (default 1, 2, 4, 8 and 32 frames, one after the other).
  layers   each BatchNorm of the stem alone on the map it sees there (16 channels of 400 x 667 with the GELU, 32 of 200 x 334,
           64 of 100 x 167), input and parameters asking for a gradient: what the per-layer size rule is read from.

Where models/fused.py has the DFORMER_TRAIN switch the two routes (dfx.ops.batch_norm_train / the modules) alternate in one
process, --reps times each with the size rules set to 0 (--shipped-rule keeps those of models/fused.py: what a training
step takes by default); elsewhere the one route the commit has is timed.

With --parent-pkg DIR (a built copy of the parent commit's package) the tool itself starts no GPU work: it runs this file in
fresh child processes, alternating this tree and the parent --rounds times, and prints the medians over the rounds side by
side.  Per repetition: HIP events around the forward launches and around the backward launches of the passes after --warmup
(device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: the medians and
every repetition's total (the spread is what a difference has to exceed).  Nothing is asserted.

    python tools/bench_dformer_train.py [--frames 1,2,4,8,32] [--iters 0] [--warmup 2] [--reps 3] [--pkg DIR] [--label NAME]
    python tools/bench_dformer_train.py --parent-pkg DIR [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
H, W = 800, 1333
LAYERS = [("BN16 + GELU 400x667", 16, 400, 667, True), ("BN32 200x334", 32, 200, 334, False), ("BN64 100x167", 64, 100, 167, False)]


def one_pass(fn, leaves, gout, iters, warmup):
    """(forward seconds, backward seconds) per pass: events around each launch group, summed over `iters` passes"""
    import torch
    for _ in range(warmup):
        torch.autograd.grad(fn(), leaves, gout)
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in marks:
        a.record()
        out = fn()
        b.record()
        torch.autograd.grad(out, leaves, gout)
        c.record()
    torch.cuda.synchronize()
    return (sum(a.elapsed_time(b) for a, b, _ in marks) * 1e-3 / iters, sum(b.elapsed_time(c) for _, b, c in marks) * 1e-3 / iters)


def record(label, what, route, times):
    tot = [f + b for f, b in times]
    rec = {"label": label, "what": what, "route": route, "forward_ms": statistics.median(f for f, _ in times) * 1e3,
           "backward_ms": statistics.median(b for _, b in times) * 1e3, "total_ms": statistics.median(tot) * 1e3,
           "reps_ms": [t * 1e3 for t in tot]}
    print(f"[{label}] [{what:28s}] {route:7s} forward {rec['forward_ms']:8.3f} ms  backward {rec['backward_ms']:8.3f} ms  total median "
          f"{rec['total_ms']:8.3f} ms  reps {' '.join(f'{t:.3f}' for t in rec['reps_ms'])}", flush=True)
    return rec


def measure(args):
    """Times both workloads in this process with the package at args.pkg -> list of result records (also printed)."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from torch import nn
    from models import fused
    from models.dformer_backbone import DFormerBackbone
    from util.misc import NestedTensor
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    switch = hasattr(fused, "DFORMER_TRAIN")
    routes = [("kernels", True), ("library", False)] if switch else [("library", None)]
    if switch and not args.shipped_rule:
        fused.DFORMER_TRAIN_MIN_PIXELS = 0
        if hasattr(fused, "DFORMER_TRAIN_MIN_PIXELS_GELU"):
            fused.DFORMER_TRAIN_MIN_PIXELS_GELU = 0

    def select(on):
        if switch:
            fused.DFORMER_TRAIN = on

    def alternate(what, fn, leaves, gout, iters):
        times = {r: [] for r, _ in routes}
        for rep in range(args.reps + 1):                     # (repetition 0 warms both routes up and is dropped)
            for r, on in routes:
                select(on)
                t = one_pass(fn, leaves, gout, iters, args.warmup)
                if rep:
                    times[r].append(t)
        select(True)
        return [record(args.label, what, r, times[r]) for r, _ in routes]

    print(f"[{args.label}] {args.reps} repetitions after {args.warmup} warm-up passes; routes: {', '.join(r for r, _ in routes)}"
          + (" (alternating)" if switch else ""), flush=True)
    records = []
    for frames in args.frames:
        iters = args.iters or max(3, 32 // frames)
        g = torch.Generator().manual_seed(frames)
        if not args.no_stem:
            torch.manual_seed(0)
            net = DFormerBackbone(train_backbone=True, freeze_batchnorm=False).cuda().train()
            depth = torch.randn(frames, 1, H, W, generator=g).cuda()
            nt = NestedTensor(depth, torch.zeros(frames, H, W, dtype=torch.bool, device="cuda"))
            stages = net.depth_backbone.downsample_layers_e[:-1]
            leaves = list(stages.parameters())
            fn = lambda: net(nt)["0"].tensors                    # noqa: E731
            gout = torch.randn_like(fn().detach())
            records += alternate(f"stem {frames} x {H} x {W}", fn, leaves, gout, iters)
            del net, depth, nt, leaves, gout
        if not args.no_layers:
            for name, C, h, w, gelu in LAYERS:
                torch.manual_seed(0)
                bn, act = nn.BatchNorm2d(C).cuda().train(), nn.GELU()
                seq = nn.Sequential(bn, act) if gelu else nn.Sequential(bn)
                x = torch.randn(frames, C, h, w, generator=g).cuda().requires_grad_()
                gout = torch.randn(frames, C, h, w, generator=g).cuda()
                if switch:
                    from models.dformer_backbone import _run_stage_train
                    fn = lambda: _run_stage_train(seq, x) if fused.DFORMER_TRAIN else seq(x)     # noqa: E731
                else:
                    fn = lambda: seq(x)                                                           # noqa: E731
                records += alternate(f"{frames} x {name}", fn, [x] + list(bn.parameters()), gout, iters)
                del bn, seq, x, gout
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(records), flush=True)
    return records


def compare(args):
    """Alternates child processes on this tree and on the parent's package; medians over the rounds, one table."""
    runs, order = {}, []
    for rnd in range(args.rounds):
        for label, pkg in (("this tree", args.pkg), ("parent", args.parent_pkg)):
            cmd = [sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--label", label, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--frames", ",".join(str(f) for f in args.frames)]
            cmd += (["--no-stem"] if args.no_stem else []) + (["--no-layers"] if args.no_layers else []) + (["--shipped-rule"] if args.shipped_rule else [])
            env = dict(os.environ)
            env.pop("DFX_LIBRARY", None)
            env.pop("DFX_DFORMER_TRAIN", None)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=args.child_timeout)
            sys.stdout.write("".join(l + "\n" for l in res.stdout.splitlines() if not l.startswith("RESULT ")))
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"round {rnd}: the run on {label} ended with {res.returncode}; nothing more is started")
            for rec in json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:]):
                runs.setdefault((rec["what"], label, rec["route"]), []).append(rec)
                if rec["what"] not in order:
                    order.append(rec["what"])
    med = lambda key, field: statistics.median(r[field] for r in runs[key])      # noqa: E731
    spread = lambda key: (lambda t: f"{min(t):.3f}-{max(t):.3f}")([t for r in runs[key] for t in r["reps_ms"]])      # noqa: E731
    lines = ["| workload | parent fwd + bwd ms (smallest-largest) | this tree, DFX_DFORMER_TRAIN=0 ms (smallest-largest) | kernels: fwd ms | bwd ms | "
             "total ms (smallest-largest) | parent / kernels |", "|---|---|---|---|---|---|---|"]
    for what in order:
        par, off, on = (what, "parent", "library"), (what, "this tree", "library"), (what, "this tree", "kernels")
        lines.append(f"| {what} | {med(par, 'total_ms'):.3f} ({spread(par)}) | {med(off, 'total_ms'):.3f} ({spread(off)}) | "
                     f"{med(on, 'forward_ms'):.3f} | {med(on, 'backward_ms'):.3f} | {med(on, 'total_ms'):.3f} ({spread(on)}) | "
                     f"{med(par, 'total_ms') / med(on, 'total_ms'):.2f}x |")
    table = "\n".join(lines) + "\n"
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"medians over {args.rounds} alternating rounds of {args.reps} repetitions; HIP-event device time\n\n" + table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=lambda s: [int(v) for v in s.split(",")], default=[1, 2, 4, 8, 32])
    ap.add_argument("--iters", type=int, default=0, help="passes per repetition (0: max(3, 32 // frames))")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pkg", default=PKG)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-stem", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--shipped-rule", action="store_true", help="keep the size rules of models/fused.py (default: 0, every layer on the route)")
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_pkg:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
