#!/usr/bin/env python
"""The front of the detector under a training step (the same file times any commit of this project: --pkg names the package
directory to import):

  projections   one models.detector_common._ConvGN forward + backward in grad mode (input, convolution and norm all ask for a
                gradient) at --frames (4) frames of 50 x 84: Conv2d(2048, 256, 1) + GroupNorm(32, 256) (RGB) and Conv2d(128, 256, 1) +
                GroupNorm (depth).  Where models/fused.py has the CONVGN_TRAIN switch the two routes alternate in one process,
                --reps times each; elsewhere the one route the commit has is timed.
  backbone      the forward of the frozen ResNet-50 body (FrozenBatchNorm2d, dilated, fused_inference on, every parameter
                frozen) in grad mode at 4 x 800 x 1333: op by op on a commit that routes on grad mode alone, the fused
                inference route on one that asks whether anything needs a gradient.

With --parent-pkg DIR (a built copy of the parent commit's package) the tool itself starts no GPU work: it runs this file in
fresh child processes, alternating this tree and the parent --rounds times, and prints the medians over the rounds side by
side.  Per repetition: HIP events around the forward launches and around the backward launches of --iters passes after
--warmup (device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: the
medians and every repetition's total (the spread is what a difference has to exceed).  Nothing is asserted.

    python tools/bench_convgn_train.py [--iters 20] [--warmup 3] [--reps 3] [--frames 4] [--pkg DIR] [--label NAME]
    python tools/bench_convgn_train.py --parent-pkg DIR [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
PROJECTIONS = [("rgb 2048 -> 256", 2048), ("depth 128 -> 256", 128)]
H, W = 50, 84


def one_pass(fn, leaves, gout, iters, warmup):
    """(forward seconds, backward seconds) per pass: events around each launch group, summed over `iters` passes;
    leaves = None times the forward alone."""
    import torch
    back = (lambda out: torch.autograd.grad(out, leaves, gout)) if leaves else (lambda out: None)
    for _ in range(warmup):
        back(fn())
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for a, b, c in marks:
        a.record()
        out = fn()
        b.record()
        back(out)
        c.record()
    torch.cuda.synchronize()
    return (sum(a.elapsed_time(b) for a, b, _ in marks) * 1e-3 / iters, sum(b.elapsed_time(c) for _, b, c in marks) * 1e-3 / iters)


def record(label, what, route, times):
    tot = [f + b for f, b in times]
    rec = {"label": label, "what": what, "route": route, "forward_ms": statistics.median(f for f, _ in times) * 1e3,
           "backward_ms": statistics.median(b for _, b in times) * 1e3, "total_ms": statistics.median(tot) * 1e3,
           "reps_ms": [t * 1e3 for t in tot]}
    print(f"[{label}] [{what:18s}] {route:7s} forward {rec['forward_ms']:8.3f} ms  backward {rec['backward_ms']:8.3f} ms  total median "
          f"{rec['total_ms']:8.3f} ms  reps {' '.join(f'{t:.3f}' for t in rec['reps_ms'])}", flush=True)
    return rec


def measure(args):
    """Times both workloads in this process with the package at args.pkg -> list of result records (also printed)."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from models import fused
    from models.backbone_scratch import FusionBackbone
    from models.detector_common import _conv_gn
    from util.misc import NestedTensor
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    switch = hasattr(fused, "CONVGN_TRAIN")
    routes = [("kernels", True), ("library", False)] if switch else [("library", None)]

    def select(on):
        if switch:
            fused.CONVGN_TRAIN = on

    print(f"[{args.label}] {args.reps} x {args.iters} passes after {args.warmup}; projection routes: {', '.join(r for r, _ in routes)}"
          + (" (alternating)" if switch else ""), flush=True)
    records = []
    for name, cin in PROJECTIONS:
        torch.manual_seed(0)
        m = _conv_gn(cin, 256).cuda().train()
        g = torch.Generator().manual_seed(cin)
        x = torch.randn(args.frames, cin, H, W, generator=g).cuda().requires_grad_()
        gout = torch.randn(args.frames, H * W, 256, generator=g).cuda().transpose(1, 2).unflatten(2, (H, W))    # token-major, as it flows back
        leaves = [x] + list(m.parameters())
        fn = lambda: m(x)                                   # noqa: E731
        times = {r: [] for r, _ in routes}
        for rep in range(args.reps + 1):                     # (repetition 0 warms both routes up and is dropped)
            for r, on in routes:
                select(on)
                t = one_pass(fn, leaves, gout, args.iters, args.warmup)
                if rep:
                    times[r].append(t)
        records += [record(args.label, name, r, times[r]) for r, _ in routes]
        select(True)
        del m, x, gout, leaves
    if not args.no_backbone:
        torch.manual_seed(0)
        bb = FusionBackbone("resnet50", "resnet18", False, None, True, True, "Baseline_rgb", [3], 256, False).cuda().eval()
        bb.fused_inference = True
        assert not any(p.requires_grad for p in bb.body.parameters())
        frames = torch.randn(4, 3, 800, 1333, generator=torch.Generator().manual_seed(1)).cuda()
        nt = NestedTensor(frames, torch.zeros(4, 800, 1333, dtype=torch.bool, device="cuda"))
        assert torch.is_grad_enabled()
        times = [one_pass(lambda: bb(nt), None, None, max(1, args.iters // 4), 2) for _ in range(args.reps)]
        records.append(record(args.label, "frozen body 4x800x1333", "forward", times))
    print("RESULT " + json.dumps(records), flush=True)
    return records


def compare(args):
    """Alternates child processes on this tree and on the parent's package; medians over the rounds, one table."""
    runs = {}
    for rnd in range(args.rounds):
        for label, pkg in (("this tree", args.pkg), ("parent", args.parent_pkg)):
            cmd = [sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--label", label, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--frames", str(args.frames)] + (["--no-backbone"] if args.no_backbone else [])
            env = dict(os.environ)
            env.pop("DFX_LIBRARY", None)
            env.pop("DFX_CONVGN_TRAIN", None)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=args.child_timeout)
            sys.stdout.write("".join(l + "\n" for l in res.stdout.splitlines() if not l.startswith("RESULT ")))
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"round {rnd}: the run on {label} ended with {res.returncode}; nothing more is started")
            for rec in json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:]):
                runs.setdefault((rec["what"], label, rec["route"]), []).append(rec)
    med = lambda key, field: statistics.median(r[field] for r in runs[key])      # noqa: E731
    spread = lambda key: (lambda t: f"{min(t):.3f}-{max(t):.3f}")([t for r in runs[key] for t in r["reps_ms"]])      # noqa: E731
    lines = ["| workload | parent fwd + bwd ms (smallest-largest) | this tree, DFX_CONVGN_TRAIN=0 ms (smallest-largest) | kernels: fwd ms | bwd ms | "
             "total ms (smallest-largest) | parent / kernels |", "|---|---|---|---|---|---|---|"]
    for name, _ in PROJECTIONS:
        par, off, on = (name, "parent", "library"), (name, "this tree", "library"), (name, "this tree", "kernels")
        lines.append(f"| {args.frames} x {H} x {W}, {name} | {med(par, 'total_ms'):.3f} ({spread(par)}) | {med(off, 'total_ms'):.3f} ({spread(off)}) | "
                     f"{med(on, 'forward_ms'):.3f} | {med(on, 'backward_ms'):.3f} | {med(on, 'total_ms'):.3f} ({spread(on)}) | "
                     f"{med(par, 'total_ms') / med(on, 'total_ms'):.2f}x |")
    if not args.no_backbone:
        what = "frozen body 4x800x1333"
        par, on = (what, "parent", "forward"), (what, "this tree", "forward")
        lines += ["", "| workload | parent forward ms (smallest-largest) | this tree forward ms (smallest-largest) | parent / this tree |", "|---|---|---|---|",
                  f"| frozen ResNet-50 body in grad mode, 4 x 800 x 1333 | {med(par, 'forward_ms'):.3f} ({spread(par)}) | "
                  f"{med(on, 'forward_ms'):.3f} ({spread(on)}) | {med(par, 'forward_ms') / med(on, 'forward_ms'):.2f}x |"]
    table = "\n".join(lines) + "\n"
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"medians over {args.rounds} alternating rounds of {args.reps} x {args.iters} passes; HIP-event device time\n\n" + table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4, help="frames of 50 x 84 the projections run on")
    ap.add_argument("--pkg", default=PKG)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-backbone", action="store_true")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_pkg:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
