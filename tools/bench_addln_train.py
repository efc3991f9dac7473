#!/usr/bin/env python
"""The tail of a transformer sub-layer, norm(residual + dropout(y)), under a training step (the same file times any commit of
this project: --pkg names the package directory to import):

  tail      one models.transformer_layers._norm_add forward + backward in grad mode with all four gradients (y, the residual,
            the norm's weight and bias) at C = 256 and 4 x 300, 32 x 300, 4 x 4200, 12 x 4200 and 32 x 4200 rows, with a live
            dropout (p = 0.1) and without one (p = 0).
  layer     one whole DeformableTransformerEncoderLayer(256, 1024, 0.1, 4 levels) forward + backward in train mode at
            4 x 4200 and 32 x 4200 tokens (levels 50 x 63, 25 x 32, 13 x 16, 7 x 6).

Where models/fused.py has the ADDLN_TRAIN switch the two routes alternate in one process (the size rule set to 0 rows, so that
every size runs on the kernels), --reps times each; elsewhere the one route the commit has is timed.

With --parent-pkg DIR (a built copy of the parent commit's package) the tool itself starts no GPU work: it runs this file in
fresh child processes, alternating this tree and the parent --rounds times, and prints the medians over the rounds side by
side.  Per repetition: HIP events around the forward launches and around the backward launches of --iters passes after
--warmup (device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: the
medians and every repetition's total (the spread is what a difference has to exceed).  Nothing is asserted.

    python tools/bench_addln_train.py [--iters 20] [--warmup 3] [--reps 3] [--pkg DIR] [--label NAME] [--no-layer]
    python tools/bench_addln_train.py --parent-pkg DIR [--rounds 2] [--out FILE]
    python tools/bench_addln_train.py --inference [--iters 20] [--warmup 3] [--reps 3]       (ops.add_layernorm alone)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
TAILS = [(4, 300), (32, 300), (4, 4200), (12, 4200), (32, 4200)]
LAYERS = [4, 32]
LEVELS = [(50, 63), (25, 32), (13, 16), (7, 6)]         # 4200 tokens
C = 256


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
    print(f"[{label}] [{what:22s}] {route:7s} forward {rec['forward_ms']:8.3f} ms  backward {rec['backward_ms']:8.3f} ms  total median "
          f"{rec['total_ms']:8.3f} ms  reps {' '.join(f'{t:.3f}' for t in rec['reps_ms'])}", flush=True)
    return rec


def tail_name(frames, tokens, p):
    return f"tail {frames} x {tokens} p={p}"


def layer_name(frames):
    return f"encoder layer {frames} x 4200"


def measure(args):
    """Times the workloads in this process with the package at args.pkg -> list of result records (also printed)."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from torch import nn
    from models import fused, transformer_layers as tl
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    switch = hasattr(fused, "ADDLN_TRAIN")
    routes = [("kernels", True), ("library", False)] if switch else [("library", None)]
    if switch:
        fused.ADDLN_TRAIN_MIN_ROWS = 0

    def select(on):
        if switch:
            fused.ADDLN_TRAIN = on

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

    print(f"[{args.label}] {args.reps} x {args.iters} passes after {args.warmup}; routes: {', '.join(r for r, _ in routes)}"
          + (" (alternating)" if switch else ""), flush=True)
    records = []
    for frames, tokens in TAILS:
        for p in (0.1, 0.0):
            torch.manual_seed(0)
            norm, drop = nn.LayerNorm(C).cuda().train(), nn.Dropout(p).train()
            g = torch.Generator().manual_seed(frames * tokens)
            y, r, gout = (torch.randn(frames, tokens, C, generator=g).cuda() for _ in range(3))
            y.requires_grad_()
            r.requires_grad_()
            # the call of the layers: the dropout module handed over where the commit's _norm_add takes it, applied first elsewhere
            fn = (lambda: tl._norm_add(norm, r, y, dropout=drop)) if switch else (lambda: tl._norm_add(norm, r, drop(y)))
            records += alternate(tail_name(frames, tokens, p), fn, [y, r] + list(norm.parameters()), gout, args.iters)
            del norm, y, r, gout
    if not args.no_layer:
        shapes, lsi = tl.make_level_tensors(LEVELS, "cuda")[:2]
        for frames in LAYERS:
            torch.manual_seed(0)
            layer = tl.DeformableTransformerEncoderLayer(C, 1024, 0.1, "relu", len(LEVELS), 8, 4).cuda().train()
            with torch.no_grad():
                layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
            g = torch.Generator().manual_seed(frames)
            src, pos, gout = (torch.randn(frames, 4200, C, generator=g).cuda() for _ in range(3))
            ref = (0.05 + 0.9 * torch.rand(frames, 4200, len(LEVELS), 2, generator=g)).cuda()
            src.requires_grad_()
            fn = lambda: layer(src, pos, ref, shapes, lsi, None)                                   # noqa: E731
            records += alternate(layer_name(frames), fn, [src] + list(layer.parameters()), gout, max(2, args.iters // 4))
            del layer, src, pos, gout, ref
    print("RESULT " + json.dumps(records), flush=True)
    return records


def measure_inference(args):
    """--inference: ops.add_layernorm alone (the inference tail, no autograd) at C = 256, 32 x 4200 and 32 x 300 rows, with and
    without a residual: HIP events around --iters x 10 launches, the median of --reps repetitions in microseconds per launch."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from torch import nn
    from dfx import ops
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    norm = nn.LayerNorm(C).cuda().eval()
    records = []
    with torch.no_grad():
        for frames, tokens in ((32, 4200), (32, 300)):
            g = torch.Generator().manual_seed(frames * tokens)
            x, r = (torch.randn(frames, tokens, C, generator=g).cuda() for _ in range(2))
            for res in (r, None):
                what = f"add_layernorm {frames} x {tokens} {'residual' if res is not None else 'no residual'}"
                for _ in range(args.warmup):
                    ops.add_layernorm(x, res, norm)
                reps = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.iters * 10):
                        ops.add_layernorm(x, res, norm)
                    b.record()
                    torch.cuda.synchronize()
                    reps.append(a.elapsed_time(b) * 1e3 / (args.iters * 10))
                records.append({"label": args.label, "what": what, "us": statistics.median(reps), "reps_us": reps})
                print(f"[{args.label}] [{what:40s}] median {records[-1]['us']:8.2f} us  reps {' '.join(f'{t:.2f}' for t in reps)}", flush=True)
    print("RESULT " + json.dumps(records), flush=True)
    return records


def compare(args):
    """Alternates child processes on this tree and on the parent's package; medians over the rounds, one table."""
    runs = {}
    for rnd in range(args.rounds):
        for label, pkg in (("this tree", args.pkg), ("parent", args.parent_pkg)):
            cmd = [sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--label", label, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)] + (["--no-layer"] if args.no_layer else [])
            env = dict(os.environ)
            env.pop("DFX_LIBRARY", None)
            env.pop("DFX_ADDLN_TRAIN", None)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=args.child_timeout)
            sys.stdout.write("".join(l + "\n" for l in res.stdout.splitlines() if not l.startswith("RESULT ")))
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"round {rnd}: the run on {label} ended with {res.returncode}; nothing more is started")
            for rec in json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:]):
                runs.setdefault((rec["what"], label, rec["route"]), []).append(rec)
    med = lambda key, field: statistics.median(r[field] for r in runs[key])      # noqa: E731
    spread = lambda key: (lambda t: f"{min(t):.3f}-{max(t):.3f}")([t for r in runs[key] for t in r["reps_ms"]])      # noqa: E731
    lines = ["| workload | parent fwd + bwd ms (smallest-largest) | this tree, DFX_ADDLN_TRAIN=0 ms (smallest-largest) | kernels: fwd ms | bwd ms | "
             "total ms (smallest-largest) | parent / kernels |", "|---|---|---|---|---|---|---|"]
    names = [tail_name(f, t, p) for f, t in TAILS for p in (0.1, 0.0)] + ([] if args.no_layer else [layer_name(f) for f in LAYERS])
    for name in names:
        par, off, on = (name, "parent", "library"), (name, "this tree", "library"), (name, "this tree", "kernels")
        lines.append(f"| {name} | {med(par, 'total_ms'):.3f} ({spread(par)}) | {med(off, 'total_ms'):.3f} ({spread(off)}) | "
                     f"{med(on, 'forward_ms'):.3f} | {med(on, 'backward_ms'):.3f} | {med(on, 'total_ms'):.3f} ({spread(on)}) | "
                     f"{med(par, 'total_ms') / med(on, 'total_ms'):.2f}x |")
    table = "\n".join(lines) + "\n"
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"medians over {args.rounds} alternating rounds of {args.reps} x {args.iters} passes (layers: a quarter of the passes); "
                    "HIP-event device time\n\n" + table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pkg", default=PKG)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--inference", action="store_true", help="time ops.add_layernorm (no autograd) instead of the training tails")
    args = ap.parse_args()
    if args.inference:
        measure_inference(args)
    elif args.parent_pkg:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
