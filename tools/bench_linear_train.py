#!/usr/bin/env python
"""One models.fused.Linear forward + backward in grad mode (input, weight and bias all ask for a gradient), the call the FFNs
and the MSDeformAttn projections make in a training step (so the same file times any commit of this project: --pkg names the
package directory to import).

Shapes: rows F x 4200 (encoder tokens of a 50 x 84 level) and F x 300 (queries) for F = 4 and 32; widths in -> out
    256 -> 256    value_proj / output_proj          256 -> 1024   FFN linear1        1024 -> 256   FFN linear2
    256 -> 64     sampling_offsets, single level    256 -> 32     attention_weights, single level
    256 -> 128    attention_weights, four levels

Where models/fused.py has the LINEAR_TRAIN switch three routes alternate in one process, --reps times each: the MFMA route
with the split rule's two candidates (at least 32 / at least 16 row steps per range of the weight gradient:
dfx.ops._WGRAD_MIN_STEPS; --max-ranges sets dfx.ops._WGRAD_MAX_RANGES for both) and nn.Linear (the switch off); elsewhere the one route the commit has is timed.  With
--parent-pkg DIR (a built copy of the parent commit's package) the tool itself starts no GPU work: it runs this file in
fresh child processes, alternating this tree and the parent --rounds times, and prints the medians over the rounds side by
side.

Per repetition: HIP events around the forward launches and around the backward launches of --iters passes after --warmup
(device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: the medians
of forward, backward and total and every repetition's total (the spread is what a difference has to exceed).  Nothing is
asserted.

    python tools/bench_linear_train.py [--iters 20] [--warmup 3] [--reps 3] [--pkg DIR] [--label NAME]
    python tools/bench_linear_train.py --parent-pkg DIR [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
ROWS = [("4 x 300", 1200), ("4 x 4200", 16800), ("32 x 300", 9600), ("32 x 4200", 134400)]
WIDTHS = [(256, 256), (256, 1024), (1024, 256), (256, 64), (256, 32), (256, 128)]


def one_pass(fn, leaves, gout, iters, warmup):
    """(forward seconds, backward seconds) per pass: events around each launch group, summed over `iters` passes."""
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


def measure(args):
    """Times every shape in this process with the package at args.pkg -> list of result records (also printed)."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from dfx import ops
    from models import fused
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    switch = hasattr(fused, "LINEAR_TRAIN")
    routes = [("mfma32", True, 32), ("mfma16", True, 16), ("library", False, 32)] if switch else [("library", None, None)]

    def select(on, steps):
        if switch:
            fused.LINEAR_TRAIN = on
            ops._WGRAD_MIN_STEPS = steps

    print(f"[{args.label}] models.fused.Linear forward + backward; {args.reps} x {args.iters} passes after {args.warmup}; "
          f"routes: {', '.join(r for r, _, _ in routes)}" + (" (alternating)" if switch else ""), flush=True)
    if switch and args.max_ranges:
        ops._WGRAD_MAX_RANGES = args.max_ranges
    warm = fused.Linear(256, 256).cuda()            # (clocks, allocator and the libraries' first calls: not on the first shape's account)
    xw = torch.randn(1200, 256, device="cuda", requires_grad=True)
    for r, on, steps in routes:
        select(on, steps)
        one_pass(lambda: warm(xw), [xw] + list(warm.parameters()), torch.ones(1200, 256, device="cuda"), 20, 3)
    records = []
    for rows_name, M in ROWS:
        for K, N in WIDTHS:
            torch.manual_seed(0)
            m = fused.Linear(K, N).cuda().train()
            g = torch.Generator().manual_seed(M + K + N)
            x = torch.randn(M, K, generator=g).cuda().requires_grad_()
            gout = torch.randn(M, N, generator=g).cuda()
            leaves = [x] + list(m.parameters())
            fn = lambda: m(x)                                   # noqa: E731
            times = {r: [] for r, _, _ in routes}
            for _ in range(args.reps):
                for r, on, steps in routes:
                    select(on, steps)
                    times[r].append(one_pass(fn, leaves, gout, args.iters, args.warmup))
            for r, on, steps in routes:
                tot = [f + b for f, b in times[r]]
                select(on, steps)
                rec = {"label": args.label, "rows": rows_name, "M": M, "K": K, "N": N, "route": r,
                       "splits": ops._wgrad_splits(M, N, K) if switch and on else None,
                       "forward_ms": statistics.median(f for f, _ in times[r]) * 1e3,
                       "backward_ms": statistics.median(b for _, b in times[r]) * 1e3,
                       "total_ms": statistics.median(tot) * 1e3, "reps_ms": [t * 1e3 for t in tot]}
                records.append(rec)
                print(f"[{args.label}] [{rows_name:9s} {K:4d} -> {N:4d}] {r:7s} forward {rec['forward_ms']:7.3f} ms  backward "
                      f"{rec['backward_ms']:7.3f} ms  total median {rec['total_ms']:7.3f} ms  reps "
                      f"{' '.join(f'{t:.3f}' for t in rec['reps_ms'])}  ranges {rec['splits']}", flush=True)
            select(True, 32)
            del m, x, gout, leaves
    print("RESULT " + json.dumps(records), flush=True)
    return records


def compare(args):
    """Alternates child processes on this tree and on the parent's package; medians over the rounds, one table."""
    runs = {}
    for rnd in range(args.rounds):
        for label, pkg in (("this tree", args.pkg), ("parent", args.parent_pkg)):
            cmd = [sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--label", label, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--max-ranges", str(args.max_ranges)]
            env = dict(os.environ)
            env.pop("DFX_LIBRARY", None)
            env.pop("DFX_LINEAR_TRAIN", None)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=args.child_timeout)
            sys.stdout.write("".join(l + "\n" for l in res.stdout.splitlines() if not l.startswith("RESULT ")))
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"round {rnd}: the run on {label} ended with {res.returncode}; nothing more is started")
            for rec in json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:]):
                runs.setdefault((rec["M"], rec["K"], rec["N"], label, rec["route"]), []).append(rec)
    lines = ["| rows | in -> out | parent fwd + bwd ms (spread) | this tree, DFX_LINEAR_TRAIN=0 ms | MFMA route, >= 32 steps: fwd ms | bwd ms "
             "| total ms (spread) | ranges | >= 16 steps: total ms | ranges | parent / >= 32 steps | parent / >= 16 steps |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    med = lambda key, field: statistics.median(r[field] for r in runs[key])
    spread = lambda key: (lambda t: f"{min(t):.3f}-{max(t):.3f}")([t for r in runs[key] for t in r["reps_ms"]])
    for rows_name, M in ROWS:
        for K, N in WIDTHS:
            par, off = (M, K, N, "parent", "library"), (M, K, N, "this tree", "library")
            on, on16 = (M, K, N, "this tree", "mfma32"), (M, K, N, "this tree", "mfma16")
            lines.append(f"| {rows_name} | {K} -> {N} | {med(par, 'total_ms'):.3f} ({spread(par)}) | {med(off, 'total_ms'):.3f} | "
                         f"{med(on, 'forward_ms'):.3f} | {med(on, 'backward_ms'):.3f} | {med(on, 'total_ms'):.3f} ({spread(on)}) | "
                         f"{runs[on][0]['splits']} | {med(on16, 'total_ms'):.3f} | {runs[on16][0]['splits']} | "
                         f"{med(par, 'total_ms') / med(on, 'total_ms'):.2f}x | {med(par, 'total_ms') / med(on16, 'total_ms'):.2f}x |")
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
    ap.add_argument("--pkg", default=PKG)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-ranges", type=int, default=0, help="0: the rule's own limit")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_pkg:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
