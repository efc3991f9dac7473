#!/usr/bin/env python
"""One nn.MultiheadAttention(256, 8) forward + backward in grad mode through models.transformer_layers._mha, the call the
300-query layers make (so the same file times any commit of this project: --pkg names the package directory to import).

Geometries (B, Lq, Lk), each with attention dropout p = 0 and p = 0.1 (the reference's default), module in train mode:
    self-4     4 x 300 x 300     decoder-layer self-attention of a 4-frame block (q = k = x + pos, v = x)
    self-32   32 x 300 x 300     the same over 32 frames
    cross-4    4 x 300 x 2400    temporal query encoder cross-attention to a long list of reference queries

Where models/fused_mha.py has the MHA_TRAIN switch the two routes - fused attention forward + backward between library
Linears, and nn.MultiheadAttention itself - alternate in one process, --reps times each; elsewhere the one route the commit
has is timed.  With --parent-pkg DIR (a built copy of the parent commit's package) the tool itself starts no GPU work: it
runs this file in fresh child processes, alternating this tree and the parent --rounds times, and prints the medians over
the rounds side by side.

Per repetition: HIP events around the forward launches and around the backward launches of --iters passes after --warmup
(device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: the medians
of forward, backward and total, every repetition's total (the spread is what a difference has to exceed), and
torch.cuda.max_memory_allocated of one pass above what is held before it.  Nothing is asserted.

    python tools/bench_mha_train.py [--iters 50] [--warmup 5] [--reps 5] [--pkg DIR] [--label NAME]
    python tools/bench_mha_train.py --parent-pkg DIR [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
GEOMETRIES = [("self-4", 4, 300, 300), ("self-32", 32, 300, 300), ("cross-4", 4, 300, 2400)]
DROPOUTS = [0.0, 0.1]


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
    """Times every geometry in this process with the package at args.pkg -> list of result records (also printed)."""
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from models import fused_mha
    from models.transformer_layers import _mha
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    switch = hasattr(fused_mha, "MHA_TRAIN")
    routes = [("fused", True), ("module", False)] if switch else [("module", None)]
    print(f"[{args.label}] nn.MultiheadAttention(256, 8) forward + backward through _mha; {args.reps} x {args.iters} passes after "
          f"{args.warmup}; routes: {', '.join(r for r, _ in routes)}" + (" (alternating)" if switch else ""), flush=True)
    records = []
    for name, B, Lq, Lk in GEOMETRIES:
        for p in DROPOUTS:
            torch.manual_seed(0)
            m = torch.nn.MultiheadAttention(256, 8, dropout=p).cuda().train()
            g = torch.Generator().manual_seed(B + Lq + Lk)
            x = torch.randn(B, Lq, 256, generator=g).cuda().requires_grad_()
            pos = torch.randn(B, Lq, 256, generator=g).cuda()
            ref = torch.randn(B, Lk, 256, generator=g).cuda().requires_grad_()
            gout = torch.randn(B, Lq, 256, generator=g).cuda()
            if name.startswith("self"):
                leaves = [x] + list(m.parameters())

                def fn():
                    qk = x + pos
                    return _mha(m, qk, qk, x)
            else:
                leaves = [x, ref] + list(m.parameters())

                def fn():
                    return _mha(m, x + pos, ref, ref)
            times = {r: [] for r, _ in routes}
            for _ in range(args.reps):
                for r, on in routes:
                    if switch:
                        fused_mha.MHA_TRAIN = on
                    times[r].append(one_pass(fn, leaves, gout, args.iters, args.warmup))
            for r, on in routes:
                if switch:
                    fused_mha.MHA_TRAIN = on
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                torch.autograd.grad(fn(), leaves, gout)
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                tot = [f + b for f, b in times[r]]
                rec = {"label": args.label, "geometry": name, "B": B, "Lq": Lq, "Lk": Lk, "p": p, "route": r,
                       "forward_ms": statistics.median(f for f, _ in times[r]) * 1e3,
                       "backward_ms": statistics.median(b for _, b in times[r]) * 1e3,
                       "total_ms": statistics.median(tot) * 1e3, "reps_ms": [t * 1e3 for t in tot], "peak_mb": peak / 1e6}
                records.append(rec)
                print(f"[{args.label}] [{name:8s} {B:2d} x {Lq} x {Lk:4d} p {p:.1f}] {r:6s} forward {rec['forward_ms']:7.3f} ms  backward "
                      f"{rec['backward_ms']:7.3f} ms  total median {rec['total_ms']:7.3f} ms  reps "
                      f"{' '.join(f'{t:.3f}' for t in rec['reps_ms'])}  peak above the inputs {rec['peak_mb']:7.1f} MB", flush=True)
            if switch:
                fused_mha.MHA_TRAIN = True
    print("RESULT " + json.dumps(records), flush=True)
    return records


def compare(args):
    """Alternates child processes on this tree and on the parent's package; medians over the rounds, one table."""
    runs = {}
    for rnd in range(args.rounds):
        for label, pkg in (("this tree", args.pkg), ("parent", args.parent_pkg)):
            cmd = [sys.executable, os.path.abspath(__file__), "--pkg", pkg, "--label", label, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            env = dict(os.environ)
            env.pop("DFX_LIBRARY", None)
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env, timeout=args.child_timeout)
            sys.stdout.write("".join(l + "\n" for l in res.stdout.splitlines() if not l.startswith("RESULT ")))
            sys.stdout.flush()
            if res.returncode != 0:
                raise SystemExit(f"round {rnd}: the run on {label} ended with {res.returncode}; nothing more is started")
            for rec in json.loads(next(l for l in res.stdout.splitlines() if l.startswith("RESULT "))[7:]):
                runs.setdefault((rec["geometry"], rec["p"], label, rec["route"]), []).append(rec)
    lines = ["| geometry (B x Lq x Lk) | p | parent (module) fwd + bwd ms | this tree, DFX_MHA_TRAIN=0 ms | this tree, fused: fwd ms | bwd ms "
             "| total ms | parent / fused | peak MB parent -> fused |", "|---|---|---|---|---|---|---|---|---|"]
    med = lambda key, field: statistics.median(r[field] for r in runs[key])
    for name, B, Lq, Lk in GEOMETRIES:
        for p in DROPOUTS:
            par, off, on = (name, p, "parent", "module"), (name, p, "this tree", "module"), (name, p, "this tree", "fused")
            lines.append(f"| {name} {B} x {Lq} x {Lk} | {p:.1f} | {med(par, 'total_ms'):.3f} | {med(off, 'total_ms'):.3f} | "
                         f"{med(on, 'forward_ms'):.3f} | {med(on, 'backward_ms'):.3f} | {med(on, 'total_ms'):.3f} | "
                         f"{med(par, 'total_ms') / med(on, 'total_ms'):.2f}x | {med(par, 'peak_mb'):.1f} -> {med(on, 'peak_mb'):.1f} |")
    table = "\n".join(lines) + "\n"
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"medians over {args.rounds} alternating rounds of {args.reps} x {args.iters} passes; HIP-event device time\n\n" + table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg", default=PKG)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_pkg:
        compare(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
