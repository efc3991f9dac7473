#!/usr/bin/env python
"""One models.fused.Linear forward + backward in grad mode (input, weight and bias all ask for a gradient) on the fp32 route
(dfx.ops.linear_train) and on the opt-in bf16 route (models.fused.LINEAR_BF16_TRAIN -> dfx.ops.linear_bf16_train), alternating in
one process.  Modelled on tools/bench_linear_train.py.

Shapes: the FFN's 256 -> 1024 and 1024 -> 256, the 256 -> 256 projections and the two narrow projections of a single-level
MSDeformAttn (256 -> 64, 256 -> 32) at 32 x 4200, 12 x 4200 and 4 x 4200 encoder tokens, 9600 and 300 queries.

Per repetition: HIP events around the forward launches and around the backward launches of --iters passes after --warmup (device
time per launch group, the host's launch gaps included: that is what a training step pays).  Printed per shape and route: the
median of --reps repetitions of forward, backward and total with the smallest and largest total.  For the bf16 route also the
three products' own kernel times (the library's per-launch timestamps, dfx.ops.profile_start: median of --reps passes with the
smallest and largest) with the bytes they must move (fp32 operands read once, the bf16 weight copy read once, fp32 results
written once; the weight gradient's partial slabs written and read once more) and their flops, as TB/s and TFLOP/s; and the
cost of rebuilding the two bf16 weight copies, which every optimizer step makes stale (models.fused.bf16_weight_pair).
Nothing is asserted.

    python tools/bench_linear_bf16_train.py [--iters 20] [--warmup 3] [--reps 5] [--out FILE]
    python tools/bench_linear_bf16_train.py --ranges 8,16,32,64,128,256 [--out FILE]     # the weight gradient alone, by range count
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"))
ROWS = [("32 x 4200", 134400), ("12 x 4200", 50400), ("4 x 4200", 16800), ("9600", 9600), ("300", 300)]
WIDTHS = [(256, 1024), (1024, 256), (256, 256)]
NARROW = [(256, 64), (256, 32)]         # sampling_offsets and attention_weights of a single-level MSDeformAttn: the 64 x 128 tile
ROUTES = [("fp32", False), ("bf16", True)]


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


def kernel_times(fn, leaves, gout, reps):
    """[(forward, grad_x, grad_w kernel, grad_w reduction) seconds] of `reps` profiled passes on the bf16 route"""
    import torch
    from dfx import ops
    out = []
    for _ in range(reps):
        ops.profile_start()
        torch.autograd.grad(fn(), leaves, gout)
        torch.cuda.synchronize()
        rec = [(sec, tag) for sec, _, tag, _ in ops.profile_stop() if tag in (-5, -6, -7)]
        gemm = [s for s, t in rec if t == -5]
        assert len(gemm) == 2 and sum(t == -6 for _, t in rec) == 1, rec
        out.append((gemm[0], gemm[1], sum(s for s, t in rec if t == -6), sum(s for s, t in rec if t == -7)))
    return out


def copies_time(m, iters):
    """seconds per rebuild of the two bf16 weight copies (a stale key: what the first forward after an optimizer step pays)"""
    import torch
    from models import fused
    for _ in range(3):
        m.__dict__.pop("_weight_bf16_pair", None)
        fused.bf16_weight_pair(m)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        m.__dict__.pop("_weight_bf16_pair", None)
        fused.bf16_weight_pair(m)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def range_counts(args, say):
    """--ranges: the weight gradient alone (kernel + reduction, dfx.ops.linear_bf16_backward(need_x=False)) over a list of
    requested range counts, every shape: what the split rule's two constants are chosen from."""
    import torch
    from dfx import ops
    med = statistics.median
    say(f"bf16 weight gradient alone, kernel + reduction launch, by requested ranges; median of {args.reps} repetitions of {args.iters} "
        f"calls after {args.warmup} (smallest - largest), HIP-event device time")
    for rows_name, M in ROWS:
        for K, N in WIDTHS + NARROW:
            g = torch.Generator().manual_seed(M + K + N)
            x, gout = torch.randn(M, K, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
            wt = torch.zeros(K, N, dtype=torch.bfloat16, device="cuda")
            rule = ops._wgrad_bf16_splits(M, N, K)
            seen, cands = set(), []
            for want in [rule] + [int(v) for v in args.ranges.split(",")]:
                n = ops._wgrad_bf16_ranges(M, max(1, want))[1]
                if n not in seen and n * ops._wgrad_tiles(N, K)[0] <= 2 * ops._wgrad_tiles(N, K)[1]:
                    seen.add(n)
                    cands.append(n)
            times = {n: [] for n in cands}
            for _ in range(args.reps):
                for n in cands:
                    call = lambda: ops.linear_bf16_backward(gout, x, wt, need_x=False, splits=n)      # noqa: E731
                    for _ in range(args.warmup):
                        call()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.iters):
                        call()
                    b.record()
                    torch.cuda.synchronize()
                    times[n].append(a.elapsed_time(b) * 1e-3 / args.iters)
            say(f"[{rows_name:9s} {K:4d} -> {N:4d}] rule {rule:3d} | " + " | ".join(
                f"{n:3d}: {med(times[n]) * 1e6:6.1f} ({min(times[n]) * 1e6:.1f}-{max(times[n]) * 1e6:.1f})" for n in sorted(cands)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranges", default=None, help="e.g. 8,16,32,64,128,256: time the weight gradient alone at these range counts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from dfx import ops
    from models import fused
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.ranges:
        range_counts(args, say)
        return finish()
    say(f"models.fused.Linear forward + backward, fp32 route and bf16 route alternating; median of {args.reps} repetitions of "
        f"{args.iters} passes after {args.warmup} (smallest - largest); HIP-event device time; kernel times from the library's launch stamps")
    fused.LINEAR_BF16_TRAIN_MIN_ELEMENTS = 0            # (the size rule is what this table decides: every shape takes the route here)
    warm = fused.Linear(256, 256).cuda()           # (clocks, allocator and the libraries' first calls: not on the first shape's account)
    xw = torch.randn(1200, 256, device="cuda", requires_grad=True)
    for _, on in ROUTES:
        fused.LINEAR_BF16_TRAIN = on
        one_pass(lambda: warm(xw), [xw] + list(warm.parameters()), torch.ones(1200, 256, device="cuda"), 20, 3)
    med = statistics.median
    for rows_name, M in ROWS:
        for K, N in WIDTHS + NARROW:
            torch.manual_seed(0)
            m = fused.Linear(K, N).cuda().train()
            g = torch.Generator().manual_seed(M + K + N)
            x = torch.randn(M, K, generator=g).cuda().requires_grad_()
            gout = torch.randn(M, N, generator=g).cuda()
            leaves = [x] + list(m.parameters())
            fn = lambda: m(x)                                   # noqa: E731
            times = {r: [] for r, _ in ROUTES}
            for _ in range(args.reps):
                for r, on in ROUTES:
                    fused.LINEAR_BF16_TRAIN = on
                    times[r].append(one_pass(fn, leaves, gout, args.iters, args.warmup))
            tot = {r: [f + b for f, b in times[r]] for r, _ in ROUTES}
            for r, _ in ROUTES:
                say(f"[{rows_name:9s} {K:4d} -> {N:4d}] {r}  forward {med(f for f, _ in times[r]) * 1e6:8.1f} us  backward "
                    f"{med(b for _, b in times[r]) * 1e6:8.1f} us  total {med(tot[r]) * 1e6:8.1f} us ({min(tot[r]) * 1e6:.1f} - {max(tot[r]) * 1e6:.1f})")
            beyond = max(tot["bf16"]) < min(tot["fp32"])
            say(f"[{rows_name:9s} {K:4d} -> {N:4d}] fp32 / bf16 = {med(tot['fp32']) / med(tot['bf16']):.2f}x "
                f"({'beyond' if beyond else 'INSIDE'} the repetition spread)")
            fused.LINEAR_BF16_TRAIN = True
            kt = kernel_times(fn, leaves, gout, args.reps)
            splits = ops._wgrad_bf16_splits(M, N, K)
            io = (M * K + M * N) * 4 + N * K * 2                # forward and input gradient: two fp32 matrices and the bf16 weight
            wbytes = (M * K + M * N) * 4 + (N * K + N) * 4 * (2 * splits + 1 if splits > 1 else 1)
            flops = 2.0 * M * N * K
            for i, (what, nbytes) in enumerate((("forward", io), ("grad_x", io), ("grad_w kernel", wbytes), ("grad_w reduction", 0))):
                t = [k[i] for k in kt]
                if med(t) <= 0:
                    continue
                rate = f"{nbytes / med(t) * 1e-12:5.2f} TB/s  {flops / med(t) * 1e-12:6.1f} TFLOP/s" if nbytes else f"({splits} ranges; its bytes are in the kernel's line)"
                say(f"[{rows_name:9s} {K:4d} -> {N:4d}]   {what:16s} {med(t) * 1e6:8.1f} us ({min(t) * 1e6:.1f} - {max(t) * 1e6:.1f})  {rate}")
            say(f"[{rows_name:9s} {K:4d} -> {N:4d}]   rebuilding the two bf16 weight copies: {copies_time(m, 50) * 1e6:.1f} us per optimizer step")
            fused.LINEAR_BF16_TRAIN = False
            del m, x, gout, leaves
    finish()


if __name__ == "__main__":
    main()
