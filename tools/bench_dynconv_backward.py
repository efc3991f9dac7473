#!/usr/bin/env python
"""DynamicConv forward + backward (csrc/dynconv.hip, csrc/dynconv_backward.hip) against the library route of grad mode
(torch.bmm + nn.LayerNorm + ReLU under autograd - what DFX_DYNCONV_TRAIN=0 selects in DynamicConv.forward), at
K = 9600 (32 frames x 300 queries) and K = 1200, R = 49, C = 256, dim_dynamic = 64.

Per K and per need_feats (on: the pooled features need a gradient; off: the memory is detached, dX is skipped), the two
routes alternate in one process, --reps times each: HIP events around --iters forward + backward passes after --warmup.
Printed: every repetition's time per pass (the spread is what a difference has to exceed), the median, the fused backward
alone with its rate against its algorithmic bytes 4 * (2 * K * 2*C*dd + 3 * K*R*C) and against the padded MFMA count
(6 products, rows padded to 64), and torch.cuda.max_memory_allocated of one forward + backward on each route (above
the inputs, which both routes hold).  Nothing is asserted.

    python tools/bench_dynconv_backward.py [--iters 20] [--warmup 3] [--reps 5] [--sizes 9600,1200]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"))

R, C, DD = 49, 256, 64
HBM_RATE, MFMA_RATE = 8e12, 157e12      # published peak figures of the MI355X: bytes/s, fp32 matrix FLOP/s


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="9600,1200")
    args = ap.parse_args()
    from dfx import ops
    n1, n2 = torch.nn.LayerNorm(DD).cuda(), torch.nn.LayerNorm(C).cuda()
    relu = torch.nn.ReLU(inplace=True)
    print(f"DynamicConv forward + backward, R {R}, C {C}, dd {DD}; {args.reps} x {args.iters} passes after {args.warmup}, routes alternating")
    for K in (int(v) for v in args.sizes.split(",")):
        g = torch.Generator().manual_seed(K)
        feats0 = torch.randn(K, R, C, generator=g).cuda()
        params = (torch.randn(K, 2 * C * DD, generator=g) / 8).cuda().requires_grad_()
        go = torch.randn(K, R, C, generator=g).cuda()
        nbytes = 4 * (2 * K * 2 * C * DD + 3 * K * R * C)
        flops = 6 * 2 * K * 64 * C * DD
        for need_feats in (True, False):
            feats = feats0.clone().requires_grad_(need_feats)
            leaves = [t for t in (feats, params, n1.weight, n1.bias, n2.weight, n2.bias) if t.requires_grad]

            def fused():
                torch.autograd.grad(ops.dynamic_conv(feats, params, n1, n2), leaves, go)

            def library():
                k1 = params[:, : C * DD].reshape(K, C, DD)
                k2 = params[:, C * DD:].reshape(K, DD, C)
                y = relu(n2(torch.bmm(relu(n1(torch.bmm(feats, k1))), k2)))
                torch.autograd.grad(y, leaves, go)

            def backward_only():
                ops.dynamic_conv_backward(go, feats.detach(), params.detach(), n1, n2, need_feats=need_feats)

            times = {"fused": [], "library": []}
            for _ in range(args.reps):
                for name, fn in (("fused", fused), ("library", library)):
                    times[name].append(timed(fn, args.iters, args.warmup))
            peak = {}
            for name, fn in (("fused", fused), ("library", library)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
            t_bwd = statistics.median(timed(backward_only, args.iters, args.warmup) for _ in range(args.reps))
            skipped = 0 if need_feats else 4 * K * R * C
            tag = f"[K {K:5d} need_feats {'on ' if need_feats else 'off'}]"
            for name in ("fused", "library"):
                ts = times[name]
                print(f"{tag} {name:8s} forward + backward: median {statistics.median(ts) * 1e3:8.3f} ms   "
                      f"reps {' '.join(f'{t * 1e3:.3f}' for t in ts)}   peak above the inputs {peak[name] / 1e9:6.3f} GB")
            mf = flops if need_feats else flops * 5 // 6
            print(f"{tag} fused backward alone: {t_bwd * 1e3:8.3f} ms   {(nbytes - skipped) / 1e9:5.2f} GB -> "
                  f"{(nbytes - skipped) / t_bwd / 1e12:5.2f} TB/s ({(nbytes - skipped) / t_bwd / HBM_RATE:5.1%} of 8 TB/s)   "
                  f"{mf / 1e12:5.2f} TFLOP padded -> {mf / t_bwd / 1e12:6.1f} TFLOP/s ({mf / t_bwd / MFMA_RATE:5.1%} of 157)   "
                  f"library / fused {statistics.median(times['library']) / statistics.median(times['fused']):5.2f}x")


if __name__ == "__main__":
    main()
