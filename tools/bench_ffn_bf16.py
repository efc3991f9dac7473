#!/usr/bin/env python
"""One FFN of a transformer layer in GPU inference, norm(x + linear2(relu(linear1(x)))) with 256 -> 1024 -> 256 columns, on its
two routes in one process, alternating:

  fp32    the fused fp32 route as it stands: dfx.ops.linear (+ bias + ReLU), dfx.ops.linear, dfx.ops.add_layernorm
  bf16    models.fused.LINEAR_BF16: dfx.ops.linear_bf16 (fp32 in, bf16 hidden tensor out), dfx.ops.linear_bf16 (+ residual),
          dfx.ops.add_layernorm

at 32 x 4200, 12 x 4200, 4 x 4200, 9600 and 300 rows, and the single-Linear GELU FFN of the fusion layers (256 -> 256) at
32 x 4200 and 4 x 4200 rows.  Both routes are called through the layer's own forward_ffn with the switch toggled.  Three launches
per FFN on either route (two for the GELU FFN).

Per repetition: HIP events around --iters passes after --warmup (device time of the three launches, the host's launch gaps
included).  Printed per workload and route: the median over --reps repetitions, the smallest and largest repetition (the spread a
difference has to exceed), and - from one profiled pass (dfx_profile_*: the kernels' own begin / end stamps) - each GEMM's time,
its one-pass bytes (inputs + outputs + weights) over that time as a fraction of 8 TB/s, and its TFLOP/s.  Also the relative
deviation of the bf16 route's output from the fp32 route's.  Nothing is asserted.

    python tools/bench_ffn_bf16.py [--iters 20] [--warmup 3] [--reps 5] [--out profiles/r21_ffn_bf16.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd")
ROWS = [32 * 4200, 12 * 4200, 4 * 4200, 9600, 300]
FUSION_ROWS = [32 * 4200, 4 * 4200]
HBM = 8e12


def gemm_bytes(M, N, K, a_bytes, c_bytes, w_bytes, residual):
    return M * K * a_bytes + M * N * c_bytes + N * K * w_bytes + N * 4 + (M * N * 4 if residual else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_ffn_bf16.txt"))
    args = ap.parse_args()
    sys.path.insert(0, PKG)
    import torch
    from dfx import ops
    from models import fused, transformer_layers as tl
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def passes(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / n

    def workload(name, layer, rows, gemms):
        """gemms: route -> [(M, N, K, bytes)] of the route's GEMM launches, in launch order"""
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, 256, generator=g).cuda()
        times, outs = {"fp32": [], "bf16": []}, {}
        with torch.no_grad():
            for rep in range(args.reps + 1):                     # (repetition 0 warms both routes up and is dropped)
                for route in ("fp32", "bf16"):
                    fused.LINEAR_BF16 = route == "bf16"
                    passes(lambda: layer.forward_ffn(x), args.warmup)
                    t = passes(lambda: layer.forward_ffn(x), args.iters)
                    if rep:
                        times[route].append(t)
            for route in ("fp32", "bf16"):
                fused.LINEAR_BF16 = route == "bf16"
                ops.profile_start()
                outs[route] = layer.forward_ffn(x)
                torch.cuda.synchronize()
                kernels = [(sec, ta) for (sec, _, ta, _) in ops.profile_stop() if ta in (-2, -5) and sec > 0]
                med = statistics.median(times[route])
                say(f"[{name:28s}] {route}  median {med * 1e6:9.1f} us per FFN  (repetitions {min(times[route]) * 1e6:.1f} - "
                    f"{max(times[route]) * 1e6:.1f} us)")
                if len(kernels) != len(gemms[route]) or any(ta != (-5 if route == "bf16" else -2) for _, ta in kernels):
                    say(f"    unexpected GEMM launches (seconds, family): {kernels}")
                    continue
                for (sec, _), (M, N, K, nbytes) in zip(kernels, gemms[route]):
                    say(f"    GEMM {M} x {N} x {K}: {sec * 1e6:8.1f} us, {nbytes / 1e6:7.1f} MB one-pass -> {nbytes / sec / 1e9:7.0f} GB/s = "
                        f"{nbytes / sec / HBM:.3f} of 8 TB/s, {2.0 * M * N * K / sec / 1e12:6.1f} TFLOP/s")
        fused.LINEAR_BF16 = False
        a, b = statistics.median(times["fp32"]), statistics.median(times["bf16"])
        beyond = min(times["fp32"]) > max(times["bf16"]) or min(times["bf16"]) > max(times["fp32"])
        dev = ((outs["bf16"] - outs["fp32"]).norm() / outs["fp32"].norm()).item()
        say(f"[{name:28s}] fp32 / bf16 = {a / b:.2f}x ({'beyond' if beyond else 'INSIDE'} the repetition spread); "
            f"output deviation (relative L2) {dev:.2e}")

    say(f"{args.reps} repetitions x {args.iters} passes after {args.warmup}, the routes alternating; HIP-event time per FFN (3 launches), "
        "kernel stamps per GEMM")
    torch.manual_seed(0)
    ffn = tl.DeformableTransformerDecoderLayer(256, 1024, 0.1, "relu", 1, 8, 4).cuda().eval()
    for rows in ROWS:
        gemms = {"fp32": [(rows, 1024, 256, gemm_bytes(rows, 1024, 256, 4, 4, 4, False)), (rows, 256, 1024, gemm_bytes(rows, 256, 1024, 4, 4, 4, False))],
                 "bf16": [(rows, 1024, 256, gemm_bytes(rows, 1024, 256, 4, 2, 2, False)), (rows, 256, 1024, gemm_bytes(rows, 256, 1024, 2, 4, 2, True))]}
        workload(f"FFN 256-1024-256, {rows} rows", ffn, rows, gemms)
    fusion = tl.DeformableTransformerFusionLayerV2(256, 1024, 0.1, "gelu", 1, 8, 4).cuda().eval()
    for rows in FUSION_ROWS:
        gemms = {"fp32": [(rows, 256, 256, gemm_bytes(rows, 256, 256, 4, 4, 4, False))], "bf16": [(rows, 256, 256, gemm_bytes(rows, 256, 256, 4, 4, 2, False))]}
        workload(f"GELU FFN 256-256, {rows} rows", fusion, rows, gemms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
