#!/usr/bin/env python
"""RoIAlign backward (csrc/roi_align.hip, NHWC) at the bench geometry: 32 images of 50 x 84 x 256, 9600 RoIs
(32 frames x 300 queries), 7 x 7 bins, sampling_ratio 2, spatial_scale 1/32.

Prints, per box set and per kernel form (merged per-axis taps / plain four adds per sample, DFX_ROI_BWD_PLAIN):
time per launch from HIP events around --iters launches after --warmup (the entry point's zero fill of grad_input
included), the atomic bytes added per launch (host-side count of pixel rows x C x 4 bytes), bytes / time, and the
forward's time on the same inputs.  Nothing is asserted.  --deterministic times the fixed-point twin of each form
(csrc/fixed_sum.h: int64 workspace zero fill, absmax, adds, convert) alternating with the float form, --reps times each,
and prints medians, every repetition and fixed / float.

Box sets: "image" = boxes of an 800 x 1344 image, which spatial_scale 1/32 puts on the top-left 25 x 42 of the
stride-16 map (the quirk of the reference that the model keeps); "map" = boxes spread over the whole 50 x 84 map.
Both: centres uniform over the area widened by 10 % a side, sides 1/16 .. 1/2 of the area's.

    python tools/bench_roi_backward.py [--iters 20] [--warmup 3] [--deterministic [--reps 5]]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"))

N, H, W, C, Q, SIZE, SR, SCALE = 32, 50, 84, 256, 300, 7, 2, 1 / 32
GUIDE_RATE = 1.3e12     # chip-wide fp32 atomic-add rate of the MI355X, bytes added per second (a published guide figure)


def boxes(area_h, area_w, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(N * Q, generator=g)
    cx, cy = (u() * 1.2 - 0.1) * area_w, (u() * 1.2 - 0.1) * area_h
    w, h = (1 / 16 + u() * (1 / 2 - 1 / 16)) * area_w, (1 / 16 + u() * (1 / 2 - 1 / 16)) * area_h
    b = torch.arange(N).repeat_interleave(Q).float()
    return torch.stack([b, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def axis_rows(start, side, n):
    """Per (RoI, bin) of one axis: valid samples, and distinct map rows with a non-zero merged weight - the fp32
    arithmetic of load_roi / locate."""
    binw = (side / SIZE)[:, None, None]
    i = torch.arange(SIZE, dtype=torch.float32)[None, :, None]
    s = torch.arange(SR, dtype=torch.float32)[None, None, :]
    v = start[:, None, None] + i * binw + (s + 0.5) * binw / SR
    ok = ~((v < -1.0) | (v > n))
    v = v.clamp(min=0.0)
    lo = v.clamp(max=float(n)).long()
    top = lo >= n - 1
    lo = torch.where(top, torch.full_like(lo, n - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    frac = torch.where(top, lo.float(), v) - lo.float()
    wsum = torch.zeros(v.shape[0], SIZE, n)
    wsum.scatter_add_(2, lo, (1.0 - frac) * ok)
    wsum.scatter_add_(2, hi, frac * ok)
    return ok.sum(2), (wsum != 0).sum(2)


def atomic_rows(rois):
    """(merged, plain) pixel rows added per launch."""
    x1, y1 = rois[:, 1] * SCALE - 0.5, rois[:, 2] * SCALE - 0.5
    rw, rh = rois[:, 3] * SCALE - 0.5 - x1, rois[:, 4] * SCALE - 0.5 - y1
    oky, rows = axis_rows(y1, rh, H)
    okx, cols = axis_rows(x1, rw, W)
    merged = (rows[:, :, None] * cols[:, None, :]).sum().item()
    plain = 4 * (oky[:, :, None] * okx[:, None, :]).sum().item()
    return merged, plain


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
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import statistics
    from dfx import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g).cuda()
    go = torch.randn(N * Q, SIZE * SIZE, C, generator=g).cuda()
    bins = N * Q * SIZE * SIZE
    print(f"RoIAlign backward NHWC: {N} x {H} x {W} x {C}, {N * Q} RoIs, {SIZE}x{SIZE} bins, sr {SR}, scale 1/32; "
          f"{args.iters} launches after {args.warmup}")
    for name, rois in (("image", boxes(800, 1344, 2)), ("map", boxes(H / SCALE, W / SCALE, 3))):
        merged, plain = atomic_rows(rois)
        r = rois.cuda()
        t_fwd = timed(lambda: ops.roi_align(x, r, SIZE, SCALE, SR, True, channels_last=True), args.iters, args.warmup)
        print(f"[{name}] forward {t_fwd * 1e6:9.1f} us")
        for form, rows, env in (("merged", merged, None), ("plain", plain, "1")):
            if env is None:
                os.environ.pop("DFX_ROI_BWD_PLAIN", None)
            else:
                os.environ["DFX_ROI_BWD_PLAIN"] = env
            ops.reload_tuning()
            run = lambda det=False: timed(lambda: ops.roi_align_backward(go, r, (N, H, W, C), SIZE, SCALE, SR, True,
                                                                        channels_last=True, **({"deterministic": True} if det else {})),
                                          args.iters, args.warmup)
            if args.deterministic:
                reps = [(run(False), run(True)) for _ in range(args.reps)]
                flt, fix = statistics.median(a for a, _ in reps), statistics.median(b for _, b in reps)
                print(f"[{name}] backward {form:6s} float {flt * 1e6:9.1f} us  fixed {fix * 1e6:9.1f} us  fixed / float {fix / flt:5.2f}x  "
                      f"reps (float, fixed) {' '.join(f'({a * 1e6:.1f}, {b * 1e6:.1f})' for a, b in reps)}")
            t = run()
            nbytes = rows * C * 4
            print(f"[{name}] backward {form:6s} {t * 1e6:9.1f} us   {rows / bins:5.2f} atomic rows / bin   "
                  f"{nbytes / 1e9:6.3f} GB added   {nbytes / t / 1e12:5.2f} TB/s   "
                  f"({nbytes / GUIDE_RATE * 1e6:7.1f} us at the guide's 1.3 TB/s)")
        os.environ.pop("DFX_ROI_BWD_PLAIN", None)
        ops.reload_tuning()


if __name__ == "__main__":
    main()
