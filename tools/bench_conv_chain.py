"""conv3 + next conv1 as one launch (dfx.ops.conv1x1_chain) beside the two launches it replaces, on the five producer
shapes of ResNet-50 layer1 / layer2 at an 800x1333 frame.  Alternating rounds in one process, median and minimum of the
event-timed launches; prints one line per shape.

    python tools/bench_conv_chain.py [frames=32] [rounds=7]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"), ROOT]
from dfx import ops  # noqa: E402

# (name, Co, K1, K2, C1, H, W)
SHAPES = [("layer1[1,2] conv3 -> conv1", 256, 64, 0, 64, 200, 334),
          ("layer1[0] conv3+shortcut -> conv1", 256, 64, 64, 64, 200, 334),
          ("layer1[2] conv3 -> layer2[0] conv1", 256, 64, 0, 128, 200, 334),
          ("layer2[0..2] conv3 -> conv1", 512, 128, 0, 128, 100, 167),
          ("layer2[3] conv3 -> layer3[0] conv1", 512, 128, 0, 256, 100, 167)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, Co, K1, K2, C1, H, W in SHAPES:
        rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
        x = rnd(frames, K1, H, W)
        x2 = rnd(frames, K2, H, W) if K2 else None
        res = None if K2 else rnd(frames, Co, H, W)
        w3, b3 = rnd(Co, K1 + K2) / (K1 + K2) ** 0.5, rnd(Co)
        w1, b1 = rnd(C1, Co) / Co ** 0.5, rnd(C1)

        def two():
            y = ops.conv1x1(x, w3, b3, residual=res, relu=True) if x2 is None else ops.conv1x1_pair(x, x2, w3, b3, relu=True)
            return y, ops.conv1x1(y, w1, b1, relu=True)

        def one():
            return ops.conv1x1_chain(x, w3, b3, w1, b1, residual=res, x2=x2)

        ya, za = two()
        yb, zb = one()
        same = torch.equal(ya, yb) and torch.equal(za, zb)
        del ya, za, yb, zb
        t2, t1 = [], []
        for _ in range(rounds):
            t2.append(timed(two))
            t1.append(timed(one))
        flops = 2.0 * frames * H * W * (Co * (K1 + K2) + C1 * Co)
        # bytes the chain must move: X, residual, Y, Z once
        nbytes = 4.0 * frames * H * W * (K1 + K2 + (0 if K2 else Co) + Co + C1)
        m2, m1 = statistics.median(t2), statistics.median(t1)
        print(f"{name:38s} Co={Co} K={K1 + K2} C1={C1} frames={frames}: two launches {m2:.3f} ms (min {min(t2):.3f}), "
              f"chain {m1:.3f} ms (min {min(t1):.3f}), {m2 / m1:.3f}x, chain {flops / m1 * 1e-9:.1f} TFLOP/s "
              f"{nbytes / m1 * 1e-9:.2f} TB/s, outputs {'EQUAL' if same else 'DIFFER'}", flush=True)
        del x, x2, res


if __name__ == "__main__":
    main()
