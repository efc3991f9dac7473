"""Stamped duration of the level-in-LDS MSDA kernel (block-major operands, encoder geometry 50 x 84) for N frames with
per-query offsets of `spread` px:  python tools/level_time.py [spread]   (DFX_LEVEL_NOT_PERSISTENT=1: one workgroup per item)
python tools/level_time.py --backward: the same stamps for the grad_value kernel of the level's backward (csrc/msda_level_backward.hip),
float and fixed-point policy, 4 and 32 frames of 4200 and of 300 queries; median and smallest of 40 launches each."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "depth-fusion-in-transformer-based-video-object-detection_amd"))
import torch

from dfx import ops

dev = torch.device("cuda:0")
H, W = 50, 84
S = H * W
torch.manual_seed(0)


def backward():
    for N, Lq in ((4, 4200), (32, 4200), (4, 300), (32, 300)):
        g = torch.Generator().manual_seed(N + Lq)
        grad_out, logits = torch.randn(N, Lq, 256, generator=g).to(dev), torch.randn(N, Lq, 32, generator=g).to(dev)
        offsets = (2.5 * torch.randn(N, Lq, 64, generator=g)).to(dev)
        ref = torch.rand(N, Lq, 1, 2, generator=g).to(dev)
        for fixed in (False, True):
            for _ in range(3):
                ops.msda_level_grad_value(grad_out, ref, offsets, logits, N, H, W, deterministic=fixed)
            torch.cuda.synchronize()
            ops.profile_start()
            for _ in range(40):
                ops.msda_level_grad_value(grad_out, ref, offsets, logits, N, H, W, deterministic=fixed)
            torch.cuda.synchronize()
            t = sorted(r[0] for r in ops.profile_stop() if (r[2], r[3]) == (Lq, S))
            assert len(t) == 40, len(t)
            print(f"[level] [grad_value {'fixed' if fixed else 'float'} {N:2d} x {Lq:4d}] median {t[20] * 1e6:8.2f} us  min {t[0] * 1e6:8.2f} us", flush=True)


if "--backward" in sys.argv[1:]:
    backward()
    sys.exit(0)
spread = float(sys.argv[1]) if len(sys.argv) > 1 else 2.5
for N in (32, 8, 4):
    value_blk = torch.randn(64, N * S, 4, device=dev)
    qproj = torch.randn(8, N * S, 12, device=dev)
    qproj[..., :8] *= spread
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H, (torch.arange(W) + 0.5) / W, indexing="ij")
    ref = torch.stack([xs.reshape(-1), ys.reshape(-1)], -1).view(1, S, 1, 2).expand(N, S, 1, 2).contiguous().to(dev)
    big = torch.empty(96 * 1024 * 1024, device=dev)             # 384 MB: evicts the operands from the Infinity Cache
    for _ in range(3):
        ops.msda_level_forward(value_blk, ref, qproj, N, H, W)
    torch.cuda.synchronize()
    ops.profile_start()
    for _ in range(20):
        big.fill_(1.0)
        ops.msda_level_forward(value_blk, ref, qproj, N, H, W)
    torch.cuda.synchronize()
    rec = ops.profile_stop()
    t = sorted(r[0] for r in rec)
    nbytes = rec[0][1]
    med = t[len(t) // 2]
    print(f"N={N:2d}  median {med * 1e6:7.2f} us  min {t[0] * 1e6:7.2f} us  algorithmic {nbytes / 1e6:.1f} MB -> {nbytes / med / 1e12:.2f} TB/s = {nbytes / med / 8e12:.3f} of 8 TB/s", flush=True)
