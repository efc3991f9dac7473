#!/usr/bin/env python
"""One MSDeformAttn(256, 4, 8, 4) forward + backward in grad mode, through the module's public surface only (so the same
file times any commit of this project: --pkg names the package directory to import).

Geometries (L = 4 levels of an 800 x 1333 frame: 100x167, 50x84, 25x42, 13x21; --frames frames per call):
    encoder           Lq = S = 22223 per frame, query and memory need gradients, 2-d reference points
    decoder           Lq = 300, query and memory need gradients
    decoder-detached  Lq = 300, the memory is detached (a fixed pretrained single-frame model): no value gradient
    decoder-box       Lq = 300, 4-d reference points (box refinement)

--set single: MSDeformAttn(256, 1, 8, 4) over the ONE level of the depth-fusion layers (50 x 84 = 4200 tokens):
    encoder-1l           Lq = S = 4200 per frame, query and memory need gradients
    decoder-1l           Lq = 300, query and memory need gradients
    encoder-1l-detached  Lq = 4200, the memory is detached and value_proj frozen (with a trainable value_proj the value
                         map still needs its gradient): no value gradient, the LDS grad_value kernel must not run
Here the routes are those of grad_value in dfx.ops.msda_fused_backward where the tree has the switch (dfx.ops.USE_LEVEL_BWD):
"lds" (csrc/msda_level_backward.hip) and "atomics" alternate in one process; a tree without it has "atomics" only.  The
launches of the LDS kernel in one pass are counted and printed.  --deterministic adds the fixed-point twin of each route
("lds-fixed", "atomics-fixed": dfx.ops.deterministic_mode() forced on, csrc/fixed_sum.h) to the alternation and prints
fixed / float per route.

Where the module has the MSDA_TRAIN switch (models/ops/modules/ms_deform_attn.py) the two routes - fused forward + fused
backward, and the operator sequence with MSDeformAttnFunction - alternate in one process, --reps times each; elsewhere
the one route the commit has is timed.  Per repetition: HIP events around the forward launches and around the backward
launches of --iters passes (x 25 at Lq = 300, so that a repetition lasts some hundreds of milliseconds) after --warmup
(device time per launch group, the host's launch gaps included: that is what a training step pays).  Printed: every repetition's total (the spread is what a difference has to exceed), the medians
of forward, backward and total, and torch.cuda.max_memory_allocated of one pass above what is held before it.
Nothing is asserted.

    python tools/bench_msda_train.py [--iters 20] [--warmup 3] [--reps 5] [--frames 4] [--set multi|single] [--only GEOMETRY]
                                     [--deterministic] [--pkg DIR] [--label NAME]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(100, 167), (50, 84), (25, 42), (13, 21)]
# (name, Lq or None = S, ref_dim, the memory needs a gradient, passes per repetition as a multiple of --iters: a repetition
# lasts some hundreds of milliseconds at every geometry)
GEOMETRIES = [("encoder", None, 2, True, 1), ("decoder", 300, 2, True, 25), ("decoder-detached", 300, 2, False, 25),
              ("decoder-box", 300, 4, True, 25)]
SINGLE_SIZES = [(50, 84)]
SINGLE_GEOMETRIES = [("encoder-1l", None, 2, True, 10), ("decoder-1l", 300, 2, True, 25), ("encoder-1l-detached", None, 2, False, 10)]
LEVEL_ENTRIES = ("dfx_msda_level_grad_value_f32", "dfx_msda_level_grad_value_fixed_f32")


def one_pass(fn, leaves, gout, iters, warmup):
    """(forward seconds, backward seconds) per pass: events around each launch group, summed over `iters` passes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--set", choices=("multi", "single"), default="multi")
    ap.add_argument("--only", default=None, help="time this geometry alone")
    ap.add_argument("--deterministic", action="store_true", help="--set single: time the fixed-point twins as well")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "depth-fusion-in-transformer-based-video-object-detection_amd"))
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from dfx import ops
    from models.ops.modules import MSDeformAttn
    from models.ops.modules import ms_deform_attn as mod_file
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    single = args.set == "single"
    sizes, geometries = (SINGLE_SIZES, SINGLE_GEOMETRIES) if single else (SIZES, GEOMETRIES)
    if single:
        switch = hasattr(ops, "USE_LEVEL_BWD")
        routes = [("lds", True), ("atomics", False)] if switch else [("atomics", None)]
        if args.deterministic:      # (route, LDS switch, deterministic mode)
            assert switch and hasattr(ops, "deterministic_mode"), "this tree has no deterministic mode"
            routes = [(r + tail, (on, det)) for r, on in routes for tail, det in (("", "0"), ("-fixed", "1"))]
    else:
        switch = hasattr(mod_file, "MSDA_TRAIN")
        routes = [("fused", True), ("operator", False)] if switch else [("operator", None)]

    def take(on):
        if switch and single and args.deterministic:
            ops.USE_LEVEL_BWD, ops._DETERMINISTIC_ENV = on
        elif switch and single:
            ops.USE_LEVEL_BWD = on
        elif switch:
            mod_file.MSDA_TRAIN = on

    launches, real_call = [], getattr(ops, "_call", None)
    if single and real_call is not None:       # count the LDS kernel's launches (outside the timed passes)
        def counting_call(what, name, *a):
            launches.append(name)
            return real_call(what, name, *a)

    L = len(sizes)
    torch.manual_seed(0)
    m = MSDeformAttn(256, L, 8, 4).cuda().train()
    with torch.no_grad():     # the initialisation zeroes these; spread the samples as a trained layer does
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    shapes = torch.as_tensor(sizes, dtype=torch.long, device="cuda")
    areas = shapes[:, 0] * shapes[:, 1]
    lsi = torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])
    N, S = args.frames, int(areas.sum())
    print(f"[{args.label}] MSDeformAttn(256, {L}, 8, 4) forward + backward, {N} frames, S {S}; {args.reps} x {args.iters} passes after "
          f"{args.warmup}; routes: {', '.join(r for r, _ in routes)}" + (" (alternating)" if switch else ""))
    for name, Lq, ref_dim, need_memory, scale in geometries:
        if args.only not in (None, name):
            continue
        iters = args.iters * scale
        for p in m.value_proj.parameters():     # single set: "detached" means no value gradient at all
            p.requires_grad_(need_memory or not single)
        Lq = S if Lq is None else Lq
        g = torch.Generator().manual_seed(Lq + ref_dim)
        query = torch.randn(N, Lq, 256, generator=g).cuda().requires_grad_()
        memory = torch.randn(N, S, 256, generator=g).cuda().requires_grad_(need_memory)
        ref = torch.rand(N, Lq, L, ref_dim, generator=g)
        if ref_dim == 4:
            ref[..., 2:] = 0.05 + 0.3 * ref[..., 2:]
        ref = ref.cuda()
        gout = torch.randn(N, Lq, 256, generator=g).cuda()
        leaves = [query] + ([memory] if need_memory else []) + [p for p in m.parameters() if p.requires_grad]
        fn = lambda: m(query, ref, memory, shapes, lsi)
        times = {r: [] for r, _ in routes}
        for _ in range(args.reps):
            for r, on in routes:
                take(on)
                times[r].append(one_pass(fn, leaves, gout, iters, args.warmup))
        peak, lds_launches = {}, {}
        for r, on in routes:
            take(on)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch.autograd.grad(fn(), leaves, gout)
            torch.cuda.synchronize()
            peak[r] = torch.cuda.max_memory_allocated() - base
            if single and real_call is not None:
                del launches[:]
                ops._call = counting_call
                try:
                    torch.autograd.grad(fn(), leaves, gout)
                    torch.cuda.synchronize()
                finally:
                    ops._call = real_call
                lds_launches[r] = sum(launches.count(e) for e in LEVEL_ENTRIES)
        tag = f"[{args.label}] [{name:16s} Lq {Lq:6d} ref_dim {ref_dim} passes {iters:4d}]"
        med = {}
        for r, _ in routes:
            tot = [f + b for f, b in times[r]]
            med[r] = statistics.median(tot)
            print(f"{tag} {r:8s} forward {statistics.median(f for f, _ in times[r]) * 1e3:8.3f} ms  backward "
                  f"{statistics.median(b for _, b in times[r]) * 1e3:8.3f} ms  total median {med[r] * 1e3:8.3f} ms  "
                  f"reps {' '.join(f'{t * 1e3:.3f}' for t in tot)}  peak above the inputs {peak[r] / 1e6:8.1f} MB"
                  + (f"  LDS grad_value launches per pass {lds_launches[r]}" if r in lds_launches else ""))
        if switch and single:
            print(f"{tag} atomics / lds {med['atomics'] / med['lds']:5.2f}x")
            if args.deterministic:
                print(f"{tag} fixed / float: lds {med['lds-fixed'] / med['lds']:5.2f}x  atomics {med['atomics-fixed'] / med['atomics']:5.2f}x"
                      f"   atomics-fixed / lds-fixed {med['atomics-fixed'] / med['lds-fixed']:5.2f}x")
            take((True, None) if args.deterministic else True)
        elif switch:
            print(f"{tag} operator / fused {med['operator'] / med['fused']:5.2f}x   peak memory {peak['operator'] / 1e6:.1f} -> "
                  f"{peak['fused'] / 1e6:.1f} MB")
            mod_file.MSDA_TRAIN = True


if __name__ == "__main__":
    main()
