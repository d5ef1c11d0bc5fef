#!/usr/bin/env python3
"""What the accelerated Chambolle-Pock solver costs per iteration and what it saves in iterations, on one GPU, one process:
ms per iteration of ``ChambollePock``'s kernel pair (fused=False, persistent=False: 3 Nd + 6 words per voxel), of its one-sweep path
(2 Nd + 5), of ``AcceleratedChambollePock``'s kernel pair (3 Nd + 5) and of its one-sweep path (``set_fused(True)``: 2 Nd + 5), then
iterations and wall time of ``run_until(1e-3, 400)`` for ``ChambollePock`` (default path) and for the accelerated solver on both paths.
Same process, the four loops timed in turn, twice; the smaller median counts.
usage: timeout 900 python tools/cp_accel_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytv-4d_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch, pytv
from bench import synth_slab

args = sys.argv[1:]
shape = tuple(int(v) for v in args.pop(0).split("x")) if args and "x" in args[0] else (64, 8, 1024, 1024)
schemes = args or ["upwind", "downwind", "central", "hybrid"]
dev = torch.device("cuda", 0)
LAM, KW = 25.0, dict(reg_z_over_reg=1.0, reg_time=1.0)


def timed(fn, n=6, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def make(kind, x0, scheme):
    if kind == "pair":
        return pytv.solvers.ChambollePock(x0, LAM, scheme=scheme, fused=False, persistent=False, **KW)
    if kind == "one-sweep":
        return pytv.solvers.ChambollePock(x0, LAM, scheme=scheme, **KW)
    s = pytv.solvers.AcceleratedChambollePock(x0, LAM, scheme=scheme, **KW)
    s.set_fused(kind == "accelerated one-sweep")
    return s


KINDS = ("pair", "one-sweep", "accelerated", "accelerated one-sweep")
V = float(np.prod(shape))
x0 = synth_slab(shape, 0, shape[0], dev)
print("== %s fp32 (%.0f Mvox), lambda %g, %r; frac = words x 4 bytes x voxels / time / 8 TB/s" % ("x".join(map(str, shape)), V / 1e6, LAM, KW), flush=True)
for scheme in schemes:
    best, words, label = {}, {}, {}
    for rep in range(2):
        for kind in KINDS:
            s = make(kind, x0, scheme)
            nd = s.geo.nd
            if kind == "one-sweep":
                label[kind] = "one-sweep" if s.fused else "default (no one-sweep here)"
                words[kind] = (2 * nd + 5) if s.fused else (3 * nd + 6)
            elif kind == "accelerated one-sweep":
                label[kind], words[kind] = kind, 2 * nd + 5
            else:
                label[kind], words[kind] = kind, 3 * nd + (6 if kind == "pair" else 5)
            t = timed(s.step)
            best[kind] = min(best.get(kind, t), t)
            del s
            torch.cuda.empty_cache()
    for kind in KINDS:
        note = ""
        if kind == "accelerated":
            note = "   accelerated / pair = %.3f" % (best["accelerated"] / best["pair"])
        elif kind == "accelerated one-sweep":
            note = "   / accelerated = %.3f   / one-sweep = %.3f" % (best[kind] / best["accelerated"], best[kind] / best["one-sweep"])
        print("  %-8s %-21s %8.3f ms / iteration  (%2d words, frac %.2f)%s" % (scheme, label[kind], best[kind], words[kind],
                                                                             words[kind] * 4 * V / best[kind] / 1e6 / 8000, note), flush=True)
    for kind in ("one-sweep", "accelerated", "accelerated one-sweep"):
        s = make(kind, x0, scheme)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = s.run_until(1e-3, 400)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("  %-8s %-21s run_until(1e-3, 400): %3d iterations, %7.3f s wall, converged %s, gap / primal %.3e" % (
            scheme, "ChambollePock" if kind == "one-sweep" else kind, info["iterations"], dt, info["converged"], info["gap"] / info["primal"]), flush=True)
        del s
        torch.cuda.empty_cache()
