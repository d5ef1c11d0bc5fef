#!/usr/bin/env python3
"""What one iteration of ``RobustChambollePock`` costs beside the kernel pair of ``AcceleratedChambollePock`` (``set_fused(False)``), on one
GPU, one process: both loops are tv_cp_dual + one D^T pass with a pointwise prox and the extrapolation folded in, 3 Nd + 5 words per voxel,
so the expectation is parity.  The loops are timed in turn, twice; the smaller median counts.  Then one ``residuals()`` check.
usage: timeout 900 python tools/robust_cp_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytv-4d_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch, pytv
from bench import synth_slab

args = sys.argv[1:]
shape = tuple(int(v) for v in args.pop(0).split("x")) if args and "x" in args[0] else (64, 8, 1024, 1024)
schemes = args or ["upwind", "downwind", "central", "hybrid"]
dev = torch.device("cuda", 0)
LAM, KW = 25.0, dict(reg_z_over_reg=1.0, reg_time=1.0)
TAU, DELTA = 5.0, 2.0


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
    if kind == "accelerated pair":
        s = pytv.solvers.AcceleratedChambollePock(x0, LAM, scheme=scheme, **KW)
        s.set_fused(False)
        return s
    return pytv.solvers.RobustChambollePock(x0, LAM, fidelity=kind, delta=DELTA if kind == "huber" else None, scheme=scheme, tau=TAU, **KW)


KINDS = ("accelerated pair", "l1", "huber")
V = float(np.prod(shape))
x0 = synth_slab(shape, 0, shape[0], dev)
print("== %s fp32 (%.0f Mvox), lambda %g, %r, robust tau %g delta %g; frac = words x 4 bytes x voxels / time / 8 TB/s" % (
    "x".join(map(str, shape)), V / 1e6, LAM, KW, TAU, DELTA), flush=True)
for scheme in schemes:
    best = {}
    for rep in range(2):
        for kind in KINDS:
            s = make(kind, x0, scheme)
            words = 3 * s.geo.nd + 5
            t = timed(s.step)
            best[kind] = min(best.get(kind, t), t)
            del s
            torch.cuda.empty_cache()
    for kind in KINDS:
        note = "" if kind == "accelerated pair" else "   / accelerated pair = %.3f" % (best[kind] / best["accelerated pair"])
        print("  %-8s %-17s %8.3f ms / iteration  (%2d words, frac %.2f)%s" % (scheme, kind, best[kind], words, words * 4 * V / best[kind] / 1e6 / 8000,
                                                                             note), flush=True)
    s = make("l1", x0, scheme)
    s.run(2, record_loss=False)
    t = timed(s.residuals, n=3, warm=1)
    print("  %-8s %-17s %8.3f ms / check (tv_cp_dual_residual + residual-mode tv_cp_primal_prox + F(x - x0), host synchronisation included)" % (
        scheme, "l1 residuals()", t), flush=True)
    del s
    torch.cuda.empty_cache()
