#!/usr/bin/env python3
"""What one iteration of ``PoissonChambollePock`` costs beside ``RobustChambollePock(fidelity="l1")``, on one GPU, one process: both loops are
tv_cp_dual + one D^T pass with a pointwise prox and the extrapolation folded in, 3 Nd + 5 words per voxel, so the expectation is parity --
unless the square root, the division and the logarithm of the Kullback-Leibler step show through the memory traffic.  The data are Poisson
counts of the ``bench.py`` phantom (seeded).  The loops are timed in turn, twice; the smaller median counts.  Then one ``residuals()`` check.
usage: timeout 900 python tools/poisson_cp_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes
(PYTV4D_LIB=<path> times another build of the library, e.g. one made with TV_VARIANT / TV_EXTRA_FLAGS of pytv-4d_amd/build.py)"""
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
TAU = 5.0


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
    if kind == "l1":
        return pytv.solvers.RobustChambollePock(x0, LAM, fidelity="l1", scheme=scheme, tau=TAU, **KW)
    return pytv.solvers.PoissonChambollePock(x0, LAM, scheme=scheme, tau=TAU, **KW)


KINDS = ("l1", "poisson")
V = float(np.prod(shape))
phantom = synth_slab(shape, 0, shape[0], dev)
torch.manual_seed(0)
x0 = torch.poisson(phantom.clamp_(min=0.0))                # counts with the phantom as their mean
del phantom
print("== %s fp32 (%.0f Mvox), lambda %g, %r, tau %g; counts: min %g max %g mean %.2f, %.3f of the sites at 0; library %s" % (
    "x".join(map(str, shape)), V / 1e6, LAM, KW, TAU, float(x0.min()), float(x0.max()), float(x0.mean()), float((x0 == 0).float().mean()),
    os.path.basename(pytv._native.LIB_PATH)), flush=True)
print("   frac = words x 4 bytes x voxels / time / 8 TB/s", flush=True)
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
        note = "" if kind == "l1" else "   / l1 = %.3f" % (best[kind] / best["l1"])
        print("  %-8s %-17s %8.3f ms / iteration  (%2d words, frac %.2f)%s" % (scheme, kind, best[kind], words, words * 4 * V / best[kind] / 1e6 / 8000,
                                                                             note), flush=True)
    s = make("poisson", x0, scheme)
    s.run(2, record_loss=False)
    t = timed(s.residuals, n=3, warm=1)
    print("  %-8s %-17s %8.3f ms / check (tv_cp_dual_residual + residual-mode tv_cp_primal_kl + F(x) in fp64 torch arithmetic, host synchronisation included)" % (
        scheme, "poisson residuals()", t), flush=True)
    del s
    torch.cuda.empty_cache()
