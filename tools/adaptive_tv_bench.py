#!/usr/bin/env python3
"""What one iteration of ``AdaptiveTVChambollePock`` costs beside the kernel pair of ``AcceleratedChambollePock`` (``set_fused(False)``), on
one GPU, one process: both loops are a dual kernel on the extrapolated point + tv_cp_primal_accel with the same step schedule; the adaptive
dual epilogue reads one more array (g), so the expectation from traffic alone is (3 Nd + 6) / (3 Nd + 5) of the pair's time.  The data are the
``bench.py`` phantom plus N(0, 10^2) noise (seeded); g = the edge-stopping weights 1 / (1 + (|D x0|_2 / kappa)^2) of the noisy input (upwind
differences, tv_D + tv_l21).  The two loops are timed in turn, three rounds: each figure is the median of its round's 6 iterations, the
smallest round counts, and the spread (max - min) / min of the pair loop's medians over the rounds is printed as the run-to-run yardstick.
Then one ``duality_gap()`` check (tv_dual_gap_wtv, the one-site kernel).
usage: timeout 900 python tools/adaptive_tv_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes
(PYTV4D_LIB=<path> times another build of the library, e.g. one made with TV_VARIANT / TV_EXTRA_FLAGS of pytv-4d_amd/build.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytv-4d_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch, pytv
from pytv import _native as nv
from bench import synth_slab

args = sys.argv[1:]
shape = tuple(int(v) for v in args.pop(0).split("x")) if args and "x" in args[0] else (64, 8, 1024, 1024)
schemes = args or ["upwind", "downwind", "central", "hybrid"]
dev = torch.device("cuda", 0)
LAM, KAPPA, KW = 25.0, 30.0, dict(reg_z_over_reg=1.0, reg_time=1.0)
ROUNDS = 3


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


def edge_weights(x0):
    """``pytv.edge_stopping_weights`` for a 4-D volume with this bench's z / t weights"""
    geo = nv.Geometry(tuple(x0.shape), "upwind", x0.dtype, x0.device, KW["reg_z_over_reg"], KW["reg_time"])
    d = torch.empty(geo.grad_shape, dtype=x0.dtype, device=x0.device)
    g = torch.empty_like(x0)
    st = nv.current_stream(x0.device)
    nv.check(nv.lib().tv_D(geo.ref, nv.ptr(x0), None, None, nv.ptr(d), st))
    nv.check(nv.lib().tv_l21(geo.ref, nv.ptr(d), geo.nd, nv.ptr(g), nv.ptr(geo.scalar()), nv.ptr(geo.workspace()), st))
    del d
    g.div_(KAPPA)
    return torch.reciprocal(g.mul_(g).add_(1.0))


def make(kind, x0, g, scheme):
    if kind == "accel pair":
        s = pytv.solvers.AcceleratedChambollePock(x0, LAM, scheme=scheme, **KW)
        s.set_fused(False)
        return s
    return pytv.solvers.AdaptiveTVChambollePock(x0, LAM, g, scheme=scheme, **KW)


KINDS = ("accel pair", "adaptive")
V = float(np.prod(shape))
x0 = synth_slab(shape, 0, shape[0], dev)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
x0 += 10.0 * torch.randn(x0.shape, dtype=x0.dtype, device=dev, generator=gen)
g = edge_weights(x0)
torch.cuda.empty_cache()
print("== %s fp32 (%.0f Mvox), lambda %g, %r; g = edge-stopping weights of the noisy input, kappa %g: min %.4f mean %.4f max %.4f; library %s" % (
    "x".join(map(str, shape)), V / 1e6, LAM, KW, KAPPA, float(g.min()), float(g.mean()), float(g.max()), os.path.basename(pytv._native.LIB_PATH)), flush=True)
print("   frac = words x 4 bytes x voxels / time / 8 TB/s;  spread = (max - min) / min of the pair loop's medians over %d rounds" % ROUNDS, flush=True)
for scheme in schemes:
    meds = {k: [] for k in KINDS}
    for rep in range(ROUNDS):
        for kind in KINDS:
            s = make(kind, x0, g, scheme)
            nd = s.geo.nd
            meds[kind].append(timed(s.step))
            del s
            torch.cuda.empty_cache()
    best = {k: min(v) for k, v in meds.items()}
    spread = (max(meds["accel pair"]) - min(meds["accel pair"])) / min(meds["accel pair"])
    for kind in KINDS:
        words = 3 * nd + (5 if kind == "accel pair" else 6)
        note = "   spread %.3f" % spread if kind == "accel pair" else "   / accel pair = %.3f  (traffic alone: %.3f)" % (
            best[kind] / best["accel pair"], (3 * nd + 6) / (3 * nd + 5))
        print("  %-8s %-12s %8.3f ms / iteration  (%2d words, frac %.2f)  medians %s%s" % (
            scheme, kind, best[kind], words, words * 4 * V / best[kind] / 1e6 / 8000, " ".join("%.3f" % t for t in meds[kind]), note), flush=True)
    s = make("adaptive", x0, g, scheme)
    s.run(2, record_loss=False)
    t = timed(s.duality_gap, n=3, warm=1)
    print("  %-8s %-12s %8.3f ms / check (tv_dual_gap_wtv, %d words per voxel, one-site kernel; all-reduce and host synchronisation included)" % (
        scheme, "duality_gap()", t, nd + 3), flush=True)
    del s
    torch.cuda.empty_cache()
