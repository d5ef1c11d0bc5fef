#!/usr/bin/env python3
"""What one iteration of ``HuberChambollePock`` costs on its two paths, beside the two paths of ``AcceleratedChambollePock``, on one GPU, one
process.  The kernel pairs are a dual kernel on the extrapolated point + tv_cp_primal_accel, 3 Nd + 5 words per voxel; the one-sweep paths
are tv_cp_huber_sweep / tv_cp_accel_sweep + tv_cp_accel_fixup, 2 Nd + 5 words (+ the fix-up's).  The Huber dual update adds one multiply per
channel and a clamped quadratic per column to either form.  The data are the ``bench.py`` phantom plus N(0, 10^2) noise (seeded).  The four
loops are timed in turn (interleaved), three rounds; each figure is the median of its round's iterations, the smallest round counts and
the spread over the rounds is printed.  Per scheme the two ratios DESIGN.md section 3.7 asks about: Huber sweep / Huber pair (< 1: the sweep
is the default on large volumes) and Huber sweep / accelerated sweep (the same words: within the 8 % box spread).  Then one
``duality_gap()`` check (tv_dual_gap_huber, the one-site kernel).
usage: timeout 900 python tools/huber_cp_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes
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
LAM, ALPHA, KW = 25.0, 2.0, dict(reg_z_over_reg=1.0, reg_time=1.0)
ROUNDS = 3


def timed(fn, n=10, warm=3):
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
    fused = kind.endswith("sweep")
    if kind.startswith("accel"):
        s = pytv.solvers.AcceleratedChambollePock(x0, LAM, scheme=scheme, **KW)
        s.set_fused(fused)
        return s
    s = pytv.solvers.HuberChambollePock(x0, LAM, ALPHA, scheme=scheme, **KW)
    s.set_fused(fused)
    return s


KINDS = ("huber pair", "huber sweep", "accel pair", "accel sweep")
V = float(np.prod(shape))
x0 = synth_slab(shape, 0, shape[0], dev)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
x0 += 10.0 * torch.randn(x0.shape, dtype=x0.dtype, device=dev, generator=gen)
print("== %s fp32 (%.0f Mvox), lambda %g, alpha %g, %r; library %s" % ("x".join(map(str, shape)), V / 1e6, LAM, ALPHA, KW,
                                                                      os.path.basename(pytv._native.LIB_PATH)), flush=True)
print("   frac = words x 4 bytes x voxels / time / 8 TB/s", flush=True)
for scheme in schemes:
    ts = {k: [] for k in KINDS}
    words = {}
    for rep in range(ROUNDS):
        for kind in KINDS:
            s = make(kind, x0, scheme)
            assert s.fused is kind.endswith("sweep")
            words[kind] = (2 if s.fused else 3) * s.geo.nd + 5
            ts[kind].append(timed(s.step))
            del s
            torch.cuda.empty_cache()
    best = {k: min(v) for k, v in ts.items()}
    for kind in KINDS:
        note = ""
        if kind == "huber sweep":
            note = "   / huber pair = %.3f   / accel sweep = %.3f" % (best[kind] / best["huber pair"], best[kind] / best["accel sweep"])
        elif kind == "accel sweep":
            note = "   / accel pair = %.3f" % (best[kind] / best["accel pair"])
        print("  %-8s %-12s %8.3f ms / iteration  (rounds %s; %2d words, frac %.2f)%s" % (
            scheme, kind, best[kind], " ".join("%.3f" % t for t in ts[kind]), words[kind], words[kind] * 4 * V / best[kind] / 1e6 / 8000, note),
            flush=True)
    s = make("huber pair", x0, scheme)
    s.run(2, record_loss=False)
    t = timed(s.duality_gap, n=3, warm=1)
    print("  %-8s %-12s %8.3f ms / check (tv_dual_gap_huber, %d words per voxel, one-site kernel; all-reduce and host synchronisation included)" % (
        scheme, "duality_gap()", t, s.geo.nd + 2), flush=True)
    del s
    torch.cuda.empty_cache()
