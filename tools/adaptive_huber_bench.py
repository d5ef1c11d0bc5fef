#!/usr/bin/env python3
"""What one iteration of ``AdaptiveHuberChambollePock`` costs on its two paths beside the one-sweep path of ``HuberChambollePock``, on one GPU,
one process.  Three loops:
    (a) huber sweep      tv_cp_huber_sweep + tv_cp_accel_fixup, 2 Nd + 5 words per voxel: the yardstick
    (b) adaptive sweep   tv_cp_hwtv_sweep  + tv_cp_accel_fixup, 2 Nd + 6 (g is one more streamed array)
    (c) adaptive pair    tv_cp_dual_hwtv   + tv_cp_primal_accel, 3 Nd + 6
The data are the ``bench.py`` phantom plus N(0, 10^2) noise (seeded); g = the edge-stopping weights 1 / (1 + (|D x0|_2 / kappa)^2) of the
noisy input (tools/adaptive_tv_bench.py).  The loops are timed in turn, three rounds: each figure is the median of its round's 6
iterations, the smallest round counts, and a loop's spread is (max - min) / min of its medians over the rounds.  Per scheme: (b) / (a)
beside (2 Nd + 6) / (2 Nd + 5), (b) / (c) beside (2 Nd + 6) / (3 Nd + 6), and the verdict of the default rule -- a scheme may default to
the sweep only where (b) is faster than (c) by more than (c)'s spread (``AdaptiveHuberChambollePock.SWEEP_DEFAULT_SCHEMES``).
usage: timeout 900 python tools/adaptive_huber_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes
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
LAM, ALPHA, KAPPA, KW = 25.0, 2.0, 30.0, dict(reg_z_over_reg=1.0, reg_time=1.0)
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
    if kind == "huber sweep":
        s = pytv.solvers.HuberChambollePock(x0, LAM, ALPHA, scheme=scheme, **KW)
    else:
        s = pytv.solvers.AdaptiveHuberChambollePock(x0, LAM, g, ALPHA, scheme=scheme, **KW)
    s.set_fused(kind.endswith("sweep"))
    return s


KINDS = ("huber sweep", "adaptive sweep", "adaptive pair")
V = float(np.prod(shape))
x0 = synth_slab(shape, 0, shape[0], dev)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
x0 += 10.0 * torch.randn(x0.shape, dtype=x0.dtype, device=dev, generator=gen)
g = edge_weights(x0)
torch.cuda.empty_cache()
print("== %s fp32 (%.0f Mvox), lambda %g, alpha %g, %r; g = edge-stopping weights of the noisy input, kappa %g: min %.4f mean %.4f max %.4f; library %s" % (
    "x".join(map(str, shape)), V / 1e6, LAM, ALPHA, KW, KAPPA, float(g.min()), float(g.mean()), float(g.max()), os.path.basename(pytv._native.LIB_PATH)),
    flush=True)
print("   frac = words x 4 bytes x voxels / time / 8 TB/s;  spread = (max - min) / min of a loop's medians over %d rounds" % ROUNDS, flush=True)
for scheme in schemes:
    meds = {k: [] for k in KINDS}
    for rep in range(ROUNDS):
        for kind in KINDS:
            s = make(kind, x0, g, scheme)
            assert s.fused is kind.endswith("sweep")
            nd = s.geo.nd
            meds[kind].append(timed(s.step))
            del s
            torch.cuda.empty_cache()
    best = {k: min(v) for k, v in meds.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in meds.items()}
    words = {"huber sweep": 2 * nd + 5, "adaptive sweep": 2 * nd + 6, "adaptive pair": 3 * nd + 6}
    for kind in KINDS:
        print("  %-8s %-14s %8.3f ms / iteration  (%2d words, frac %.2f)  medians %s  spread %.3f" % (
            scheme, kind, best[kind], words[kind], words[kind] * 4 * V / best[kind] / 1e6 / 8000, " ".join("%.3f" % t for t in meds[kind]),
            spread[kind]), flush=True)
    ba, bc = best["adaptive sweep"] / best["huber sweep"], best["adaptive sweep"] / best["adaptive pair"]
    sweep_wins = best["adaptive sweep"] < best["adaptive pair"] * (1.0 - spread["adaptive pair"])
    print("  %-8s (b)/(a) = %.3f  (traffic alone: %.3f)   (b)/(c) = %.3f  (traffic alone: %.3f)   default: %s" % (
        scheme, ba, (2 * nd + 6) / (2 * nd + 5), bc, (2 * nd + 6) / (3 * nd + 6),
        "the sweep ((b) faster than (c) by more than (c)'s spread %.3f)" % spread["adaptive pair"] if sweep_wins else
        "the pair ((b) not faster than (c) by more than (c)'s spread %.3f)" % spread["adaptive pair"]), flush=True)
