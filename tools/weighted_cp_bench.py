#!/usr/bin/env python3
"""What one iteration of ``WeightedChambollePock`` costs beside ``RobustChambollePock(fidelity="l2")``, on one GPU, one process, on the same
volume: both loops are tv_cp_dual + one D^T pass with a pointwise prox and the extrapolation folded in; the weighted one reads one more array
(w), so the expectation from traffic alone is (3 Nd + 6) / (3 Nd + 5) of the l2 loop's time.  The data is the ``bench.py`` phantom plus
N(0, 10^2) noise (seeded); a third of the sites are unknown (w = 0), the others weighted in [0.25, 2.25]; the box is [0, 255].  The loops are
timed in turn, three rounds: the smallest median counts, and the spread of the l2 loop's medians over the rounds is printed as the run-to-run
yardstick.  Then one ``residuals()`` check.
usage: timeout 900 python tools/weighted_cp_bench.py [NZxMxNYxNX] [scheme ...]      default: 64x8x1024x1024, the four schemes
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
LOWER, UPPER = 0.0, 255.0
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


def make(kind, x0, w, scheme):
    if kind == "l2":
        return pytv.solvers.RobustChambollePock(x0, LAM, fidelity="l2", scheme=scheme, **KW)
    return pytv.solvers.WeightedChambollePock(x0, LAM, w, lower=LOWER, upper=UPPER, scheme=scheme, **KW)


KINDS = ("l2", "weighted")
V = float(np.prod(shape))
torch.manual_seed(0)
x0 = synth_slab(shape, 0, shape[0], dev)
x0 += 10.0 * torch.randn_like(x0)
w = 0.25 + 2.0 * torch.rand_like(x0)
w *= (torch.rand_like(x0) >= 1.0 / 3.0)
x0 *= (w > 0)                                              # unknown sites are zero-filled
print("== %s fp32 (%.0f Mvox), lambda %g, %r, balanced default steps; box [%g, %g]; %.3f of the sites unknown (w = 0), the others w in [0.25, 2.25]; library %s" % (
    "x".join(map(str, shape)), V / 1e6, LAM, KW, LOWER, UPPER, float((w == 0).float().mean()), os.path.basename(pytv._native.LIB_PATH)), flush=True)
print("   frac = words x 4 bytes x voxels / time / 8 TB/s;  spread = (max - min) / min of the l2 loop's medians over %d rounds" % ROUNDS, flush=True)
for scheme in schemes:
    meds = {k: [] for k in KINDS}
    for rep in range(ROUNDS):
        for kind in KINDS:
            s = make(kind, x0, w, scheme)
            nd = s.geo.nd
            meds[kind].append(timed(s.step))
            del s
            torch.cuda.empty_cache()
    best = {k: min(v) for k, v in meds.items()}
    spread = (max(meds["l2"]) - min(meds["l2"])) / min(meds["l2"])
    for kind in KINDS:
        words = 3 * nd + (5 if kind == "l2" else 6)
        note = "   spread %.3f" % spread if kind == "l2" else "   / l2 = %.3f  (traffic alone: %.3f)" % (best[kind] / best["l2"], (3 * nd + 6) / (3 * nd + 5))
        print("  %-8s %-17s %8.3f ms / iteration  (%2d words, frac %.2f)  medians %s%s" % (
            scheme, kind, best[kind], words, words * 4 * V / best[kind] / 1e6 / 8000, " ".join("%.3f" % t for t in meds[kind]), note), flush=True)
    s = make("weighted", x0, w, scheme)
    s.run(2, record_loss=False)
    t = timed(s.residuals, n=3, warm=1)
    print("  %-8s %-17s %8.3f ms / check (tv_cp_dual_residual + residual-mode tv_cp_primal_wls + 1/2 sum w (x - x0)^2 in torch arithmetic, host synchronisation included)" % (
        scheme, "weighted residuals()", t), flush=True)
    del s
    torch.cuda.empty_cache()
