#!/usr/bin/env python3
"""What one iteration of ``VectorialTVChambollePock`` costs beside the kernel pair of ``AcceleratedChambollePock`` (``set_fused(False)``), on
one GPU, one process: both loops are a dual kernel on the extrapolated point + tv_cp_primal_accel with the same step schedule; only the dual
kernel differs (tv_cp_dual_vtv: a thread owns a spatial site and walks its frames).  The yardstick is traffic: the REGISTER form (up to 8
frames, hybrid 4) moves the pair's 3 Nd + 5 words per voxel, so its ratio to the pair should be near 1; the GENERIC form rereads q and x_bar
in its second pass, at most (4 Nd + 6) / (3 Nd + 5) if nothing hits in a cache.  Three fp32 volumes of (nearly) equal voxel count: 16, 8
and 3 frames.  Where the register form is the default the generic form is timed as well, forced with TV_VTV_FORM = 2: what the cut-over
buys.  The data are the ``bench.py`` phantom plus N(0, 10^2) noise (seeded).  The loops are timed in turn, three rounds: each figure is the
median of its round's 6 iterations, the smallest round counts, and the spread (max - min) / min of the pair loop's medians over the rounds is
printed as the run-to-run yardstick.  Then one ``duality_gap()`` check (tv_dual_gap_vtv).
usage: timeout 900 python tools/vectorial_tv_bench.py [NZxMxNYxNX ...] [scheme ...]      default: 32x16x1024x1024 64x8x1024x1024 170x3x1024x1024, four schemes
(PYTV4D_LIB=<path> times another build of the library, e.g. one made with TV_VARIANT / TV_EXTRA_FLAGS of pytv-4d_amd/build.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytv-4d_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch, pytv
from pytv import _native as nv
from bench import synth_slab

args = sys.argv[1:]
shapes = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a] or [(32, 16, 1024, 1024), (64, 8, 1024, 1024), (170, 3, 1024, 1024)]
schemes = [a for a in args if "x" not in a] or ["upwind", "downwind", "central", "hybrid"]
dev = torch.device("cuda", 0)
LAM, KW = 25.0, dict(reg_z_over_reg=1.0, reg_time=1.0)
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


def make(kind, x0, scheme):
    """(solver, the TV_VTV_FORM it runs under)"""
    if kind == "accel pair":
        s = pytv.solvers.AcceleratedChambollePock(x0, LAM, scheme=scheme, **KW)
        s.set_fused(False)
        return s, 0
    return pytv.solvers.VectorialTVChambollePock(x0, LAM, scheme=scheme, **KW), (2 if kind == "vtv generic" else 0)


def register_form(scheme, m):
    """the rule of csrc/tv_vtv.hip (vtv_reg_form)"""
    return 1 <= m <= (4 if scheme == "hybrid" else 8)


print("library %s;  frac = words x 4 bytes x voxels / time / 8 TB/s;  spread = (max - min) / min of the pair loop's medians over %d rounds" % (
    os.path.basename(pytv._native.LIB_PATH), ROUNDS), flush=True)
for shape in shapes:
    V = float(np.prod(shape))
    x0 = synth_slab(shape, 0, shape[0], dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    x0 += 10.0 * torch.randn(x0.shape, dtype=x0.dtype, device=dev, generator=gen)
    print("== %s fp32 (%.0f Mvox), lambda %g, %r" % ("x".join(map(str, shape)), V / 1e6, LAM, KW), flush=True)
    for scheme in schemes:
        reg = register_form(scheme, shape[1])
        kinds = ("accel pair", "vtv default") + (("vtv generic",) if reg else ())
        meds = {k: [] for k in kinds}
        for rep in range(ROUNDS):
            for kind in kinds:
                s, form = make(kind, x0, scheme)
                nd = s.geo.nd
                nv.set_option("TV_VTV_FORM", form)
                meds[kind].append(timed(s.step))
                nv.set_option("TV_VTV_FORM", None)
                del s
                torch.cuda.empty_cache()
        best = {k: min(v) for k, v in meds.items()}
        spread = (max(meds["accel pair"]) - min(meds["accel pair"])) / min(meds["accel pair"])
        for kind in kinds:
            generic = kind == "vtv generic" or (kind == "vtv default" and not reg)
            words = 4 * nd + 6 if generic else 3 * nd + 5
            if kind == "accel pair":
                note = "   spread %.3f" % spread
            else:
                note = "   %s form / accel pair = %.3f  (traffic alone: %s %.3f)" % (
                    "generic" if generic else "register", best[kind] / best["accel pair"], "at most" if generic else "", words / (3 * nd + 5))
            print("  %-8s %-12s %8.3f ms / iteration  (%2d words%s, frac %.2f)  medians %s%s" % (
                scheme, kind, best[kind], words, " at most" if generic else "", words * 4 * V / best[kind] / 1e6 / 8000,
                " ".join("%.3f" % t for t in meds[kind]), note), flush=True)
        s, _ = make("vtv default", x0, scheme)
        s.run(2, record_loss=False)
        t = timed(s.duality_gap, n=3, warm=1)
        print("  %-8s %-12s %8.3f ms / check (tv_dual_gap_vtv, %d words per voxel; all-reduce and host synchronisation included)" % (
            scheme, "duality_gap()", t, nd + 2), flush=True)
        del s
        torch.cuda.empty_cache()
    del x0
    torch.cuda.empty_cache()
