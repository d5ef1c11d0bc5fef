#!/usr/bin/env python3
"""Round 6: the persistent small-volume loops (tv_small_cp / tv_small_subgrad_descent, csrc/tv_small.hip) against the ordinary small-volume
path (kernel pair / one-pass kernel per iteration, replayed from hipGraphs) on the reference's own shapes:
  (20,4,100,100)  README.md:76-79;   (1,1,512,512) / (1,1,256,256)  the README loops, 300 iterations (README.md:107-124, 141-157);
  (20,1,100,100)  pytv/tests.py:48.
Round 7 adds the ADMM rows: tv_small_admm (ADMM(persistent=True)) against the ordinary path (ADMM(persistent=False), run(graph=None): hipGraph
replay), n_cg = 10 and 5, rho = 0.05, fp32 and fp64; the yardstick is printed with its spread (max - min of its repetitions).
usage: python tools/small_volume_bench.py [--iters 300] [--schemes a,b] [--solvers CP,SG,ADMM] [NzxMxNyxNx ...]      -> one line per (shape, scheme, solver, path)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytv-4d_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import pytv

ITERS = 300
args = sys.argv[1:]
if "--iters" in args:
    i = args.index("--iters")
    ITERS = int(args[i + 1])
    del args[i:i + 2]
SCHEMES = ("hybrid", "upwind", "central")
if "--schemes" in args:
    i = args.index("--schemes")
    SCHEMES = tuple(args[i + 1].split(","))
    del args[i:i + 2]
SOLVERS = ("CP", "SG", "ADMM")
if "--solvers" in args:
    i = args.index("--solvers")
    SOLVERS = tuple(args[i + 1].split(","))
    del args[i:i + 2]
SHAPES = [tuple(int(v) for v in a.split("x")) for a in args] or [(20, 4, 100, 100), (1, 1, 512, 512), (1, 1, 256, 256), (20, 1, 100, 100), (64, 4, 128, 128)]


def timed_all(make, n, reps=3, warm=4):
    times, loss = [], None
    for _ in range(reps):
        s = make()
        s.run(warm)                   # warm-up of this instance (graph capture, workspace)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = s.run(n)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, loss


def timed(make, n, reps=3):
    times, loss = timed_all(make, n, reps)
    return min(times), loss


for shape in SHAPES:
    rng = np.random.default_rng(0)
    x0 = torch.as_tensor((100.0 * rng.random(shape)).astype(np.float32)).cuda()
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0 if shape[1] > 1 else 0.0)
    for scheme in SCHEMES:
        for name, mk in (("CP", lambda pers: pytv.solvers.ChambollePock(x0, 25.0, scheme=scheme, persistent=pers, **kw)),
                         ("SG", lambda pers: pytv.solvers.SubgradientDescent(x0, 25.0, 5e-3, scheme=scheme, persistent=pers, **kw))):
            if name not in SOLVERS:
                continue
            t_old, l_old = timed(lambda: mk(False), ITERS)
            t_new, l_new = timed(lambda: mk(True), ITERS)
            rel = float(np.max(np.abs(l_new - l_old) / np.abs(l_old)))
            print("%-18s %-8s %s  %d iterations: ordinary path %8.3f ms (%6.2f us/it) | persistent %8.3f ms (%6.2f us/it) | x%.2f | max rel loss diff %.2e"
                  % ("x".join(map(str, shape)), scheme, name, ITERS, 1e3 * t_old, 1e6 * t_old / ITERS, 1e3 * t_new, 1e6 * t_new / ITERS, t_old / t_new, rel), flush=True)
        if "ADMM" not in SOLVERS:
            continue
        for dtype in (torch.float32, torch.float64):
            xd = x0.to(dtype)
            for n_cg in (10, 5):
                mk = lambda pers: pytv.solvers.ADMM(xd, 25.0, 0.05, n_cg=n_cg, scheme=scheme, persistent=pers, **kw)      # noqa: E731
                # warm-up of 12 outer iterations: enough for the ordinary path to go through its capture once (run() captures from 2 + 2 GRAPH_BLOCK on;
                # every run() captures its own graph, so the yardstick contains one capture per 300 outer iterations -- what a caller of run() pays)
                ts_old, l_old = timed_all(lambda: mk(False), ITERS, warm=12)
                ts_new, l_new = timed_all(lambda: mk(True), ITERS, warm=12)
                t_old, t_new, spread = min(ts_old), min(ts_new), max(ts_old) - min(ts_old)
                rel = float(np.max(np.abs(l_new - l_old) / np.abs(l_old)))
                verdict = "pays" if t_old - t_new > spread else "DOES NOT PAY"
                print("%-18s %-8s ADMM n_cg=%-2d %s  %d outer iterations: ordinary path %8.3f ms (%7.2f us/it, spread %6.2f us/it) | persistent %8.3f ms (%7.2f us/it) | x%.2f %s | max rel loss diff %.2e"
                      % ("x".join(map(str, shape)), scheme, n_cg, "f32" if dtype == torch.float32 else "f64", ITERS, 1e3 * t_old, 1e6 * t_old / ITERS,
                         1e6 * spread / ITERS, 1e3 * t_new, 1e6 * t_new / ITERS, t_old / t_new, verdict, rel), flush=True)
