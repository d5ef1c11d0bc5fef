"""Thin and uneven z-slabs through the Python layer that does the sharding (pytv/slab.py, ``_SlabProblem`` and every solver of
pytv/solvers.py), with the harness of tests/test_gpu_multirank.py: 2 - 4 processes share cuda:0 and talk over gloo.  The kernels see
one-plane z-ranges through the C-ABI elsewhere (tests/test_gpu_parity.py, tests/test_gpu_sweep_ranges.py); here the SOLVERS see ranks of
one plane, partitions with a remainder, ranks that sit exactly on an overlap threshold beside a rank below it (two schedules in one job:
``ChambollePock.overlap`` / ``overlap_fused`` at 3 planes, ``SubgradientDescent.overlap`` and ADMM's normal operator at 5), and ranks
that disagree about the chunks of the one-sweep kernel.

Expected values are fp64 runs on the UNSHARDED volume: ``orc.chambolle_pock`` / ``orc.admm`` / ``orc.subgradient_descent``, and for the
eight extrapolated Chambolle-Pock solvers (``AcceleratedChambollePock``, ``HuberChambollePock``, ``AdaptiveTVChambollePock``,
``AdaptiveHuberChambollePock``, ``VectorialTVChambollePock``, ``RobustChambollePock``, ``PoissonChambollePock``, ``WeightedChambollePock``:
twelve solver classes in all) the NumPy restatements of their own test files (imported, not copied).  Each rank's result is compared
with ``slab.local`` of it, the loss history and the certificate (``duality_gap()`` / ``residuals()``) with the global value.

Tolerances are those the project states already:
  ChambollePock, SubgradientDescent   fp32: loss rtol 1e-5, x rtol 1e-5 atol 2e-3 (tests/test_gpu_multirank.py)
                                      fp64: loss rtol 1e-10, x rtol 1e-10 atol 1e-9 (tests/test_gpu_parity.py, the fp64 Chambolle-Pock loops)
  ADMM                                fp32: loss rtol 1e-6, x rtol 2e-6 atol 2e-4 (tests/test_gpu_multirank.py)
                                      fp64: loss rtol 1e-9, x rtol 1e-9 atol 1e-8 (tests/test_gpu_weight_volume.py)
  ChambollePockOperator               fp32: loss rtol 2e-5, x rtol 1e-4 atol 2e-3 (tests/test_gpu_multirank.py); fp64 as ChambollePock
  the extrapolated solvers            fp64: loss rtol 1e-10, max|dx| <= 1e-9 max|x0|; fp32: loss rtol 1e-5 (Poisson / weighted: the ``ltol`` of
                                      their ``np_trajectory``), x rtol 1e-5 atol 2e-3 (tests/test_gpu_cp_accel.py and the files after it)
  certificates                        primal and gap to R * primal, R = 1e-10 in fp64 (``run_until`` of tests/test_gpu_cp_huber.py) and the
                                      project's fp32 rtol 1e-5 on that scale; residuals in fp64 to rtol 1e-9 plus the rounding floor their
                                      restatement returns (tests/test_gpu_cp_prox.py, _kl.py, _wls.py)
"""
import datetime
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT, SCHEMES
from test_gpu_cp_prox_multirank import _free_port

pytestmark = pytest.mark.gpu

JOB_LIMIT_S = 120          # a spawned job that is not done by then is ended and fails its test (a healthy one takes a few seconds)

# (nz_global, world) -> planes per rank
PARTITIONS = {(3, 3): (1, 1, 1), (4, 3): (2, 1, 1), (5, 4): (2, 1, 1, 1), (8, 3): (3, 3, 2), (7, 2): (4, 3), (9, 2): (5, 4),
              (6, 4): (2, 2, 1, 1)}
ONE_PLANE = [k for k, v in PARTITIONS.items() if min(v) < 2]
SWEEP_FRAME, SITE_FRAME, SEAM_FRAME = (3, 10, 64), (2, 8, 12), (9, 5, 68)   # one-sweep eligible, Ny ragged / one-site kernels / time-window seam
CASES = [(nzg, w, SWEEP_FRAME, "float32") for nzg, w in PARTITIONS] + [(nzg, w, SWEEP_FRAME, "float64") for nzg, w in PARTITIONS] \
    + [(nzg, w, SITE_FRAME, "float64") for nzg, w in PARTITIONS] + [(8, 3, SEAM_FRAME, "float64"), (3, 3, SEAM_FRAME, "float64")]
TWO = ("hybrid", "upwind")             # the schemes of every solver but ChambollePock (which runs all four)
KW = dict(reg_z_over_reg=1.3, reg_time=0.7)          # tests/test_gpu_multirank.py
XKW = dict(reg_z_over_reg=0.7, reg_time=0.25)        # the ``_kw_of`` of the extrapolated solvers' test files
N_IT = 6


# ------------------------------------------------------------------------------------------------
# the ranks
# ------------------------------------------------------------------------------------------------
def _worker(rank, world, port, nzg, dtype_name, jobs, ret):
    """Every job: build the solver on this rank's slab, run it, return the iterate, the loss history, the certificate, the iteration
    ``run_until`` stopped at and the attributes that say which path ran.  A 4-D array whose axis 0 is the global z axis is cut with
    ``slab.local`` wherever it appears among a job's arguments."""
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=JOB_LIMIT_S // 2))
    try:
        import pytv
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(nzg)
        tdt = getattr(torch, dtype_name)

        def is_volume(v):
            return isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg

        def local(a):
            t = torch.as_tensor(np.ascontiguousarray(slab.local(a)))
            return (t if t.dtype == torch.bool else t.to(tdt)).cuda()

        out = {"z": (slab.z0, slab.nz)}
        for job in jobs:
            def build():
                x0 = local(job["x0"])
                # (a per-voxel time weight goes in as a host array of this rank's slab shape, as in tests/test_gpu_weight_volume.py)
                kw = {k: (np.ascontiguousarray(slab.local(v)) if k == "mask_static" else local(v)) if is_volume(v) else v
                      for k, v in job["kw"].items()}
                args = [local(v) if is_volume(v) else v for v in job["args"]]
                cls = getattr(pytv.solvers, job["cls"])
                if job["cls"] == "ChambollePockOperator":
                    return cls(lambda v: v.clone(), lambda v: v.clone(), x0.clone(), x0, *args, slab=slab, **kw)
                return cls(x0, *args, slab=slab, **kw)

            s = build()
            res = {}
            if job.get("one_sweep_refused"):
                # the extrapolated solvers have no sweep / exchange / fix-up schedule for slabs: the default is the kernel pair and
                # asking for the one-sweep kernel is an error, on every rank alike
                assert s.fused is False
                with pytest.raises(ValueError, match=job["one_sweep_refused"]):
                    s.set_fused(True)
                assert s.fused is False
            res["attrs"] = {a: getattr(s, a) for a in ("fused", "overlap", "overlap_fused", "nchunks", "zchunk", "one_pass", "cheb", "small")
                            if isinstance(getattr(s, a, None), (bool, int))}
            if job["cls"] == "ADMM":
                res["attrs"]["overlap"] = bool(s.sh and slab.nz >= 5)          # the rule of ADMM._normal / _cheb_step (no attribute holds it)
            res["loss"] = np.asarray(s.run(job["n"]), dtype=np.float64)
            res["x"] = s.result().cpu().numpy()
            if job.get("cert") == "gap":
                res["cert"] = tuple(s.duality_gap())
            elif job.get("cert") == "res":
                res["cert"] = dict(s.residuals())
                res["r0"] = s.initial_residual()
            if hasattr(s, "g_max"):
                res["g_max"] = s.g_max            # AdaptiveHuberChambollePock: the maximum of g its steps were computed from
            if job.get("until") is not None:
                t = build()
                loss, info = t.run_until(*job["until"])
                res["until"] = (int(info["iterations"]), bool(info["converged"]), len(loss))
            out[job["key"]] = res
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def _spawn(world, nzg, dtype_name, jobs):
    """the ranks of one job under ``JOB_LIMIT_S``: a rank that raises ends the others (``ProcessContext.join``), a job that hangs is ended"""
    assert world <= 4
    ret = mp.Manager().dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), nzg, dtype_name, jobs, ret), nprocs=world, join=False)
    deadline = time.monotonic() + JOB_LIMIT_S
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a %d-rank job was not done after %d s" % (world, JOB_LIMIT_S))
    assert len(ret) == world
    return [ret[r] for r in range(world)]


# ------------------------------------------------------------------------------------------------
# the problems and their fp64 expectations on the unsharded volume
# ------------------------------------------------------------------------------------------------
def _uniform(shape):
    """the data of tests/test_gpu_multirank.py: 60 * default_rng(91).random, rounded to fp32 (both precisions see the same numbers)"""
    return (60.0 * np.random.default_rng(91).random(shape)).astype(np.float32).astype(np.float64)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _gap_count(states, rel_gap, every, max_iter):
    """the iteration ``run_until`` stops at, from the fp64 (primal, gap) after ``every``, ``2 every``, ... iterations"""
    done = 0
    for primal, gap in states:
        done += every
        if gap <= rel_gap * primal or done >= max_iter:
            return done
    raise AssertionError("not enough states")


def _plan(shape, dtype_name, sizes):
    """(jobs, checks): what the ranks run and, per job key, what the result must be: dict(x, loss, kind, [ltol], [cert], [until])"""
    from oracle import tv_oracle as orc
    import test_gpu_cp_accel as t_acc
    import test_gpu_cp_huber as t_hub
    import test_gpu_cp_kl as t_kl
    import test_gpu_cp_prox as t_prox
    import test_gpu_cp_wls as t_wls
    import test_gpu_cp_wtv as t_wtv
    import test_cp_vtv_inputs as t_vin
    import test_gpu_cp_hwtv_sweep as t_hwtv        # (the restatement and certificate that tests/test_gpu_cp_hwtv.py imports from there)
    import test_gpu_cp_vtv as t_vtv
    from test_gpu_dual_gap import ref_gap
    f32 = dtype_name == "float32"
    sweep_ok = shape[3] >= 64 and shape[3] % (4 if f32 else 2) == 0      # tv_cp_fused_supported: whole 16-byte lanes, Nx >= 64, either precision
    thin = min(sizes) < 2
    refusal = "takes unsharded volumes only" if sweep_ok else "does not support this geometry"       # what ``set_fused(True)`` says on a slab
    jobs, checks = [], {}

    def add(key, cls, x0, args, kw, n, want, **more):
        job = dict(key=key, cls=cls, x0=x0, args=list(args), kw=kw, n=n)
        job.update({k: more.pop(k) for k in ("cert", "until", "one_sweep_refused") if k in more})
        jobs.append(job)
        checks[key] = dict(want, **more)

    # ---- a. ChambollePock: kernel pair and one-sweep, overlap on and off, and the library's default; c. the operator slot; e. a weight volume
    x0 = _uniform(shape)
    W = np.random.default_rng(77).random(shape) * 2.0
    for scheme in SCHEMES:
        wx, wloss, _, wq = orc.chambolle_pock(x0, N_IT, 7.0, scheme=scheme, return_state=True, **KW)
        tv, fid, gap = ref_gap(wx, wq, x0, 7.0, 1.0, scheme, KW)
        want = dict(x=wx, loss=wloss, kind="cp", cert=(fid + 7.0 * tv, gap))
        ways = [("pair", dict(fused=False, overlap=True)), ("pair_serial", dict(fused=False, overlap=False)), ("default", dict())]
        if sweep_ok:
            ways += [("sweep", dict(fused=True, overlap=True)), ("sweep_serial", dict(fused=True, overlap=False))]
        for way, how in ways:
            more = {}
            if scheme == "hybrid" and way in ("pair", "sweep"):
                states = []
                for n in (2, 4, 6):
                    sx, _, _, sq = orc.chambolle_pock(x0, n, 7.0, scheme=scheme, return_state=True, **KW)
                    stv, sfid, sgap = ref_gap(sx, sq, x0, 7.0, 1.0, scheme, KW)
                    states.append((sfid + 7.0 * stv, sgap))
                rel = float(np.sqrt((states[0][1] / states[0][0]) * (states[1][1] / states[1][0])))   # between the 2nd and the 4th iteration's
                more = dict(until=(rel, 6, 2), until_want=_gap_count(states, rel, 2, 6))
            add("cp_%s_%s" % (way, scheme), "ChambollePock", x0, (7.0,), dict(KW, scheme=scheme, **how), N_IT, want, cert="gap", **more)
        if len(sizes) == 3 and scheme in TWO and sizes in ((2, 1, 1), (3, 3, 2)):
            add("op_%s" % scheme, "ChambollePockOperator", x0, (7.0,), dict(KW, scheme=scheme), N_IT, dict(x=wx, loss=wloss, kind="op"))
        if sizes == (2, 1, 1) and scheme in TWO:
            vx, vloss = orc.chambolle_pock(x0, N_IT, 7.0, scheme=scheme, mask_static=W, **KW)
            for way, how in [("pair", dict(fused=False))] + ([("sweep", dict(fused=True))] if sweep_ok else []):
                add("cpw_%s_%s" % (way, scheme), "ChambollePock", x0, (7.0,), dict(KW, scheme=scheme, mask_static=W, **how), N_IT,
                    dict(x=vx, loss=vloss, kind="cp"))

    # ---- a. the eight extrapolated solvers (kernel pair on a slab)
    for scheme in TWO:
        # AcceleratedChambollePock
        d = _f32(t_acc.square_plus_noise(shape))
        wx, wloss, wq = t_acc.np_accel(d, N_IT, 25.0, scheme, XKW, want_q=True)
        states = []
        for n in (2, 4, 6):
            sx, _, sq = t_acc.np_accel(d, n, 25.0, scheme, XKW, want_q=True)
            states.append(t_acc.np_gap(sx, sq, d, 25.0, scheme, XKW))
        rel = float(np.sqrt((states[0][1] / states[0][0]) * (states[1][1] / states[1][0])))
        add("accel_%s" % scheme, "AcceleratedChambollePock", d, (25.0,), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", cert=states[2], scale=float(np.max(np.abs(d)))), cert="gap", one_sweep_refused=refusal,
            until=(rel, 6, 2), until_want=_gap_count(states, rel, 2, 6))
        # HuberChambollePock
        d = _f32(t_hub.noisy_square(shape))
        wx, wloss, (_, _, wq) = t_hub.np_huber_cp(d, N_IT, t_hub.REG, 2.0, scheme, XKW)
        states = []
        for n in (2, 4, 6):
            sx, _, (_, _, sq) = t_hub.np_huber_cp(d, n, t_hub.REG, 2.0, scheme, XKW)
            states.append(t_hub.np_huber_gap(sx, sq, d, t_hub.REG, 2.0, scheme, XKW))
        rel = float(np.sqrt((states[0][1] / states[0][0]) * (states[1][1] / states[1][0])))
        add("huber_%s" % scheme, "HuberChambollePock", d, (t_hub.REG, 2.0), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", cert=states[2], scale=float(np.max(np.abs(d)))), cert="gap", one_sweep_refused=refusal,
            until=(rel, 6, 2), until_want=_gap_count(states, rel, 2, 6))
        # AdaptiveTVChambollePock
        g = t_wtv.make_g(shape, np.float32).astype(np.float64)
        wx, wloss, (_, _, wq, _, _) = t_wtv.np_adaptive(d, N_IT, t_wtv.REG, g, scheme, XKW)
        wtv, fid, gap, _ = t_wtv.ref_gap(wx, wq, d, g, t_wtv.REG, scheme, XKW)
        add("wtv_%s" % scheme, "AdaptiveTVChambollePock", d, (t_wtv.REG, g), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", cert=(fid + t_wtv.REG * wtv, gap), scale=float(np.max(np.abs(d)))), cert="gap",
            until=(1e-3, 4, 2), until_want=None)
        # AdaptiveHuberChambollePock: the same data and weight map; its steps come from the maximum of g over ALL ranks
        wx, wloss, wq = t_hwtv.np_hwtv_cp(d, g, N_IT, t_hub.REG, 2.0, scheme, XKW)
        hub, fid, gap, _ = t_hwtv.np_gap_hwtv(wx, wq, d, g, t_hub.REG, 2.0, scheme, XKW)
        add("hwtv_%s" % scheme, "AdaptiveHuberChambollePock", d, (t_hub.REG, g, 2.0), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", cert=(fid + t_hub.REG * hub, gap), scale=float(np.max(np.abs(d))), g_max=float(g.max())),
            cert="gap", one_sweep_refused=refusal, until=(1e-3, 4, 2), until_want=None)
        # VectorialTVChambollePock: it has no one-sweep path on any geometry, and says so before it looks at the slab
        d = _f32(t_vtv.coupled_square(shape))
        states, state, wloss = [], None, []
        for n in (2, 2, 2):
            wx, part, state = t_vin.np_vectorial(d, n, t_vtv.REG, scheme, XKW, state=state)
            wloss.append(part)
            vtv, fid, gap, _ = t_vin.ref_gap(state[0], state[2], d, t_vtv.REG, scheme, XKW)
            states.append((fid + t_vtv.REG * vtv, gap))
        rel = float(np.sqrt((states[0][1] / states[0][0]) * (states[1][1] / states[1][0])))
        add("vtv_%s" % scheme, "VectorialTVChambollePock", d, (t_vtv.REG,), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=np.concatenate(wloss), kind="xcp", cert=states[2], scale=float(np.max(np.abs(d)))), cert="gap",
            one_sweep_refused="VectorialTVChambollePock has no one-sweep path", until=(rel, 6, 2), until_want=_gap_count(states, rel, 2, 6))
        # RobustChambollePock("l1")
        d = np.asarray(t_prox.square_with_impulses(shape))
        tau = t_prox.TAU_S
        sigma = 1.0 / (orc.normal_spectral_bound(scheme, shape, **XKW) * tau)
        wx, wloss, wq = t_prox.np_robust(d, N_IT, t_prox.REG, "l1", t_prox.DELTA_S, scheme, XKW, tau, sigma)
        wres = t_prox.np_residuals(wx, wq, d, t_prox.REG, "l1", t_prox.DELTA_S, scheme, XKW, tau, sigma)
        add("l1_%s" % scheme, "RobustChambollePock", d, (t_prox.REG,), dict(XKW, scheme=scheme, fidelity="l1", tau=tau), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", cert=(wres, 0.0), scale=float(np.max(np.abs(d)))), cert="res", until=(1e-3, 4, 2), until_want=None)
        # PoissonChambollePock (its restatement is tied to ``counts(shape)`` and ``_kw_of(shape)`` = XKW)
        d = np.asarray(t_kl.counts(shape))
        wx, wloss, wq, ltol = t_kl.np_trajectory(shape, scheme, N_IT)
        tau, sigma = t_kl._steps_of(shape, scheme)
        add("kl_%s" % scheme, "PoissonChambollePock", d, (t_kl.REG,), dict(XKW, scheme=scheme), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", ltol=ltol, cert=t_kl.np_residuals(wx, wq, d, t_kl.REG, scheme, XKW, tau, sigma),
                 scale=float(np.max(d))), cert="res", until=(1e-3, 4, 2), until_want=None)
        # WeightedChambollePock: 30 % of the sites with w = 0 and the box [0, 18]
        d, w, lower, upper = t_wls.problem(shape, "inpaint_box")
        d, w = np.asarray(d), np.asarray(w)
        assert w.dtype == np.bool_ and 0.2 < np.mean(~w) < 0.4
        wx, wloss, wq, ltol = t_wls.np_trajectory(shape, scheme, "inpaint_box", N_IT)
        tau, sigma = t_wls._steps_of(shape, scheme)
        add("wls_%s" % scheme, "WeightedChambollePock", d, (t_wls.REG, w), dict(XKW, scheme=scheme, lower=lower, upper=upper), N_IT,
            dict(x=wx, loss=wloss, kind="xcp", ltol=ltol, scale=float(np.max(np.abs(d))),
                 cert=t_wls.np_residuals(wx, wq, d, w.astype(np.float64), lower, upper, t_wls.REG, scheme, XKW, tau, sigma)),
            cert="res", until=(1e-3, 4, 2), until_want=None)

    # ---- b. the radius-2 solvers where every rank holds two planes; e. the sub-gradient with a weight volume on (7, 2); and, on the
    #         partitions they refuse, the path that serves one-plane ranks already: a z axis that is not regularised exchanges nothing
    for scheme in TWO:
        if not thin:
            sx, sloss = orc.subgradient_descent(x0, 5, 7.0, 2e-3, scheme=scheme, **KW)
            for way, how in (("sg", dict()), ("sg_serial", dict(overlap=False))):
                add("%s_%s" % (way, scheme), "SubgradientDescent", x0, (7.0, 2e-3), dict(KW, scheme=scheme, **how), 5, dict(x=sx, loss=sloss, kind="cp"))
            if sizes == (4, 3):
                vx, vloss = orc.subgradient_descent(x0, 5, 7.0, 2e-3, scheme=scheme, mask_static=W, **KW)
                add("sgw_%s" % scheme, "SubgradientDescent", x0, (7.0, 2e-3), dict(KW, scheme=scheme, mask_static=W), 5, dict(x=vx, loss=vloss, kind="cp"))
            for solver, n_cg in (("cg", 3), ("chebyshev", 4)):
                ax, aloss = orc.admm(x0, 3, 7.0, 0.1, n_cg, scheme=scheme, single_reduction=True, x_solver=solver, **KW)
                for fused in ((False, True) if sweep_ok else (False,)):
                    add("admm_%s_%s_%s" % (solver, "sweep" if fused else "plain", scheme), "ADMM", x0, (7.0, 0.1),
                        dict(KW, scheme=scheme, n_cg=n_cg, x_solver=solver, fused=fused), 3, dict(x=ax, loss=aloss, kind="admm"))
        elif scheme == "hybrid":
            kw0 = dict(reg_z_over_reg=0.0, reg_time=0.7)
            sx, sloss = orc.subgradient_descent(x0, 5, 7.0, 2e-3, scheme=scheme, **kw0)
            add("sg_z_off", "SubgradientDescent", x0, (7.0, 2e-3), dict(kw0, scheme=scheme), 5, dict(x=sx, loss=sloss, kind="cp"))
            ax, aloss = orc.admm(x0, 3, 7.0, 0.1, 4, scheme=scheme, single_reduction=True, x_solver="chebyshev", **kw0)
            add("admm_z_off", "ADMM", x0, (7.0, 0.1), dict(kw0, scheme=scheme, n_cg=4, x_solver="chebyshev", fused=False), 3,
                dict(x=ax, loss=aloss, kind="admm"))
    return jobs, checks


def _tolerances(kind, f32):
    """(loss rtol, x rtol, x atol) -- the module docstring says where each figure is stated"""
    return {"cp": (1e-5, 1e-5, 2e-3) if f32 else (1e-10, 1e-10, 1e-9),
            "admm": (1e-6, 2e-6, 2e-4) if f32 else (1e-9, 1e-9, 1e-8),
            "op": (2e-5, 1e-4, 2e-3) if f32 else (1e-10, 1e-10, 1e-9),
            "xcp": (1e-5, 1e-5, 2e-3) if f32 else (1e-10, None, None)}[kind]


@pytest.mark.parametrize("nzg,world,frame,dtype_name", CASES, ids=["%dover%d-%s-%s" % (n, w, "x".join(map(str, f)), d) for n, w, f, d in CASES])
def test_sharded_solvers_on_thin_slabs_equal_the_unsharded_oracle(nzg, world, frame, dtype_name, tvopt):
    from pytv.slab import partition
    sizes = PARTITIONS[(nzg, world)]
    assert tuple(n for _, n in partition(nzg, world)) == sizes
    tvopt("TV_FUSED_MIN_KVOXELS", 0)                 # the default path of these small volumes is the one-sweep kernel where it applies
    tvopt("TV_ZCHUNK", 1 if (nzg, world) == (8, 3) else 0)       # (8, 3): 3, 3, 2 chunks -- the one-sweep overlap threshold beside a rank below it
    shape = (nzg,) + frame
    f32 = dtype_name == "float32"
    jobs, checks = _plan(shape, dtype_name, sizes)
    t0 = time.monotonic()
    ranks = _spawn(world, nzg, dtype_name, jobs)
    print("%d jobs on %d ranks: %.1f s" % (len(jobs), world, time.monotonic() - t0))
    R = 1e-5 if f32 else 1e-10
    sweep_ok = frame[2] >= 64                        # (both frames of that width hold whole 16-byte lanes in either precision)
    for key, chk in checks.items():
        lrt, xrt, xat = _tolerances(chk["kind"], f32)
        got0 = ranks[0][key]
        print("PATH %s planes %s %s %s %s: %s" % (key, "+".join(map(str, sizes)), "x".join(map(str, frame)), dtype_name,
                                                  "TV_ZCHUNK=1" if (nzg, world) == (8, 3) else "",
                                                  " | ".join(",".join("%s=%s" % kv for kv in sorted(ranks[r][key]["attrs"].items())) for r in range(world))))
        for r in range(world):
            got = ranks[r][key]
            z0, nz = ranks[r]["z"]
            assert nz == sizes[r]
            msg = "%s, rank %d (planes [%d, %d) of %d)" % (key, r, z0, z0 + nz, nzg)
            wx = chk["x"][z0:z0 + nz]
            assert got["x"].shape == wx.shape, msg
            # ---- the loss history is the global one, on every rank
            if "ltol" in chk and f32:
                assert np.all(np.abs(got["loss"] - chk["loss"]) <= chk["ltol"]), msg
            else:
                np.testing.assert_allclose(got["loss"], chk["loss"], rtol=lrt, atol=0, err_msg=msg)
            np.testing.assert_array_equal(got["loss"], got0["loss"], err_msg=msg)
            # ---- this rank's planes of the iterate
            if xrt is None:
                assert float(np.max(np.abs(got["x"] - wx))) <= 1e-9 * chk["scale"], msg
            else:
                np.testing.assert_allclose(got["x"], wx, rtol=xrt, atol=xat, err_msg=msg)
            # ---- the certificate: the same numbers on every rank, and the oracle's
            if "cert" in got:
                assert got["cert"] == got0["cert"], msg
            if "g_max" in chk:
                assert got["g_max"] == chk["g_max"], msg          # the maximum over ALL ranks, on every rank
            if "until" in got:
                assert got["until"] == got0["until"] and got["until"][0] == got["until"][2], msg      # every rank stops at the same iteration
                if chk.get("until_want") is not None:
                    assert got["until"][0] == chk["until_want"], msg
        if "cert" in got0 and isinstance(got0["cert"], tuple):
            primal, dual, gap = got0["cert"]
            wprimal, wgap = chk["cert"]
            assert abs(primal - wprimal) <= R * wprimal and abs(gap - wgap) <= R * wprimal and dual == primal - gap, key
        elif "cert" in got0 and not f32:
            wres, floor = chk["cert"]
            for k in ("tv", "fid", "x", "q"):
                assert abs(got0["cert"][k] - wres[k]) <= 1e-9 * abs(wres[k]) + (floor if k == "x" else 0.0), (key, k, got0["cert"], wres)
            assert got0["cert"]["total"] == got0["cert"]["x"] + got0["cert"]["q"], key
    # ---- the paths that ran: read from the solvers' attributes inside the ranks
    at = lambda key, name: [ranks[r][key]["attrs"].get(name) for r in range(world)]         # noqa: E731
    for scheme in SCHEMES:
        assert at("cp_pair_%s" % scheme, "fused") == [False] * world and at("cp_pair_serial_%s" % scheme, "overlap") == [False] * world
        assert at("cp_pair_%s" % scheme, "overlap") == [n >= 3 for n in sizes]               # solvers.py: overlap needs an interior plane
        assert at("cp_default_%s" % scheme, "fused") == [sweep_ok] * world
        if sweep_ok:
            nch = at("cp_sweep_%s" % scheme, "nchunks")
            # tv_fused.hip, fused_zchunk on a slab of these sizes: chunks of 4 planes, clipped to the slab -- one chunk up to 4 planes
            assert nch == (list(sizes) if (nzg, world) == (8, 3) else [-(-n // min(4, n)) for n in sizes])
            assert at("cp_sweep_%s" % scheme, "overlap_fused") == [c >= 3 and n >= 3 for c, n in zip(nch, sizes)]
            assert at("cp_sweep_serial_%s" % scheme, "overlap_fused") == [False] * world
    if min(sizes) >= 2:
        for scheme in TWO:
            assert at("sg_%s" % scheme, "one_pass") == [True] * world
            assert at("sg_%s" % scheme, "overlap") == [n >= 5 for n in sizes] and at("sg_serial_%s" % scheme, "overlap") == [False] * world
            assert at("admm_cg_plain_%s" % scheme, "overlap") == [n >= 5 for n in sizes]
    if (nzg, world) == (8, 3):          # two schedules side by side in one job
        assert len(set(at("cp_pair_hybrid", "overlap"))) == 2
        if sweep_ok:
            assert len(set(at("cp_sweep_hybrid", "overlap_fused"))) == 2
    if (nzg, world) == (9, 2):
        assert len(set(at("sg_hybrid", "overlap"))) == 2 and len(set(at("admm_chebyshev_plain_hybrid", "overlap"))) == 2


# ------------------------------------------------------------------------------------------------
# d. refusal: one process, no process group -- anything that communicates before the check surfaces as another exception
# ------------------------------------------------------------------------------------------------
def _radius2_makers(pytv, W=None):
    kw = dict(KW) if W is None else dict(KW, mask_static=W)
    return [("SubgradientDescent", lambda x, slab: pytv.solvers.SubgradientDescent(x, 7.0, 2e-3, slab=slab, **kw)),
            ("ADMM", lambda x, slab: pytv.solvers.ADMM(x, 7.0, 0.1, n_cg=3, x_solver="cg", slab=slab, **kw)),
            ("ADMM", lambda x, slab: pytv.solvers.ADMM(x, 7.0, 0.1, n_cg=4, slab=slab, **kw))]


@pytest.mark.parametrize("nzg,world", ONE_PLANE)
def test_radius2_solvers_refuse_a_partition_with_a_one_plane_rank(nzg, world):
    import pytv
    from pytv.slab import Slab
    assert not dist.is_initialized()
    sizes = list(PARTITIONS[(nzg, world)])
    messages = {}
    for r in range(world):
        slab = Slab(nzg, rank=r, world=world)
        assert slab.nz == sizes[r]
        x = torch.zeros((slab.nz,) + SITE_FRAME, dtype=torch.float64, device="cuda")
        # (with a per-voxel time weight the constructor's first communication is the exchange of the weight's ghost planes)
        for W in (None, np.ones((slab.nz,) + SITE_FRAME)):
            for name, make in _radius2_makers(pytv, W):
                with pytest.raises(ValueError, match="every rank must hold >= 2 planes") as e:
                    make(x, slab)
                messages.setdefault(name, set()).add(str(e.value))
    for name, texts in messages.items():
        assert len(texts) == 1, texts                          # the same text from every rank, those that hold two planes included
        text = texts.pop()
        assert name in text and str(sizes) in text and "%d planes over %d ranks" % (nzg, world) in text


@pytest.mark.parametrize("nzg,world", ONE_PLANE)
def test_one_plane_halo_solvers_and_an_unregularised_z_axis_are_not_refused(nzg, world):
    """``Slab``'s own rule stays (nz_global >= world); the radius-2 solvers exchange nothing when the z axis is not regularised, so a
    one-plane rank constructs and steps without a process group"""
    import pytv
    from pytv.slab import HaloPlan, Slab
    assert not dist.is_initialized()
    r = world - 1
    slab = Slab(nzg, rank=r, world=world)
    assert slab.nz == 1
    x = torch.ones((1,) + SITE_FRAME, dtype=torch.float64, device="cuda")
    assert pytv.solvers.ChambollePock(x, 7.0, slab=slab, **KW).plan.on
    kw0 = dict(reg_z_over_reg=0.0, reg_time=0.7)
    sg = pytv.solvers.SubgradientDescent(x, 7.0, 2e-3, slab=slab, **kw0)
    assert not sg.plan.on and sg.xh_prev is None and sg.xh_next is None
    sg.step()
    ad = pytv.solvers.ADMM(x, 7.0, 0.1, n_cg=4, slab=slab, **kw0)
    assert not ad.plan.on and ad.h2_prev is None
    torch.cuda.synchronize()
    # the exchange itself refuses to slice short
    plan = HaloPlan(slab, "hybrid", True)
    buf = torch.zeros((2,) + SITE_FRAME, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="two-plane halos need a slab of >= 2 planes"):
        plan.exchange_image2(x, buf, None)
    assert HaloPlan(slab, "hybrid", False).exchange_image2(x, buf, None) == []
