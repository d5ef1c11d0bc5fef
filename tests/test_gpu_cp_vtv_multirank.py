"""``VectorialTVChambollePock`` on z-slabs with ONE GPU (the harness of tests/test_gpu_cp_hwtv_multirank.py: the ranks are child processes
that share cuda:0 and talk over gloo, halo planes staged through the host, joined under a hard time limit), 2 and 3 ranks.  tv_cp_dual_vtv is
the first kernel in which one thread walks all M frames of the halo planes x_prev / x_next itself, and tv_dual_gap_vtv does the same with
q_prev / q_next: a halo that is exchanged, indexed or all-reduced wrongly changes seam planes only, which no unsharded test sees.

Expected values: the fp64 NumPy restatement ``np_vectorial`` / ``ref_gap`` of tests/test_cp_vtv_inputs.py on the UNSHARDED volume (imported, as
is the data ``coupled_square`` of tests/test_gpu_cp_vtv.py); the unsharded GPU solver in this process is a second, tighter comparison.  Each
spawned job runs every (scheme, weighting) of its (shape, world, precision) in a row, as tests/test_gpu_thin_slabs.py does.

    shapes      (4, 2, 8, 64) whole lanes, M = 2: register form in every scheme; 3 ranks hold 2 + 1 + 1 planes
                (5, 5, 6, 8)  M = 5: register form in upwind, generic form in hybrid; 3 + 2 and 2 + 2 + 1 planes
                (4, 9, 5, 13) scalar rows, M = 9: generic form in every scheme
    weightings  plain, no_time, mask (a (1, 1, Ny, Nx) map, the same on every rank), weight_vol (a per-voxel time weight cut by planes and
                passed as a host array: its ghost planes travel before the first step, its maximum is all-reduced into L^2)
    schemes     all four at 2 ranks on the first shape, hybrid and upwind elsewhere;  fp64 everywhere, fp32 on the first shape

The restatement must itself make the joint projection act where the ranks meet: in the seam planes (the first and last plane of every rank) at
least ``MIN_SHARE`` of the spatial sites are "coupled" in the last iteration (|v_s|_F > REG while a frame of the site has |v_s[:, m]|_2 <=
REG) -- there a per-frame projection gives another q.  With REG = 10 and 10 iterations the smallest such share over all cases is 0.237
(``test_the_joint_projection_acts_in_the_seam_planes_of_the_restatement`` prints them all; no GPU).

Tolerances are the project's: fp64 loss rtol 1e-10, max|dx| <= 1e-9 max|x0|, primal and gap to 1e-10 primal against the restatement and to
1e-11 primal against the unsharded GPU run; fp32 (fp32-rounded input) loss rtol 1e-5, x rtol 1e-5 / atol 2e-3, certificate to 1e-5 primal.
Measured against the restatement on an MI355X, the largest over all cases, sharded | unsharded (the test prints both for every case):
fp64 loss 6.7e-16 | 6.7e-16, max|dx| 5.7e-14 | 5.7e-14 (1e-9 max|x0| = 1.2e-7), primal 3.6e-16 | 3.6e-16, gap / primal 5.8e-17 | 6.0e-17, sharded
against unsharded primal 2.1e-16; fp32 loss 7.3e-8 | 7.3e-8, max|dx| 3.0e-5 | 3.0e-5, primal 1.8e-8 | 1.8e-8."""
import datetime
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT, SCHEMES
from oracle import tv_oracle as orc
from test_cp_vtv_inputs import MIN_SHARE, case_kw, np_vectorial, ref_gap, shares
from test_gpu_cp_prox_multirank import _free_port
from test_gpu_cp_vtv import coupled_square
from test_gpu_thin_slabs import _gap_count

REG, N_ITER = 10.0, 10
CHILD_LIMIT_S = 120
SEGMENTS = (2, 2, 2, 3, 1)             # the restatement stops after 2, 4, 6 (the checks of run_until), 9 (v of the last iteration) and 10 iterations
UNTIL = (6, 2)                         # run_until(rel, 6, 2)
REFUSAL = ("set_fused(True): VectorialTVChambollePock has no one-sweep path (the one-sweep kernels project each frame's dual vector on its "
           "own)")
WEIGHTINGS = ("plain", "no_time", "mask", "weight_vol")
TWO = ("hybrid", "upwind")
LANES, ODD, ROWS = (4, 2, 8, 64), (5, 5, 6, 8), (4, 9, 5, 13)
PARTITIONS = {(4, 2): (2, 2), (4, 3): (2, 1, 1), (5, 2): (3, 2), (5, 3): (2, 2, 1)}
# (shape, world, precision, schemes)
CASES = [(LANES, 2, "float64", SCHEMES), (LANES, 3, "float64", TWO), (LANES, 2, "float32", SCHEMES), (LANES, 3, "float32", TWO),
         (ODD, 2, "float64", TWO), (ODD, 3, "float64", TWO), (ROWS, 2, "float64", TWO), (ROWS, 3, "float64", TWO)]
IDS = ["%s-%dranks-%s" % ("x".join(map(str, s)), w, d) for s, w, d, _ in CASES]


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _problem(shape, weighting, f32):
    """(x0, kw): the data and the weighting, both rounded to fp32 where the ranks compute in fp32"""
    x0, kw = np.asarray(coupled_square(shape)), case_kw(weighting, shape)
    if f32:
        x0 = _f32(x0)
        if weighting == "weight_vol":
            kw = dict(kw, mask_static=_f32(kw["mask_static"]))
    return x0, kw


@functools.lru_cache(maxsize=None)
def reference(shape, scheme, weighting, f32):
    """the restatement on the unsharded volume, once per problem: x and the loss history after ``N_ITER`` iterations, (primal, gap) after 2, 4,
    6 and ``N_ITER``, and v = q + sigma D x_bar of the last dual step"""
    x0, kw = _problem(shape, weighting, f32)
    state, loss, certs, done, v_last = None, [], {}, 0, None
    for n in SEGMENTS:
        if done == N_ITER - 1:
            _, xb, q, _, sigma = state
            v_last = q + sigma * orc.D(xb, scheme, **kw)
        x, part, state = np_vectorial(x0, n, REG, scheme, kw, state=state)
        loss.append(part)
        done += n
        vtv, fid, gap, _ = ref_gap(state[0], state[2], x0, REG, scheme, kw)
        certs[done] = (fid + REG * vtv, gap)
    assert done == N_ITER and v_last is not None
    return dict(x=x, loss=np.concatenate(loss), certs=certs, v=v_last, scale=float(np.max(np.abs(x0))), L2=orc.normal_spectral_bound(scheme, shape, **kw))


def _until(ref):
    """(rel, the iteration run_until(rel, 6, 2) stops at): rel between the 2nd and the 4th iteration's relative gaps"""
    states = [ref["certs"][n] for n in (2, 4, 6)]
    rel = float(np.sqrt((states[0][1] / states[0][0]) * (states[1][1] / states[1][0])))
    # (no check sits on the threshold: the fp32 certificate is good to 1e-5 primal)
    assert all(abs(gap / primal - rel) > 1e-3 * rel for primal, gap in states)
    return rel, _gap_count(states, rel, UNTIL[1], UNTIL[0])


def _seam_planes(nzg, world):
    from pytv.slab import partition
    return sorted({z for z0, nz in partition(nzg, world) for z in (z0, z0 + nz - 1)})


def _seam_share(ref, nzg, world):
    """the share of coupled sites among the spatial sites of the seam planes, in the last dual step of the restatement"""
    return float(np.mean(shares(ref["v"], REG)[3][_seam_planes(nzg, world)]))


def test_the_joint_projection_acts_in_the_seam_planes_of_the_restatement():
    """on the fp64 restatement alone (no GPU): every case of the sharded test has >= MIN_SHARE coupled sites in its seam planes"""
    low = 1.0
    for shape, world, dtype_name, schemes in CASES:
        for scheme in schemes:
            for weighting in WEIGHTINGS:
                share = _seam_share(reference(shape, scheme, weighting, dtype_name == "float32"), shape[0], world)
                print("%s %d ranks %s %s %s: coupled share of the seam planes %.3f" % (shape, world, dtype_name, scheme, weighting, share))
                assert share >= MIN_SHARE, (shape, world, dtype_name, scheme, weighting, share)
                low = min(low, share)
    print("smallest share %.3f" % low)


# ------------------------------------------------------------------------------------------------
# the ranks
# ------------------------------------------------------------------------------------------------
def _run(pytv, x0, kw, scheme, rel, slab=None):
    """one configuration on this process's planes: N_ITER iterations, the certificate, the steps, the refusal, and run_until on a fresh solver"""
    def build():
        return pytv.solvers.VectorialTVChambollePock(x0.clone(), REG, scheme=scheme, slab=slab, **kw)

    s = build()
    out = dict(fused=[s.fused], L2=s.L2, start=(s.tau0, s.sigma0, s.gamma), steps=[s._steps(k) for k in range(N_ITER)])
    try:
        s.set_fused(True)
        out["refusal"] = None
    except ValueError as e:
        out["refusal"] = str(e)
    out["fused"].append(s.fused)
    out["loss"] = np.asarray(s.run(N_ITER), dtype=np.float64)
    out["x"] = s.result().cpu().numpy()
    out["cert"] = tuple(s.duality_gap())
    t = build()
    loss, info = t.run_until(rel, *UNTIL)
    out["until"] = (int(info["iterations"]), bool(info["converged"]), len(loss))
    return out


def _worker(rank, world, port, nzg, dtype_name, jobs, ret):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=CHILD_LIMIT_S // 2))
    try:
        import pytv
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(nzg)
        tdt = getattr(torch, dtype_name)
        out = {"z": (slab.z0, slab.nz)}
        for job in jobs:
            x0 = torch.as_tensor(np.ascontiguousarray(slab.local(job["x0"]))).to(tdt).cuda()
            # (a per-voxel time weight goes in as a host array of this rank's slab shape, as in tests/test_gpu_thin_slabs.py)
            kw = {k: np.ascontiguousarray(slab.local(v)) if isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg else v
                  for k, v in job["kw"].items()}
            out[job["key"]] = _run(pytv, x0, kw, job["scheme"], job["rel"], slab)
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def _spawn(world, nzg, dtype_name, jobs):
    """the ranks as child processes, joined under CHILD_LIMIT_S: a child that hangs is killed and the test fails"""
    assert world <= 3
    ret = mp.Manager().dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), nzg, dtype_name, jobs, ret), nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_LIMIT_S
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish within %d s" % CHILD_LIMIT_S)
    assert len(ret) == world
    return [ret[r] for r in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,world,dtype_name,schemes", CASES, ids=IDS)
def test_sharded_solver_equals_the_unsharded_restatement(shape, world, dtype_name, schemes):
    import pytv
    from pytv.slab import partition
    nzg, f32 = shape[0], dtype_name == "float32"
    sizes = PARTITIONS[(nzg, world)]
    assert tuple(n for _, n in partition(nzg, world)) == sizes
    jobs, refs = [], {}
    for scheme in schemes:
        for weighting in WEIGHTINGS:
            key = "%s_%s" % (scheme, weighting)
            x0, kw = _problem(shape, weighting, f32)
            ref = refs[key] = dict(reference(shape, scheme, weighting, f32))
            ref["rel"], ref["stop"] = _until(ref)
            assert _seam_share(ref, nzg, world) >= MIN_SHARE, key                # the joint projection acts where the ranks meet
            jobs.append(dict(key=key, scheme=scheme, x0=x0, kw=kw, rel=ref["rel"]))
    t0 = time.monotonic()
    ranks = _spawn(world, nzg, dtype_name, jobs)
    print("%d configurations on %d ranks: %.1f s" % (len(jobs), world, time.monotonic() - t0))
    R = 1e-5 if f32 else 1e-10
    for job in jobs:
        key, ref = job["key"], refs[job["key"]]
        whole = _run(pytv, torch.as_tensor(job["x0"]).to(getattr(torch, dtype_name)).cuda(), job["kw"], job["scheme"], ref["rel"])
        got0 = ranks[0][key]
        wprimal, wgap = ref["certs"][N_ITER]
        primal, dual, gap = got0["cert"]
        uprimal, _, ugap = whole["cert"]
        print("%s %s planes %s %s: loss rel %.3e (unsharded %.3e)  primal rel %.3e gap / primal %.3e (unsharded %.3e %.3e; sharded against "
              "unsharded %.3e %.3e)  stop %r want %d" % (
                  "x".join(map(str, shape)), key, "+".join(map(str, sizes)), dtype_name, np.max(np.abs(got0["loss"] / ref["loss"] - 1.0)),
                  np.max(np.abs(whole["loss"] / ref["loss"] - 1.0)), abs(primal - wprimal) / wprimal, abs(gap - wgap) / wprimal,
                  abs(uprimal - wprimal) / wprimal, abs(ugap - wgap) / wprimal, abs(primal - uprimal) / uprimal, abs(gap - ugap) / uprimal,
                  got0["until"], ref["stop"]))
        assert whole["L2"] == ref["L2"] and whole["refusal"] == REFUSAL, key
        for r in range(world):
            got = ranks[r][key]
            z0, nz = ranks[r]["z"]
            assert nz == sizes[r]
            msg = "%s, rank %d (planes [%d, %d) of %d)" % (key, r, z0, z0 + nz, nzg)
            wx = ref["x"][z0:z0 + nz]
            dx = float(np.max(np.abs(got["x"] - wx)))
            print("   rank %d: max|dx| %.3e (unsharded on these planes %.3e; 1e-9 max|x0| = %.3e)" % (
                r, dx, np.max(np.abs(whole["x"][z0:z0 + nz] - wx)), 1e-9 * ref["scale"]))
            # ---- the path: the kernel pair, and this class's own refusal of the one-sweep path (not the parent class's slab refusal)
            assert got["fused"] == [False, False] and got["refusal"] == REFUSAL, msg
            # ---- the schedule and the bound it starts from: the unsharded solver's, bit for bit, on every rank
            assert got["L2"] == whole["L2"] and got["start"] == whole["start"] and got["steps"] == whole["steps"], msg
            # ---- the loss history is the global one, identical on every rank
            np.testing.assert_allclose(got["loss"], ref["loss"], rtol=1e-5 if f32 else 1e-10, atol=0, err_msg=msg)
            np.testing.assert_array_equal(got["loss"], got0["loss"], err_msg=msg)
            # ---- this rank's planes of the iterate
            assert got["x"].shape == wx.shape, msg
            if f32:
                np.testing.assert_allclose(got["x"], wx, rtol=1e-5, atol=2e-3, err_msg=msg)
            else:
                assert dx <= 1e-9 * ref["scale"], msg
            # ---- the certificate and the stopping iteration: the same on every rank
            assert got["cert"] == got0["cert"], msg
            assert got["until"] == got0["until"] and got["until"][0] == got["until"][2] == ref["stop"], msg
        assert dual == primal - gap, key
        assert abs(primal - wprimal) <= R * wprimal and abs(gap - wgap) <= R * wprimal, key
        if not f32:
            assert gap > 0.0, key
            assert abs(primal - uprimal) <= 1e-11 * uprimal and abs(gap - ugap) <= 1e-11 * uprimal, key
        assert whole["until"] == got0["until"], key
