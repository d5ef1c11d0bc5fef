"""``AdaptiveHuberChambollePock`` on z-slabs with ONE GPU (the harness of tests/test_gpu_cp_wtv_multirank.py: the ranks share cuda:0 and talk
over gloo, halo planes staged through the host), 2 and 3 ranks: the sharded iteration (the kernel pair) with the weight g split by planes and
its duality gap against the unsharded pair in this process, and the steps, which come from the maximum of g over ALL ranks: the largest weight
sits in plane 0, on rank 0 only, and every rank takes the steps of the unsharded solver.  The children are joined under a hard time limit."""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from test_gpu_cp_prox_multirank import _free_port

pytestmark = pytest.mark.gpu

SHAPE, REG, ALPHA, N_ITER = (4, 2, 8, 64), 10.0, 2.0, 10          # 64 columns, whole lanes: a geometry the one-sweep kernel takes
KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
G_MAX = 5.0
CHILD_LIMIT_S = 120.0


def _data():
    """a centred square of height 100 plus N(0, 10^2) noise (tests/test_gpu_cp_huber.py)"""
    x = np.zeros(SHAPE)
    ny, nx = SHAPE[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    return x + 10.0 * np.random.default_rng(0).standard_normal(SHAPE)


def _weights():
    """a third of the sites 0, a third in [0.25, 1), a third in [1, 3]; ONE site of plane 0 holds the maximum G_MAX"""
    rng = np.random.default_rng(23)
    kind, u = rng.integers(0, 3, SHAPE), rng.random(SHAPE)
    g = np.where(kind == 0, 0.0, np.where(kind == 1, 0.25 + 0.75 * u, 1.0 + 2.0 * u))
    g[0, 1, 5, 7] = G_MAX
    assert float(g[1:].max()) <= 3.0
    return g


def _run(x0, g, scheme, slab=None):
    import pytv
    cp = pytv.solvers.AdaptiveHuberChambollePock(torch.as_tensor(x0.copy()).cuda(), REG, torch.as_tensor(g.copy()).cuda(), ALPHA, scheme=scheme,
                                                 slab=slab, **KW)
    cp.set_fused(False)                                                   # the pair on both sides (a slab has no other path)
    out = dict(steps=(cp.tau, cp.sigma, cp.theta, cp.g_max), local_max=float(g.max()), loss=cp.run(N_ITER), x=cp.result().cpu().numpy())
    out["gap"] = cp.duality_gap()
    return out


def _worker(rank, world, port, scheme, ret):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pytv
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(SHAPE[0])
        out = _run(slab.local(_data()), slab.local(_weights()), scheme, slab)
        out["z"] = (slab.z0, slab.nz)
        cp = pytv.solvers.AdaptiveHuberChambollePock(torch.as_tensor(slab.local(_data()).copy()).cuda(), REG,
                                                     torch.as_tensor(slab.local(_weights()).copy()).cuda(), ALPHA, scheme=scheme, slab=slab, **KW)
        out["default_fused"] = cp.fused
        try:
            cp.set_fused(True)
            out["refused"] = False
        except ValueError as e:
            out["refused"] = "unsharded" in str(e)    # the slab refusal itself: the geometry is one the sweep supports
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def _spawn(world, scheme):
    """the ranks as child processes, joined under CHILD_LIMIT_S: a child that hangs is killed and the test fails"""
    ret = mp.Manager().dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), scheme, ret), nprocs=world, join=False)
    deadline = time.monotonic() + CHILD_LIMIT_S
    while not ctx.join(timeout=1.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish within %.0f s" % CHILD_LIMIT_S)
    return dict(ret)


@pytest.mark.parametrize("world,scheme", [(2, "upwind"), (2, "downwind"), (2, "central"), (2, "hybrid"), (3, "hybrid"), (3, "upwind")])
def test_sharded_solver_equals_the_unsharded_pair(world, scheme):
    """fp64: a slab's sites see the arithmetic of the whole volume, so only the order of the fp64 sums differs.  Tolerances: the fp64 trajectory
    tolerance (loss rtol 1e-10, result 1e-9 max|x0|) and the fp64 scalar tolerance 1e-11 of the sums the certificate is made of"""
    whole = _run(_data(), _weights(), scheme)
    assert whole["steps"][3] == G_MAX
    ret = _spawn(world, scheme)
    assert len(ret) == world
    tol = 1e-9 * float(np.max(np.abs(_data())))
    assert ret[0]["local_max"] == G_MAX and all(ret[r]["local_max"] <= 3.0 for r in range(1, world))       # g_max lives on rank 0 only
    for r in range(world):
        z0, nz = ret[r]["z"]
        print("%s rank %d of %d planes [%d, %d): steps %r max|dx| %.3e (tol %.3e) gap %r unsharded %r" % (
            scheme, r, world, z0, z0 + nz, ret[r]["steps"], np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz])), tol, ret[r]["gap"], whole["gap"]))
        assert ret[r]["steps"] == whole["steps"], (r, ret[r]["steps"], whole["steps"])       # identical on every rank, bit for bit
        assert float(np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz]))) <= tol
        np.testing.assert_allclose(ret[r]["loss"], whole["loss"], rtol=1e-10)
        assert ret[r]["gap"] == ret[0]["gap"]
        assert ret[r]["default_fused"] is False and ret[r]["refused"] is True
    primal, dual, gap = ret[0]["gap"]
    wprimal, wdual, wgap = whole["gap"]
    assert gap > 0.0 and dual == primal - gap
    assert abs(primal - wprimal) <= 1e-11 * wprimal
    assert abs(gap - wgap) <= 1e-11 * wprimal                            # (the gap's terms are of the size of the primal's)
