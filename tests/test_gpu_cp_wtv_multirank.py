"""``AdaptiveTVChambollePock`` on z-slabs with ONE GPU (the harness of tests/test_gpu_cp_huber_multirank.py: two processes share cuda:0 and
talk over gloo, halo planes staged through the host): the sharded iteration with the weight g split by planes and its duality gap against the
unsharded solver in this process, and the constructor's collective refusal of a bad g that only one rank holds."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT, SCHEMES
from test_gpu_cp_prox_multirank import _free_port

pytestmark = pytest.mark.gpu

SHAPE, REG, N_ITER = (4, 2, 16, 20), 10.0, 10
KW = dict(reg_z_over_reg=0.7, reg_time=0.25)


def _data():
    """a centred square of height 100 plus N(0, 10^2) noise (tests/test_gpu_cp_huber.py)"""
    x = np.zeros(SHAPE)
    ny, nx = SHAPE[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    return x + 10.0 * np.random.default_rng(0).standard_normal(SHAPE)


def _weights():
    """a third of the sites 0, a third in (0, 1), a third in (1, 3)"""
    rng = np.random.default_rng(23)
    kind, u = rng.integers(0, 3, SHAPE), rng.random(SHAPE)
    return np.where(kind == 0, 0.0, np.where(kind == 1, 0.05 + 0.9 * u, 1.0 + 2.0 * u))


def _run(x0, g, scheme, slab=None):
    import pytv
    cp = pytv.solvers.AdaptiveTVChambollePock(torch.as_tensor(x0.copy()).cuda(), REG, torch.as_tensor(g.copy()).cuda(), scheme=scheme, slab=slab,
                                              **KW)
    out = dict(loss=cp.run(N_ITER), x=cp.result().cpu().numpy())
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
        # a bad g on rank 1 only: every rank raises (the check is collective), none hangs in a later collective
        refused = []
        for bad_value in (-1.0, float("nan"), float("inf")):
            g = slab.local(_weights()).copy()
            if rank == 1:
                g[0, 0, 3, 4] = bad_value
            try:
                pytv.solvers.AdaptiveTVChambollePock(torch.as_tensor(slab.local(_data()).copy()).cuda(), REG, torch.as_tensor(g).cuda(),
                                                     scheme=scheme, slab=slab, **KW)
                refused.append(False)
            except ValueError as e:
                refused.append("finite and >= 0" in str(e))
        out["refused"] = refused
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sharded_adaptive_solver_equals_the_unsharded_one(scheme):
    """fp64: a slab's sites see the arithmetic of the whole volume (tests/test_gpu_cp_wtv.py, z-ranges: bit-equal arrays), so only the order of
    the fp64 sums differs.  Tolerances: the fp64 trajectory tolerance of tests/test_gpu_cp_huber.py (loss rtol 1e-10, result 1e-9 max|x0|) and
    the fp64 scalar tolerance 1e-11 of the sums the certificate is made of"""
    world = 2
    whole = _run(_data(), _weights(), scheme)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), scheme, ret), nprocs=world, join=True)
    assert len(ret) == world
    tol = 1e-9 * float(np.max(np.abs(_data())))
    for r in range(world):
        z0, nz = ret[r]["z"]
        print("%s rank %d planes [%d, %d): max|dx| %.3e (tol %.3e)  gap %r  unsharded %r" % (
            scheme, r, z0, z0 + nz, np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz])), tol, ret[r]["gap"], whole["gap"]))
        assert float(np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz]))) <= tol
        np.testing.assert_allclose(ret[r]["loss"], whole["loss"], rtol=1e-10)
        assert ret[r]["gap"] == ret[0]["gap"]                            # every rank gets the same numbers
        assert ret[r]["refused"] == [True, True, True], (r, ret[r]["refused"])
    primal, dual, gap = ret[0]["gap"]
    wprimal, wdual, wgap = whole["gap"]
    assert gap > 0.0 and dual == primal - gap
    assert abs(primal - wprimal) <= 1e-11 * wprimal
    assert abs(gap - wgap) <= 1e-11 * wprimal                            # (the gap's terms are of the size of the primal's)
