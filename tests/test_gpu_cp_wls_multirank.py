"""``WeightedChambollePock`` on z-slabs with ONE GPU (the harness of tests/test_gpu_cp_kl_multirank.py: two processes share cuda:0 and talk over
gloo, halo planes staged through the host): the sharded iteration and its optimality residuals against the unsharded solver in this process."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from test_gpu_cp_prox_multirank import _free_port

pytestmark = pytest.mark.gpu

SHAPE, REG, N_ITER = (4, 2, 16, 20), 0.5, 10
KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
BOX = dict(lower=1.0, upper=18.0)          # a box without 0: every rank shifts by the same constant


def _data():
    """the phantom of tests/test_gpu_cp_wls.py (2 with a centred square of 20, N(0, 1) noise); a third of the sites unknown and zero-filled,
    the others weighted in [0.25, 2.25]"""
    rng = np.random.default_rng(0)
    c = np.full(SHAPE, 2.0)
    ny, nx = SHAPE[2:]
    c[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 20.0
    x0 = c + rng.standard_normal(SHAPE)
    w = np.where(rng.random(SHAPE) < 1.0 / 3.0, 0.0, 0.25 + 2.0 * rng.random(SHAPE))
    x0[w == 0.0] = 0.0
    return x0, w


def _run(x0, w, scheme, slab=None):
    import pytv
    cp = pytv.solvers.WeightedChambollePock(torch.as_tensor(x0.copy()).cuda(), REG, torch.as_tensor(w.copy()).cuda(), scheme=scheme, slab=slab,
                                            **BOX, **KW)
    out = dict(r0=cp.initial_residual(), loss=cp.run(N_ITER), x=cp.result().cpu().numpy(), shift=cp.shift)
    out["res"] = cp.residuals()
    return out


def _worker(rank, world, port, scheme, ret):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(SHAPE[0])
        x0, w = _data()
        out = _run(slab.local(x0), slab.local(w), scheme, slab)
        out["z"] = (slab.z0, slab.nz)
        # a negative weight on ONE rank is refused on every rank (the check is collective); so are weights that vanish on every rank, while
        # weights that vanish on one rank only are fine
        import pytv
        bad = slab.local(w).copy()
        if rank == 1:
            bad[0, 0, 3, 4] = -1.0
        refused = []
        for weights in (bad, np.zeros_like(bad)):
            try:
                pytv.solvers.WeightedChambollePock(torch.as_tensor(slab.local(x0).copy()).cuda(), REG, torch.as_tensor(weights).cuda(),
                                                   scheme=scheme, slab=slab, **KW)
                refused.append(False)
            except ValueError:
                refused.append(True)
        out["refused"] = refused
        one = slab.local(w).copy() * (rank == 0)
        pytv.solvers.WeightedChambollePock(torch.as_tensor(slab.local(x0).copy()).cuda(), REG, torch.as_tensor(one).cuda(), scheme=scheme,
                                           slab=slab, **KW)
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("scheme", ("hybrid", "upwind"))
def test_sharded_weighted_solver_equals_the_unsharded_one(scheme):
    """fp64: a slab's sites see the arithmetic of the whole volume (tests/test_gpu_cp_wls.py, z-ranges: bit-equal arrays), so only the order
    of the fp64 sums differs"""
    world = 2
    whole = _run(*_data(), scheme)
    assert whole["shift"] == 1.0
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), scheme, ret), nprocs=world, join=True)
    assert len(ret) == world
    tol = 1e-12 * float(np.max(np.abs(whole["x"])))
    for r in range(world):
        z0, nz = ret[r]["z"]
        print("%s rank %d planes [%d, %d): max|dx| %.3e (tol %.3e)  residuals %r  unsharded %r" % (
            scheme, r, z0, z0 + nz, np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz])), tol, ret[r]["res"], whole["res"]))
        assert float(np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz]))) <= tol
        np.testing.assert_allclose(ret[r]["loss"], whole["loss"], rtol=1e-12)
        assert ret[r]["res"] == ret[0]["res"] and ret[r]["r0"] == ret[0]["r0"]          # every rank gets the same numbers
        assert ret[r]["res"]["total"] == ret[r]["res"]["x"] + ret[r]["res"]["q"]
        assert ret[r]["refused"] == [True, True] and ret[r]["shift"] == 1.0
    for k in ("tv", "fid", "x", "q"):
        np.testing.assert_allclose(ret[0]["res"][k], whole["res"][k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(ret[0]["r0"], whole["r0"], rtol=1e-12)
