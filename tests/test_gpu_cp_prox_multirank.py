"""``RobustChambollePock`` on z-slabs with ONE GPU (the harness of tests/test_gpu_multirank.py: two processes share cuda:0 and talk over gloo,
halo planes staged through the host): the sharded iteration and its optimality residuals against the unsharded solver in this process."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

SHAPE, REG, TAU, N_ITER = (6, 2, 16, 20), 1.0, 5.0, 20
KW = dict(reg_z_over_reg=0.7, reg_time=0.25)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data(dtype):
    """the square of height 100 with 10 % of the sites set to 0 or 255 (tests/test_gpu_cp_prox.py)"""
    x = np.zeros(SHAPE)
    ny, nx = SHAPE[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    r = np.random.default_rng(0).random(SHAPE)
    x[r < 0.05] = 0.0
    x[r > 0.95] = 255.0
    return x.astype(dtype)


def _run(x0, scheme, slab=None):
    import pytv
    cp = pytv.solvers.RobustChambollePock(torch.as_tensor(x0.copy()).cuda(), REG, fidelity="l1", scheme=scheme, tau=TAU, slab=slab, **KW)
    out = dict(r0=cp.initial_residual(), loss=cp.run(N_ITER), x=cp.result().cpu().numpy())
    out["res"] = cp.residuals()
    return out


def _worker(rank, world, port, scheme, dtype_name, ret):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytv.slab import Slab
        torch.cuda.set_device(0)
        slab = Slab(SHAPE[0])
        out = _run(slab.local(_data(np.dtype(dtype_name))), scheme, slab)
        out["z"] = (slab.z0, slab.nz)
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("scheme", ("hybrid", "upwind"))
def test_sharded_robust_solver_equals_the_unsharded_one(scheme, dtype):
    world = 2
    whole = _run(_data(dtype), scheme)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), scheme, np.dtype(dtype).name, ret), nprocs=world, join=True)
    assert len(ret) == world
    rtol = 1e-11 if dtype == np.float64 else 1e-5
    tol = rtol * float(np.max(np.abs(whole["x"])))
    for r in range(world):
        z0, nz = ret[r]["z"]
        print("%s %s rank %d planes [%d, %d): max|dx| %.3e (tol %.3e)  residuals %r  unsharded %r" % (
            scheme, np.dtype(dtype).name, r, z0, z0 + nz, np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz])), tol, ret[r]["res"], whole["res"]))
        assert float(np.max(np.abs(ret[r]["x"] - whole["x"][z0:z0 + nz]))) <= tol
        np.testing.assert_allclose(ret[r]["loss"], whole["loss"], rtol=rtol)
        assert ret[r]["res"] == ret[0]["res"] and ret[r]["r0"] == ret[0]["r0"]          # every rank gets the same numbers
        assert ret[r]["res"]["total"] == ret[r]["res"]["x"] + ret[r]["res"]["q"]
    # the sharded scalars are the unsharded ones: a slab's sites see the arithmetic of the whole volume (tests/test_gpu_cp_prox.py, z-ranges:
    # bit-equal arrays), so only the order of the fp64 sums differs -- the 1e-13 of that test per kernel, over 20 iterations of state
    for k in ("tv", "fid", "x", "q"):
        np.testing.assert_allclose(ret[0]["res"][k], whole["res"][k], rtol=rtol, err_msg=k)
    np.testing.assert_allclose(ret[0]["r0"], whole["r0"], rtol=1e-12)
