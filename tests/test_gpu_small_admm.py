"""The persistent small-volume ADMM loop (round 7: csrc/tv_small.hip k_small_admm, C-ABI tv_small_admm, pytv.solvers.ADMM(persistent=True))
against the CPU oracle's Chebyshev ADMM and against the ordinary non-fused path.

Tolerances are the project's own, the looser of the two families this loop merges (test_gpu_small.py, test_admm_chebyshev_matches_oracle):
fp64 rtol 1e-9 / atol 1e-8; fp32 loss rtol 1e-5, x rtol 1e-5 / atol 2e-3; z and u at 10 x the rtol and 3 x the atol."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

REG, RHO = 25.0, 0.05
TOL = {np.float64: (1e-9, 1e-9, 1e-8), np.float32: (1e-5, 1e-5, 2e-3)}          # loss rtol, x rtol, x atol


@pytest.fixture(scope="module")
def pytv():
    import pytv
    return pytv


def _noisy(shape, seed, dtype):
    truth = orc.phantom(shape, seed=seed, dtype=np.float64)
    rng = np.random.RandomState(seed)
    return (truth + 100.0 * rng.rand(*shape)).astype(dtype)


CASES = [((1, 1, 16, 16), 1.0, 0.0, False), ((6, 1, 16, 16), 1.0, 0.0, False), ((5, 3, 12, 16), 1.0, 1.0, False), ((4, 4, 9, 10), 2.5, 0.5, True),
         ((3, 2, 7, 13), 1.0, 1.0, False), ((2, 5, 33, 20), 0.0, 1.0, False), ((7, 2, 5, 70), 1.5, 0.25, True)]
TINY = [(1, 1, 1, 1), (1, 1, 2, 2), (1, 1, 1, 7), (1, 1, 9, 1), (3, 1, 1, 1), (1, 5, 1, 3), (2, 2, 2, 2), (1, 1, 3, 130), (2, 3, 1, 4)]


def _against_oracle(pytv, x0, n_outer, K, scheme, kw, dtype, pitch=None, loss_atol=0.0):
    import torch
    lr, xr, xa = TOL[dtype]
    wx, wloss, wz, wu = orc.admm(x0.astype(np.float64), n_outer, REG, RHO, K, scheme=scheme, x_solver="chebyshev", return_state=True, **kw)
    assert np.all(np.isfinite(wloss))
    ad = pytv.solvers.ADMM(torch.as_tensor(x0).cuda(), REG, RHO, n_cg=K, scheme=scheme, persistent=True, pitch=pitch, **kw)
    assert ad.small and not ad.fused and ad.cheb
    loss = ad.run(n_outer)
    msg = "%s %s K=%d %s" % (scheme, x0.shape, K, np.dtype(dtype).name)
    np.testing.assert_allclose(loss, wloss, rtol=lr, atol=loss_atol, err_msg=msg)
    np.testing.assert_allclose(ad.result().cpu().numpy(), wx, rtol=xr, atol=xa, err_msg=msg)
    np.testing.assert_allclose(ad.z.cpu().numpy(), wz, rtol=10 * xr, atol=3 * xa, err_msg=msg)
    np.testing.assert_allclose(ad.u.cpu().numpy(), wu, rtol=10 * xr, atol=3 * xa, err_msg=msg)
    return ad


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,lz,mu,use_mask", CASES)
def test_persistent_admm_matches_oracle(pytv, scheme, shape, lz, mu, use_mask):
    """six outer iterations with 1, 2 and 5 Chebyshev steps, fp64 and fp32; 16-byte lanes where Nx allows, scalar lanes otherwise (Nx = 10, 13)"""
    rng = np.random.default_rng(4)
    mask = (rng.random((1, 1) + shape[2:]) > 0.5) if use_mask else False
    kw = dict(reg_z_over_reg=lz, reg_time=mu, mask_static=mask, factor_reg_static=4.0 if use_mask else 0)
    for dtype in (np.float64, np.float32):
        x0 = _noisy(shape, 5, dtype)
        for K in (1, 2, 5):
            _against_oracle(pytv, x0, 6, K, scheme, kw, dtype)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_persistent_admm_on_degenerate_shapes(pytv, scheme):
    """one-voxel images, single rows / columns, two-point axes; atol: the loss of a one-voxel image is exactly 0"""
    for shape in TINY:
        x0 = _noisy(shape, 11, np.float64)
        kw = dict(reg_z_over_reg=0.7, reg_time=1.3 if shape[1] > 1 else 0.0)
        _against_oracle(pytv, x0, 6, 3, scheme, kw, np.float64, loss_atol=1e-9)


@pytest.mark.parametrize("scheme", ["hybrid", "upwind", "central"])
def test_readme_shape_persistent_equals_the_ordinary_path(pytv, scheme):
    """README.md:76-79: (20, 4, 100, 100) fp32, 10 Chebyshev steps, 50 outer iterations: the persistent loop against the kernels the
    non-fused path launches one by one (loss bound: that of test_admm_fused_equals_kernel_trio)"""
    import torch
    rng = np.random.default_rng(0)
    x0 = torch.as_tensor((100.0 * rng.random((20, 4, 100, 100))).astype(np.float32)).cuda()
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    a = pytv.solvers.ADMM(x0, REG, RHO, n_cg=10, scheme=scheme, persistent=True, **kw)
    b = pytv.solvers.ADMM(x0, REG, RHO, n_cg=10, scheme=scheme, persistent=False, fused=False, **kw)
    assert a.small and not b.small and not a.fused and not b.fused
    la, lb = a.run(50), b.run(50, graph=False)
    print("max relative loss deviation %s: %.3e" % (scheme, np.max(np.abs(la - lb) / np.abs(lb))))
    np.testing.assert_allclose(la, lb, rtol=2e-6)
    np.testing.assert_allclose(a.result().cpu().numpy(), b.result().cpu().numpy(), rtol=0, atol=2e-3)
    np.testing.assert_allclose(a.u.cpu().numpy(), b.u.cpu().numpy(), rtol=0, atol=2e-3)
    np.testing.assert_allclose(a.z.cpu().numpy(), b.z.cpu().numpy(), rtol=0, atol=2e-3)


def _golden_image():
    return np.load(os.path.join(GOLDEN, "trajectories_2d.npz"))["noisy"]          # (1, 1, 64, 64): input data only


@pytest.mark.parametrize("scheme", ["hybrid", "central"])
def test_300_outer_iterations_are_two_launches_and_a_tail(pytv, scheme):
    """SMALL_BLOCK = 128: the state carried from launch to launch is x, t, u in memory"""
    import torch
    x0 = torch.as_tensor(_golden_image().astype(np.float32)).cuda()
    a = pytv.solvers.ADMM(x0, REG, RHO, n_cg=4, scheme=scheme, persistent=True)
    b = pytv.solvers.ADMM(x0, REG, RHO, n_cg=4, scheme=scheme, persistent=False, fused=False)
    assert a.small and a.SMALL_BLOCK == 128
    la, lb = a.run(300), b.run(300, graph=False)
    np.testing.assert_allclose(la, lb, rtol=2e-6)
    np.testing.assert_allclose(a.result().cpu().numpy(), b.result().cpu().numpy(), rtol=0, atol=2e-3)


def test_run_blocks_and_single_steps_share_the_state(pytv):
    import torch
    x0 = torch.as_tensor(_golden_image().astype(np.float32)).cuda()
    a = pytv.solvers.ADMM(x0, REG, RHO, n_cg=4, persistent=True)
    b = pytv.solvers.ADMM(x0, REG, RHO, n_cg=4, persistent=False, fused=False)
    rows = torch.zeros((3, 2), dtype=torch.float64, device="cuda")
    parts = [a.run(3)]
    a.step(rows[0])
    parts.append(a.run(2))
    a.step(rows[1])
    a.step(rows[2])
    parts.append(a.run(1))
    h = rows.cpu().numpy()
    single = 0.5 * h[:, 1] + REG * h[:, 0]
    got = np.concatenate([parts[0], single[0:1], parts[1], single[1:3], parts[2]])
    want = b.run(9, graph=False)
    np.testing.assert_allclose(got, want, rtol=2e-6)
    np.testing.assert_allclose(a.result().cpu().numpy(), b.result().cpu().numpy(), rtol=0, atol=2e-3)


def _cabi_setup(shape=(3, 2, 12, 16)):
    import torch
    from pytv import _native as nv
    lib = nv.lib()
    rng = np.random.default_rng(2)
    x0 = torch.as_tensor((100.0 * rng.random(shape)).astype(np.float32)).cuda()
    geo = nv.Geometry(shape, "hybrid", x0.dtype, x0.device, 1.0, 1.0, False, 0)
    nbytes = lib.tv_small_workspace_bytes(geo.ref, 8)
    coef = [(0.5, 0.0), (0.4, 0.1), (0.35, 0.12)]
    al = (ctypes.c_double * 3)(*[c[0] for c in coef])
    be = (ctypes.c_double * 3)(*[c[1] for c in coef])
    return torch, nv, lib, x0, geo, nbytes, al, be


def test_one_workspace_serves_the_three_loops_in_any_order():
    """the epoch bookkeeping: tv_small_cp, tv_small_admm, tv_small_subgrad_descent, tv_small_admm on ONE zero-filled workspace; each result
    equals the same call on a fresh workspace bit for bit"""
    torch, nv, lib, x0, geo, nbytes, al, be = _cabi_setup()
    st = nv.current_stream(x0.device)
    nz = x0.shape[0]

    def new_ws():
        return torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")

    def cp(ws, n):
        x, p, q = x0.clone(), torch.zeros_like(x0), geo.new_grad()
        h = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        assert lib.tv_small_cp(geo.ref, nv.ptr(x), nv.ptr(x0), nv.ptr(p), nv.ptr(q), 0.1, 25.0, 0.1, 1.0, n, h.data_ptr(), 2, 1, nv.ptr(ws), st) == 0
        return [h, x, p, q]

    def sg(ws, n):
        x, xa, nrm = x0.clone(), torch.zeros_like(x0), geo.new_image(nz + 2)
        h = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        assert lib.tv_small_subgrad_descent(geo.ref, nv.ptr(x), nv.ptr(xa), nv.ptr(x0), nv.ptr(nrm), 5e-3, 25.0, n, h.data_ptr(), 2, 1, nv.ptr(ws), st) == 0
        return [h, x, xa]

    def admm(ws, n, K):
        x, t, u, g = x0.clone(), geo.new_grad(), geo.new_grad(), geo.new_grad()
        r, ea, eb = torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
        h = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        assert lib.tv_small_admm(geo.ref, nv.ptr(x), nv.ptr(x0), nv.ptr(t), nv.ptr(u), nv.ptr(r), nv.ptr(ea), nv.ptr(eb), nv.ptr(g), 0.05, 500.0,
                                 al, be, K, n, h.data_ptr(), 2, 1, nv.ptr(ws), st) == 0, lib.tv_last_error()
        return [h, x, t, u]

    calls = [lambda ws: cp(ws, 7), lambda ws: admm(ws, 5, 3), lambda ws: sg(ws, 4), lambda ws: admm(ws, 8, 2), lambda ws: cp(ws, 3)]
    shared = new_ws()
    for i, call in enumerate(calls):
        got, want = call(shared), call(new_ws())
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.isfinite(a).all()
            assert torch.equal(a, b), "call %d differs on the shared workspace" % i
    assert int(shared.view(torch.int32)[8192 * 32 + 1].item()) == 0          # nobody abandoned a launch
    # the epoch line: 2 per CP / descent iteration, 1 + 2 K n_outer per ADMM call
    assert int(shared.view(torch.int32)[8192 * 32].item()) == 2 * 7 + (1 + 2 * 3 * 5) + 2 * 4 + (1 + 2 * 2 * 8) + 2 * 3


def test_c_abi_argument_checks():
    torch, nv, lib, x0, geo, nbytes, al, be = _cabi_setup((3, 2, 8, 8))
    st = nv.current_stream(x0.device)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    h = torch.zeros(16, dtype=torch.float64, device="cuda")
    x, r, ea, eb = x0.clone(), torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
    t, u, g = geo.new_grad(), geo.new_grad(), geo.new_grad()
    arrays = [x, x0, t, u, r, ea, eb, g]
    before = [a.clone() for a in arrays]

    def call(geom=geo, arr=None, rho=0.05, thresh=500.0, alpha=al, beta=be, K=3, n=2, hist=h.data_ptr(), stride=2, off=1, wsp=None):
        p = [nv.ptr(a) for a in arrays] if arr is None else arr
        return lib.tv_small_admm(geom.ref, *p, rho, thresh, alpha, beta, K, n, hist, stride, off, nv.ptr(ws) if wsp is None else wsp, st)

    for i in range(8):                                   # every array NULL in turn
        p = [nv.ptr(a) for a in arrays]
        p[i] = None
        assert call(arr=p) == -1 and b"NULL" in lib.tv_last_error()
    assert call(alpha=None) == -1 and b"NULL" in lib.tv_last_error()
    assert call(beta=None) == -1 and b"NULL" in lib.tv_last_error()
    assert call(hist=None) == -1 and b"NULL" in lib.tv_last_error()
    assert call(wsp=0) == -1 and b"NULL" in lib.tv_last_error()
    p = [nv.ptr(a) for a in arrays]
    p[5] = p[6]
    assert call(arr=p) == -1 and b"different" in lib.tv_last_error()
    for rho in (0.0, -1.0, float("nan")):
        assert call(rho=rho) == -1 and b"rho" in lib.tv_last_error()
    assert call(thresh=-1e-3) == -1 and b"thresh" in lib.tv_last_error()
    for K in (0, -2, 33):
        assert call(K=K) == -1 and b"n_cheb" in lib.tv_last_error()
    for n in (0, -1):
        assert call(n=n) == -1 and b"n_outer" in lib.tv_last_error()
    for stride, off in ((2, 2), (2, 0), (2, -1), (0, 1)):
        assert call(stride=stride, off=off) == -1 and b"fid_offset" in lib.tv_last_error()
    slab = nv.Geometry(tuple(x0.shape), "hybrid", x0.dtype, x0.device, 1.0, 1.0, False, 0, nz_global=6, z0=3)
    assert lib.tv_small_supported(slab.ref) == 0
    assert call(geom=slab) == -1 and b"unsharded" in lib.tv_last_error()
    torch.cuda.synchronize()
    # none of them launched: arrays, history and workspace are untouched
    for a, b in zip(arrays, before):
        assert torch.equal(a, b)
    assert not h.any() and not ws.any()
    assert call(K=3, n=2) == 0                           # and the same arguments without a fault run
    torch.cuda.synchronize()
    assert torch.isfinite(h[:4]).all() and h[:4].abs().min() > 0


def test_defaults_are_unchanged_and_requests_are_checked(pytv):
    import torch
    from pytv.slab import Slab
    x_small = torch.rand((4, 2, 32, 32), device="cuda")
    kw = dict(reg_time=1.0)
    ad = pytv.solvers.ADMM(x_small, 1.0, 0.1, **kw)
    assert ad.small is False
    assert pytv.solvers.ADMM(x_small, 1.0, 0.1, persistent=False, **kw).small is False
    ap = pytv.solvers.ADMM(x_small, 1.0, 0.1, persistent=True, **kw)
    assert ap.small and not ap.fused
    ap.timing = []                                       # per-step events: the ordinary path runs
    assert not ap._small_now()
    ap.run(2)
    assert len(ap.timing) == 2
    for bad, word in ((dict(x_solver="cg"), "Chebyshev"), (dict(single_reduction=False), "single_reduction"), (dict(fused=True), "fused"),
                      (dict(n_cg=0), "n_cg"), (dict(n_cg=33), "33|32")):
        with pytest.raises(ValueError, match=word):
            pytv.solvers.ADMM(x_small, 1.0, 0.1, persistent=True, **bad, **kw)
    with pytest.raises(ValueError, match="tv_small_supported"):
        pytv.solvers.ADMM(torch.rand((20, 4, 256, 256), device="cuda"), 1.0, 0.1, persistent=True, **kw)          # 5.2 Mvoxel
    with pytest.raises(ValueError, match="unsharded"):
        pytv.solvers.ADMM(x_small, 1.0, 0.1, persistent=True, slab=Slab(8, rank=0, world=2), **kw)


def test_ragged_rows_pitch_and_a_weight_volume(pytv):
    """scalar lanes (Nx = 13, dense), an explicit (row, frame) pitch, a per-voxel time-weight volume -- each against the oracle"""
    kw = dict(reg_z_over_reg=1.0, reg_time=1.0)
    for dtype in (np.float64, np.float32):
        _against_oracle(pytv, _noisy((3, 2, 7, 13), 5, dtype), 6, 3, "hybrid", kw, dtype, pitch=None)
        _against_oracle(pytv, _noisy((3, 2, 7, 13), 5, dtype), 6, 3, "central", kw, dtype, pitch=(16, 7 * 16 + 16))
        shape = (4, 3, 9, 12)
        wv = (0.5 + 2.0 * np.random.default_rng(8).random(shape)).astype(dtype)
        _against_oracle(pytv, _noisy(shape, 5, dtype), 6, 3, "upwind", dict(kw, mask_static=wv), dtype)
        _against_oracle(pytv, _noisy(shape, 5, dtype), 6, 3, "hybrid", dict(kw, mask_static=wv), dtype)
