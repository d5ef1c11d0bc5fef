"""The reduction workspace on the GPU (``-m gpu``): every slot of csrc/tv_host.h's ``Partials`` and the stage words of the two-level
reduction, at the smallest shapes that reach them, with a guard band behind ``tv_workspace_bytes``.

  1. (520, 8, 16, 64) fp32 hybrid with TV_NO_MARCH=1: the one-site kernels launch one block per frame, 4160 blocks -- more than the 4096
     above which the reduction goes through the stage words.  tv_dual_gap (slots 0, 1, 2), tv_normal_op2 with b (the composition:
     tv_normal_op, tv_dot, k_sub_dot) and tv_cheb_step with and without ``dots`` (the spare word), each scalar against the fp64 oracle at
     the tolerance of the test that owns the quantity (test_gpu_dual_gap.check, test_gpu_admm_ops: 1e-5, test_gpu_admm_fused: 3e-5 * 100).
  2. (24, 8, 64, 128), the one-sweep path against the two-kernel path on the same data: tv_cp_sweep with TV_CP_FID_OF_INPUT |
     TV_CP_FID_BOTH (slots 0, 1, 2) + tv_cp_fixup with x0 against tv_cp_dual + tv_cp_primal -- the TV, the fidelity of x_out (fid[1] + the
     fix-up's share) and x_out itself; tv_cpop_fused + tv_cpop_fixup (the spare word) against tv_cp_dual + tv_DT_axpy.  Scalars at
     test_gpu_cp_r4's rtol 1e-5, x_out at the tolerances tests/test_gpu_parity.py uses for the same comparisons (rtol 1e-5 with atol
     1e-3 for tv_cp_fused, 2e-3 for tv_cpop_fused).
"""
import numpy as np
import pytest
import torch

from oracle import tv_oracle as orc
from test_gpu_dual_gap import check, make_inputs, ref_gap

pytestmark = pytest.mark.gpu

KW = dict(reg_z_over_reg=0.7, reg_time=0.25)
GUARD, SENTINEL = 4096, 0xA5


def _guarded_ws(nv, g):
    n = nv.lib().tv_workspace_bytes(g.ref)
    assert n > 0 and n % 8 == 0
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, n


def _guard_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def test_one_site_forms_above_4096_blocks(tvopt):
    from pytv import _native as nv
    lib = nv.lib()
    tvopt("TV_NO_MARCH", 1)
    shape, scheme, dtype, lam = (520, 8, 16, 64), "hybrid", np.float32, 5.0
    g = nv.Geometry(shape, scheme, torch.float32, "cuda", **KW)
    buf, n = _guarded_ws(nv, g)
    ws, st = buf.data_ptr(), nv.current_stream(g.device)

    # tv_dual_gap: slots 0, 1, 2
    x, q, x0 = make_inputs(shape, scheme, dtype, KW, lam, 1.0)
    xd, qd, x0d = _dev(x), _dev(q), _dev(x0)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(lib.tv_dual_gap(g.ref, nv.ptr(xd), None, None, nv.ptr(qd), None, None, nv.ptr(x0d), lam, 1.0, out.data_ptr(), ws, st))
    check(tuple(out.cpu().tolist()), ref_gap(x, q, x0, lam, 1.0, scheme, KW), lam, dtype, "dual gap, 4160 blocks")
    assert _guard_intact(buf, n)

    # tv_normal_op2 with b: the composition path
    rng = np.random.default_rng(5)
    v, b, y = [(rng.standard_normal(shape) * 10).astype(dtype) for _ in range(3)]
    v64, b64 = v.astype(np.float64), b.astype(np.float64)
    dtd = orc.D_T(orc.D(v64, scheme, **KW), scheme, **KW)
    vd, bd, yd = _dev(v), _dev(b), _dev(y)
    o, o2 = torch.empty_like(vd), torch.empty_like(vd)
    dots = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(lib.tv_normal_op2(g.ref, nv.ptr(vd), None, None, 0.3, nv.ptr(bd), nv.ptr(o), nv.ptr(o2), dots.data_ptr(), ws, st))
    res = b64 - (v64 + 0.3 * dtd)
    d0, d1 = float(np.sum(res * res)), float(np.sum(v64 * v64))
    print("normal_op2 dots", dots.cpu().tolist(), (d0, d1))
    np.testing.assert_allclose(o.cpu().numpy(), res, rtol=1e-5, atol=2e-3)
    assert torch.equal(o, o2)
    assert abs(dots[0].item() - d0) <= 1e-5 * d0 and abs(dots[1].item() - d1) <= 1e-5 * d1
    assert _guard_intact(buf, n)

    # tv_cheb_step with dots, then with dots = NULL (the totals go to a spare word of the workspace)
    rho, alpha, beta, tol = 0.15, 0.8, 0.3, 3e-5
    res = b64 - (v64 + rho * dtd)
    want = v64 + alpha * res + beta * (v64 - y.astype(np.float64))
    oc = torch.empty_like(vd)
    sc = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(lib.tv_cheb_step(g.ref, nv.ptr(vd), None, None, rho, nv.ptr(bd), nv.ptr(yd), 0.0, None, None, alpha, beta, nv.ptr(oc), sc.data_ptr(), ws, st))
    print("cheb dots", sc.cpu().tolist(), (float(np.sum(res * res)), d1))
    np.testing.assert_allclose(oc.cpu().numpy(), want, rtol=0, atol=tol * 10 * max(1.0, np.abs(want).max()))
    np.testing.assert_allclose(sc[0].item(), np.sum(res * res), rtol=tol * 100)
    np.testing.assert_allclose(sc[1].item(), d1, rtol=tol * 100)
    oc2 = torch.full_like(vd, float("nan"))
    nv.check(lib.tv_cheb_step(g.ref, nv.ptr(vd), None, None, rho, nv.ptr(bd), nv.ptr(yd), 0.0, None, None, alpha, beta, nv.ptr(oc2), None, ws, st))
    assert torch.equal(oc2, oc)
    assert _guard_intact(buf, n)


def test_one_sweep_slots_and_spare_word(tvopt):
    from pytv import _native as nv
    lib = nv.lib()
    tvopt("TV_FUSED_MIN_KVOXELS", 0)
    shape, scheme, lam = (24, 8, 64, 128), "hybrid", 5.0
    g = nv.Geometry(shape, scheme, torch.float32, "cuda", **KW)
    assert lib.tv_cp_fused_supported(g.ref) == 1
    buf, n = _guarded_ws(nv, g)
    ws, st = buf.data_ptr(), nv.current_stream(g.device)
    rng = np.random.default_rng(9)
    x, x0 = _dev((60 * rng.random(shape)).astype(np.float32)), _dev((60 * rng.random(shape)).astype(np.float32))
    q, q2, p, xo = torch.zeros(g.grad_shape, device="cuda"), torch.zeros(g.grad_shape, device="cuda"), torch.zeros_like(x), torch.empty_like(x)
    tau, sigma_a = 0.05, 1.0
    # the two-kernel path on the same data: q <- proj(q + sigma D x), then p and x in place; the input's fidelity directly
    qk, pk, xk = torch.zeros(g.grad_shape, device="cuda"), torch.zeros_like(x), x.clone()
    two = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    wk = nv.ptr(g.workspace())
    nv.check(lib.tv_cp_dual(g.ref, nv.ptr(x), None, None, nv.ptr(qk), 0.5, lam, two[0:1].data_ptr(), wk, st))
    nv.check(lib.tv_cp_primal(g.ref, nv.ptr(qk), None, None, nv.ptr(xk), nv.ptr(x0), nv.ptr(pk), tau, sigma_a, two[1:2].data_ptr(), wk, st))
    tv2, fid2 = two.cpu().tolist()
    fid_in = 0.5 * torch.sum((x.double() - x0.double()) ** 2).item()

    sc = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(lib.tv_cp_sweep(g.ref, nv.ptr(x), None, None, nv.ptr(q), nv.ptr(q2), nv.ptr(x0), nv.ptr(p), nv.ptr(xo), 0.5, lam, tau, sigma_a, 3, 0, -1,
                             sc[0:1].data_ptr(), sc[1:3].data_ptr(), ws, st))
    nv.check(lib.tv_cp_fixup(g.ref, nv.ptr(q2), None, None, nv.ptr(xo), nv.ptr(x0), tau, 0, -1, sc[3:4].data_ptr(), ws, st))
    got = sc.cpu().tolist()
    print("sweep", got, "two-kernel tv, fid", (tv2, fid2), "fid of input", fid_in)
    assert abs(got[0] - tv2) <= 1e-5 * tv2                                 # slot 0
    assert abs(got[1] - fid_in) <= 1e-5 * fid_in                           # slot 1
    assert got[2] > 0 and got[3] > 0                                       # both the sweep and the fix-up complete some sites
    assert abs((got[2] + got[3]) - fid2) <= 1e-5 * fid2                    # slot 2 + the fix-up's slot 0: the fidelity of x_out
    np.testing.assert_allclose(xo.cpu().numpy(), xk.cpu().numpy(), rtol=1e-5, atol=1e-3)
    assert _guard_intact(buf, n)

    # operator form: its fix-up's sum goes to a spare word of the workspace.  Two-kernel path: x - tau atp - tau D^T q
    qo, xo2 = torch.zeros(g.grad_shape, device="cuda"), torch.empty_like(x)
    atp = _dev((rng.standard_normal(shape)).astype(np.float32))
    base, xk2 = x - tau * atp, torch.empty_like(x)
    nv.check(lib.tv_DT_axpy(g.ref, nv.ptr(qk), None, None, None, nv.ptr(base), -tau, nv.ptr(xk2), st))
    tvo = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(lib.tv_cpop_fused(g.ref, nv.ptr(x), None, None, nv.ptr(qo), nv.ptr(atp), nv.ptr(xo2), 0.5, lam, tau, 0, -1, tvo.data_ptr(), ws, st))
    nv.check(lib.tv_cpop_fixup(g.ref, nv.ptr(qo), None, None, nv.ptr(xo2), tau, 0, -1, ws, st))
    torch.cuda.synchronize()
    assert abs(tvo.item() - tv2) <= 1e-5 * tv2
    np.testing.assert_allclose(xo2.cpu().numpy(), xk2.cpu().numpy(), rtol=1e-5, atol=2e-3)
    assert _guard_intact(buf, n)
