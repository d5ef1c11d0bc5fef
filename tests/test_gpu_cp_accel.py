"""The accelerated Chambolle-Pock iteration on the GPU (``-m gpu``): tv_cp_primal_accel through the C-ABI against the fp64 oracle (``orc.D_T``
on the same inputs, up-cast for fp32), z-ranges against the whole volume, the plane-marching form against the one-site form, and
``AcceleratedChambollePock`` against a NumPy restatement of Algorithm 2 of Chambolle & Pock 2011 built on ``orc.D`` / ``orc.D_T`` -- its
trajectory, that it accelerates, ``run_until`` and the ``accelerated`` keyword of ``denoise_tv_chambolle``.

Tolerances are the project's (tests/test_gpu_parity.py): arrays to rtol 1e-5 (fp32) / 1e-11 (fp64) of max|x|, scalars to the same rtol of the
reference."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
DTYPES = [np.float64, np.float32]
LAM = 5.0


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _storage(t):
    """the whole allocation behind a (possibly pitched) view, pads included"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def _z_channels(scheme):
    per = 2 if scheme == "hybrid" else 1
    return 2 * per, 2 * per + (1 if scheme == "hybrid" else 0)        # (adjoint looks backwards, forwards): pytv/slab.py HaloPlan


def _case_kw(name, shape):
    """the four weightings of tests/test_gpu_dual_gap.py"""
    rng = np.random.default_rng(17)
    if name == "mask":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=rng.random((1, 1) + shape[2:]) < 0.4, factor_reg_static=3.0)
    if name == "time_factor":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random((1, 1) + shape[2:])))
    if name == "weight_vol":
        return dict(reg_z_over_reg=0.7, reg_time=0.25, mask_static=(0.25 + 2.0 * rng.random(shape)))
    return dict(reg_z_over_reg=0.7, reg_time=0.25)


WEIGHTINGS = ("plain", "mask", "time_factor", "weight_vol")
PLAIN_KW = dict(reg_z_over_reg=0.7, reg_time=0.25)


def make_inputs(shape, scheme, dtype, kw, seed=5):
    rng = np.random.default_rng(seed)
    x = (60.0 * rng.random(shape)).astype(dtype)
    x0 = (60.0 * rng.random(shape)).astype(dtype)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = rng.standard_normal((shape[0], nd) + tuple(shape[1:]))
    n = np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    q = (q / np.maximum(n, 1e-30) * (LAM * np.minimum(1.0, 1.5 * rng.random(n.shape)))).astype(dtype)     # |q|_2 <= LAM per site
    return x, q, x0


def ref_primal(x, gd, x0, tau, theta):
    """(x_new, x_bar, fid) in fp64 from gd = D^T q"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    xn = (x - tau * gd + tau * x0) / (1.0 + tau)
    return xn, xn + theta * (xn - x), float(0.5 * np.sum((xn - x0) ** 2))


def gpu_primal(x, q, x0, tau, theta, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None):
    """tv_cp_primal_accel on local planes [a, b) of the arrays (whole volume by default), halo planes passed by hand.  Returns
    (x_new, x_bar, fid) as numpy / float.  keep: receives the device tensors and copies of their storage made before the call.
    drop_halo: "prev" / "next" -- pass NULL for that halo plane."""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = nv.Geometry((b - a,) + tuple(x.shape[1:]), scheme, _tdt(dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1],
                    **({k: (v[a:b] if (isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg and v.dtype != bool) else v) for k, v in kw.items()}))

    def img(arr):
        t = g.new_image(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    def grad(arr):
        t = g.new_grad(arr.shape[0])
        t.copy_(torch.as_tensor(np.ascontiguousarray(arr)))
        return t

    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), x_bar=img(np.full_like(x[a:b], 7.0)), q=grad(q[a:b]), x0=img(x0[a:b]),
               qp=img(q[a - 1:a, cb]) if (a > 0 and g.z_active and drop_halo != "prev") else None,
               qn=img(q[b:b + 1, cf]) if (b < nzg and g.z_active and drop_halo != "next") else None)
    before = {k: _storage(v).clone() for k, v in dev.items() if v is not None}
    if keep is not None:
        keep.update(dev=dev, before=before)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_primal_accel(g.ref, nv.ptr(dev["q"]), nv.ptr(dev["qp"]), nv.ptr(dev["qn"]), nv.ptr(dev["x"]), nv.ptr(dev["x_bar"]),
                                         nv.ptr(dev["x0"]), float(tau), float(theta), out.data_ptr(), nv.ptr(g.workspace()),
                                         nv.current_stream(g.device)))
    return dev["x"].cpu().numpy(), dev["x_bar"].cpu().numpy(), float(out.item())


def _inputs_untouched(keep):
    for k in ("q", "x0", "qp", "qn"):
        if keep["dev"][k] is not None:
            assert torch.equal(_storage(keep["dev"][k]), keep["before"][k]), k          # the whole allocation: pad columns included


def _pads_are_zero(t):
    pads = _storage(t).clone()
    pads.as_strided(t.shape, t.stride()).zero_()
    assert not bool(pads.any())                                        # what is not a voxel is a pad


# ------------------------------------------------------------------------------------------------
# 1. entry-point parity against the oracle
# ------------------------------------------------------------------------------------------------
# scalar rows, 2-D | 16-byte lanes | two-plane z (central: forward stencil) | M > 8
PARITY_SHAPES = [(1, 1, 9, 13), (3, 2, 16, 20), (2, 3, 12, 16), (4, 9, 8, 16)]


def _explicit_pitch(shape, dtype):
    lane = 16 // np.dtype(dtype).itemsize
    rp = -(-(shape[3] + 4) // lane) * lane                              # nx + 4 rounded up to 16 bytes
    return rp, shape[2] * rp + 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_entry_point_matches_the_oracle(shape, scheme, dtype):
    tau = 0.3
    for weighting in WEIGHTINGS:
        kw = _case_kw(weighting, shape)
        x, q, x0 = make_inputs(shape, scheme, dtype, kw)
        gd = orc.D_T(q.astype(np.float64), scheme, **kw)                # once per weighting: shared by the pitches and the thetas
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            for theta in (0.0, 0.37, 1.0):
                what = "%s %s pitch %r theta %g" % (weighting, scheme, pitch, theta)
                keep = {}
                xn, xb, fid = gpu_primal(x, q, x0, tau, theta, scheme, dtype, kw, pitch=pitch, keep=keep)
                wxn, wxb, wfid = ref_primal(x, gd, x0, tau, theta)
                tol = RTOL[dtype] * float(np.max(np.abs(wxn)))
                print("%s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  fid rel %.3e" % (what, np.max(np.abs(xn - wxn)), np.max(np.abs(xb - wxb)), tol,
                                                                                         abs(fid - wfid) / wfid))
                assert xn.dtype == dtype and xb.dtype == dtype
                assert float(np.max(np.abs(xn - wxn))) <= tol, what
                assert float(np.max(np.abs(xb - wxb))) <= tol, what
                assert abs(fid - wfid) <= RTOL[dtype] * wfid, what
                if theta == 0.0:
                    np.testing.assert_array_equal(xb, xn, err_msg=what)       # x_bar = x_new exactly
                _inputs_untouched(keep)
                if pitch != (0, 0):
                    _pads_are_zero(keep["dev"]["x"])
                    _pads_are_zero(keep["dev"]["x_bar"])


# ------------------------------------------------------------------------------------------------
# 2. z-ranges: planes [a, b) with hand-made halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_z_ranges_equal_the_whole_volume(scheme, dtype):
    shape, tau, theta = (5, 2, 16, 20), 0.3, 0.37
    x, q, x0 = make_inputs(shape, scheme, dtype, PLAIN_KW)
    wxn, wxb, wfid = gpu_primal(x, q, x0, tau, theta, scheme, dtype, PLAIN_KW)
    for cut in ((0, 1, 5), (0, 2, 5), (0, 1, 4, 5)):
        fids = []
        for a, b in zip(cut[:-1], cut[1:]):
            keep = {}
            xn, xb, fid = gpu_primal(x, q, x0, tau, theta, scheme, dtype, PLAIN_KW, z_range=(a, b), keep=keep)
            np.testing.assert_array_equal(xn, wxn[a:b], err_msg="x, cut %r planes [%d, %d)" % (cut, a, b))
            np.testing.assert_array_equal(xb, wxb[a:b], err_msg="x_bar, cut %r planes [%d, %d)" % (cut, a, b))
            _inputs_untouched(keep)                                    # q, x0 and the halo planes
            fids.append(fid)
        print("cut %r: fid parts %r sum %.17g whole %.17g" % (cut, fids, sum(fids), wfid))
        assert abs(sum(fids) - wfid) <= 1e-13 * wfid, cut


@pytest.mark.parametrize("scheme", SCHEMES)
def test_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    shape = (5, 2, 16, 20)
    x, q, x0 = make_inputs(shape, scheme, np.float32, PLAIN_KW)
    # the adjoint of a forward difference reads the previous slab, of a backward difference the next one (central, hybrid: both)
    sides = {"upwind": ("prev",), "downwind": ("next",)}.get(scheme, ("prev", "next"))
    for side in sides:
        keep = {}
        with pytest.raises(ValueError, match=r"halo.*code -2"):
            gpu_primal(x, q, x0, 0.3, 0.37, scheme, np.float32, PLAIN_KW, z_range=(1, 4), keep=keep, drop_halo=side)
        torch.cuda.synchronize()
        for k, t in keep["dev"].items():
            if t is not None:
                assert torch.equal(_storage(t), keep["before"][k]), k


# ------------------------------------------------------------------------------------------------
# 3. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_marching_form_equals_one_site_form(scheme, tvopt):
    shape, dtype, tau, theta = (2, 2, 1024, 1024), np.float32, 0.3, 0.37
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, shape[0], shape[1], **PLAIN_KW)
    x = 60.0 * rng.random(shape, dtype=np.float32)
    x0 = 60.0 * rng.random(shape, dtype=np.float32)
    q = LAM * (rng.random((shape[0], nd) + shape[1:], dtype=np.float32) - 0.5)
    march = gpu_primal(x, q, x0, tau, theta, scheme, dtype, PLAIN_KW)
    tvopt("TV_NO_MARCH", 1)
    site = gpu_primal(x, q, x0, tau, theta, scheme, dtype, PLAIN_KW)
    tol = 1e-5 * float(np.max(np.abs(site[0])))
    print("%s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  fid %.9e / %.9e" % (scheme, np.max(np.abs(march[0] - site[0])),
                                                                              np.max(np.abs(march[1] - site[1])), tol, march[2], site[2]))
    assert float(np.max(np.abs(march[0] - site[0]))) <= tol
    assert float(np.max(np.abs(march[1] - site[1]))) <= tol
    assert abs(march[2] - site[2]) <= 1e-5 * site[2]
    assert np.isfinite(march[2]) and march[2] > 0.0


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 2 with gamma-strong convexity of the fidelity)
# ------------------------------------------------------------------------------------------------
def np_accel(x0, n_iter, lam, scheme, kw, tau0=None, sigma0=None, gamma=1.0, want_q=False):
    x0 = np.asarray(x0, dtype=np.float64)
    L2 = orc.normal_spectral_bound(scheme, x0.shape, **kw)
    tau = 1.0 / np.sqrt(L2) if tau0 is None else float(tau0)
    sigma = 1.0 / np.sqrt(L2) if sigma0 is None else float(sigma0)
    x, xb = x0.copy(), x0.copy()
    q = np.zeros_like(orc.D(x0, scheme, **kw))
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        v = q + sigma * Dxb
        q = v / np.maximum(1.0, np.sqrt(np.sum(v ** 2, axis=1, keepdims=True)) / lam)
        xn = (x - tau * orc.D_T(q, scheme, **kw) + tau * x0) / (1.0 + tau)
        theta = 1.0 / np.sqrt(1.0 + 2.0 * gamma * tau)
        xb = xn + theta * (xn - x)
        x = xn
        loss[k] = 0.5 * np.sum((x - x0) ** 2) + lam * orc.compute_L21_norm(Dxb)
        tau, sigma = theta * tau, sigma / theta
    return (x, loss, q) if want_q else (x, loss)


def np_gap(x, q, x0, lam, scheme, kw):
    """(primal, gap) in fp64, the gap in its site-wise form"""
    Dx = orc.D(x, scheme, **kw)
    gd = orc.D_T(q, scheme, **kw)
    nrm = np.sqrt(np.sum(Dx * Dx, axis=1))
    gap = np.sum(0.5 * (x - x0 + gd) ** 2) + np.sum(lam * nrm - np.sum(q * Dx, axis=1))
    return float(0.5 * np.sum((x - x0) ** 2) + lam * np.sum(nrm)), float(gap)


@functools.lru_cache(maxsize=None)
def square_plus_noise(shape):
    """a centred square of height 100 plus 100 * default_rng(0).random(shape)"""
    x = np.zeros(shape)
    ny, nx = shape[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    x = x + 100.0 * np.random.default_rng(0).random(shape)
    x.setflags(write=False)
    return x


def _kw_of(shape):
    return dict(reg_z_over_reg=0.7, reg_time=0.25) if shape[0] > 1 else dict()


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, n_iter, gamma=1.0, f32_input=False):
    x0 = square_plus_noise(shape)
    if f32_input:
        x0 = x0.astype(np.float32).astype(np.float64)
    return np_accel(x0, n_iter, 25.0, scheme, _kw_of(shape), gamma=gamma)


def _solver(pytv, shape, dtype, scheme, **how):
    return pytv.solvers.AcceleratedChambollePock(torch.as_tensor(square_plus_noise(shape).astype(dtype)).cuda(), 25.0, scheme=scheme,
                                                 **_kw_of(shape), **how)


# ------------------------------------------------------------------------------------------------
# 4. solver trajectory
# ------------------------------------------------------------------------------------------------
TRAJ_SHAPES = [(1, 1, 24, 28), (3, 2, 16, 20)]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme):
    import pytv
    wx, wloss = np_trajectory(shape, scheme, 40)
    cp = _solver(pytv, shape, np.float64, scheme)
    assert cp.it == 0 and cp.gamma == 1.0 and cp.tau0 == cp.sigma0 and abs(cp.tau0 * cp.sigma0 * cp.L2 - 1.0) <= 1e-15
    assert cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape))
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(square_plus_noise(shape))))
    assert cp.it == 40
    # two calls continue the schedule: run(15); run(25) is run(40) bit for bit
    two = _solver(pytv, shape, np.float64, scheme)
    l2 = np.concatenate([two.run(15), two.run(25)])
    np.testing.assert_array_equal(l2, loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.x_bar, cp.x_bar) and torch.equal(two.q, cp.q)
    # reset() reproduces the run; record_loss=False returns nothing and computes the same
    two.reset()
    assert two.it == 0 and torch.equal(two.x, two.x0) and torch.equal(two.x_bar, two.x0) and not bool(two.q.any())
    assert two.run(40, record_loss=False) is None
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.q, cp.q)
    two.reset()
    np.testing.assert_array_equal(two.run(40), loss)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme):
    """the tolerance tests/test_gpu_parity.py gives fp32 ``ChambollePock`` trajectories against the fp64 oracle
    (test_cp_3d_4d_matches_oracle: loss rtol 1e-5; result rtol 1e-5, atol 2e-3 for pixel values of O(100))"""
    import pytv
    wx, wloss = np_trajectory(shape, scheme, 40, f32_input=True)
    cp = _solver(pytv, shape, np.float32, scheme)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_gamma_zero_is_the_constant_step_loop(scheme):
    import pytv
    shape = (3, 2, 16, 20)
    wx, wloss = np_trajectory(shape, scheme, 40, gamma=0.0)
    cp = _solver(pytv, shape, np.float64, scheme, gamma=0.0)
    loss = cp.run(40)
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(cp.result().cpu().numpy() - wx))) <= 1e-9 * float(np.max(np.abs(square_plus_noise(shape))))


def test_constructor_refuses_steps_beyond_the_bound_and_a_forced_divergence_returns_numbers():
    import pytv
    shape = (1, 1, 24, 28)
    x0 = torch.as_tensor(square_plus_noise(shape).copy()).cuda()
    L2 = 8.0
    with pytest.raises(ValueError, match="tau0"):
        pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme="upwind", tau0=1.0, sigma0=(1.0 + 1e-9) / L2)
    ok = pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme="upwind", tau0=1.0, sigma0=1.0 / L2)
    assert ok.L2 == L2
    half = pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme="upwind", tau0=0.25)
    assert half.sigma0 == 1.0 / (L2 * 0.25)
    # steps forced past the bound after construction, constant (gamma = 0): the run does not converge (q is a projection, so the iterates
    # stay bounded and oscillate; the NumPy loop ends with gap > primal) and returns what it computed
    bad = pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme="upwind", gamma=0.0)
    bad.tau0, bad.sigma0 = 40.0, 40.0
    loss = bad.run(400)
    primal, dual, gap = bad.duality_gap()                               # numbers, no exception
    print("forced steps: loss tail %r primal %.6e gap %.6e" % (loss[-3:], primal, gap))
    assert loss.shape == (400,) and isinstance(primal, float) and isinstance(gap, float)
    assert not gap <= 0.1 * primal


# ------------------------------------------------------------------------------------------------
# 5. it accelerates
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(1, 1, 48, 48), (6, 3, 24, 24)])
def test_gap_after_150_iterations_against_the_plain_loop(shape, scheme):
    """CPU / oracle figures for gap_plain / gap_accel after 150 iterations: (1,1,48,48) upwind 12.9, downwind 11.5, hybrid 17, central 1.9;
    (6,3,24,24): 16 - 25, central 1.4.  The condition: 5 times for the one-sided schemes, 1 for central."""
    import pytv
    x0 = torch.as_tensor(square_plus_noise(shape).copy()).cuda()
    kw = _kw_of(shape)
    acc = pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme=scheme, **kw)
    plain = pytv.solvers.ChambollePock(x0, 25.0, scheme=scheme, fused=False, persistent=False, **kw)
    acc.run(150)
    plain.run(150)
    pa, _, ga = acc.duality_gap()
    pp, _, gp = plain.duality_gap()
    print("%s %s: rel gap plain %.3e accelerated %.3e ratio %.2f" % (scheme, shape, gp / pp, ga / pa, gp / ga))
    assert ga > 0.0 and gp > 0.0
    assert ga <= (gp if scheme == "central" else gp / 5.0)


# ------------------------------------------------------------------------------------------------
# 6. run_until
# ------------------------------------------------------------------------------------------------
def test_run_until_certifies_in_fewer_iterations():
    """oracle figures: at most 100 accelerated iterations against at least 110 plain ones"""
    import pytv
    shape, scheme = (1, 1, 48, 48), "hybrid"
    x0 = torch.as_tensor(square_plus_noise(shape).copy()).cuda()
    x_star = np_trajectory(shape, scheme, 2000)[0]
    infos = {}
    for name, cp in (("accelerated", pytv.solvers.AcceleratedChambollePock(x0, 25.0, scheme=scheme)),
                     ("plain", pytv.solvers.ChambollePock(x0, 25.0, scheme=scheme, fused=False, persistent=False))):
        loss, info = cp.run_until(1e-3, 300, check_every=10)
        dist = float(np.sqrt(np.sum((cp.result().cpu().numpy() - x_star) ** 2)))
        print(name, info, "|x - x*| = %.6e" % dist)
        assert info["converged"] is True and info["iterations"] % 10 == 0 and len(loss) == info["iterations"] == cp.it
        assert info["gap"] <= 1e-3 * info["primal"]
        assert info["error_bound"] == np.sqrt(2 * info["gap"]) and info["error_bound"] >= dist
        infos[name] = info
    assert infos["accelerated"]["iterations"] < infos["plain"]["iterations"]


# ------------------------------------------------------------------------------------------------
# 7. front-end
# ------------------------------------------------------------------------------------------------
def test_denoise_tv_chambolle_accelerated_keyword():
    """both paths stop with a certificate |u - u*|_2 <= error_bound of their own, so the two results are at most the sum of the two bounds
    apart (triangle inequality); the keyword's default leaves the front-end as it was, bit for bit"""
    import pytv
    img = np.load(os.path.join(GOLDEN, "cameraman.npz"))["image"].astype(np.float64) / 255.0
    noisy_img = img + 0.1 * np.random.default_rng(0).standard_normal(img.shape)
    weight = 0.1
    vol = torch.as_tensor(noisy_img.reshape(1, 1, *img.shape)).cuda()
    fast = pytv.denoise_tv_chambolle(noisy_img, weight, rel_gap=1e-3, max_num_iter=2000, accelerated=True)
    slow = pytv.denoise_tv_chambolle(noisy_img, weight, rel_gap=1e-3, max_num_iter=2000)
    acc = pytv.solvers.AcceleratedChambollePock(vol, weight, scheme="upwind", reg_z_over_reg=1.0)
    _, ia = acc.run_until(1e-3, 2000)
    ref = pytv.solvers.ChambollePock(vol, weight, scheme="upwind", reg_z_over_reg=1.0)
    _, ip = ref.run_until(1e-3, 2000)
    assert ia["converged"] and ip["converged"] and ia["iterations"] < ip["iterations"]
    np.testing.assert_array_equal(fast, acc.result().cpu().numpy().reshape(img.shape))       # the front-end is that loop
    np.testing.assert_array_equal(slow, ref.result().cpu().numpy().reshape(img.shape))
    dist = float(np.sqrt(np.sum((fast - slow) ** 2)))
    print("accelerated", ia, "plain", ip, "|fast - slow| = %.6e" % dist)
    assert dist <= ia["error_bound"] + ip["error_bound"]
    # accelerated=False is the call without the keyword
    np.testing.assert_array_equal(pytv.denoise_tv_chambolle(noisy_img, weight, accelerated=False), pytv.denoise_tv_chambolle(noisy_img, weight))
    np.testing.assert_array_equal(pytv.denoise_tv_chambolle(noisy_img, weight, rel_gap=1e-3, max_num_iter=2000, accelerated=False), slow)
