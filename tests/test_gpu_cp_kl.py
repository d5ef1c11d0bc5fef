"""Chambolle-Pock with the Poisson / Kullback-Leibler data term on the GPU (``-m gpu``): tv_cp_primal_kl through the C-ABI against an fp64 NumPy
restatement of the step (the TEXTBOOK root (b + sqrt(b^2 + 4 tau x0)) / 2 on ``orc.D_T`` of the same inputs -- exact enough in fp64, while the
kernel takes the cancellation-free form), the exactness the stable form promises, the reduce-only residual mode, z-ranges against the whole
volume, the plane-marching form against the one-site form, and ``PoissonChambollePock`` / ``denoise_tv_poisson`` against a NumPy restatement of
Algorithm 1 of Chambolle & Pock 2011 built on ``orc.D`` / ``orc.D_T``.

Tolerances.  The arrays are held PER SITE: the global rtol * max|x| of the other kernel tests cannot tell the stable root from the textbook one
(both pass it).  With v = x - tau D^T q, b = v - tau, s = sqrt(b^2 + 4 tau x0):

    tol_i = RTOL x_new_i (1 + (max|v| + tau) / s_i)        RTOL = 1e-5 (fp32) / 1e-11 (fp64)

-- the rounding of b, of size RTOL (max|v| + tau), propagated to first order (d x_new / d b = x_new / s), plus a relative term.  A site with
x0 = 0 and b < 0 has tol_i = 0: the kernel returns an exact 0 there.
    x_bar      tol_i (1 + theta) + theta RTOL |x_i|
    F          sum_{x0 > 0} |1 - x0 / x_new| tol_i + RTOL sum_{x0 > 0} (|x_new - x0| + x0 |log(x0 / x_new)|) + sum_{x0 = 0} tol_i
               (dF / dx_new = 1 - x0 / x_new, plus the rounding of the two terms of F)
    R          2 sqrt(R_ref E) + E with E = sum (tol_i / tau)^2: a per-site error of tol_i in x_new (Cauchy-Schwarz)"""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc
from test_gpu_cp_prox import (DTYPES, EVERYTHING, INPUTS, LAM, PARITY_SHAPES, PLAIN_KW, RTOL, TAU, WEIGHTINGS, _case_kw, _explicit_pitch,
                              _kw_of, _pads_are_zero, _storage, _tdt, _untouched, _z_channels, make_inputs, np_project)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# the step, restated in fp64 with the textbook formula
# ------------------------------------------------------------------------------------------------
def kl_np(x, x0):
    """F(x) = sum (x - x0 + x0 log(x0 / x)), 0 log 0 = 0, +inf where x = 0 < x0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(x0 > 0, x0 * np.log(np.where(x0 > 0, x0, 1.0) / x), 0.0)
    return float(np.sum((x - x0) + t))


def prox_kl_np(v, x0, tau):
    b = v - tau
    return 0.5 * (b + np.sqrt(b * b + 4.0 * tau * x0))


def counts_by_quarters(shape, rng):
    """x0 by quarters of the sites: 0, integers 1 - 3, Poisson(30), Poisson(1e4) (all exact in fp32)"""
    which = rng.integers(0, 4, shape)
    x0 = np.zeros(shape)
    x0[which == 1] = rng.integers(1, 4, shape)[which == 1]
    x0[which == 2] = rng.poisson(30.0, shape)[which == 2]
    x0[which == 3] = rng.poisson(1.0e4, shape)[which == 3]
    return x0


@functools.lru_cache(maxsize=None)
def _inputs(shape, scheme, dtype, weighting):
    """x, q of tests/test_gpu_cp_prox.make_inputs (lambda = 5, tau = 0.3) with a third of the sites of x lowered by 80, so that b << 0 there;
    x0 by quarters.  Returns (x, q, x0, kw, ref) with the fp64 restatement ``ref`` of the step on exactly these (rounded) arrays."""
    kw = _case_kw(weighting, shape)
    x, q, _, gd = make_inputs(shape, scheme, dtype, kw)
    rng = np.random.default_rng(23)
    x = (x.astype(np.float64) - 80.0 * (rng.random(shape) < 1.0 / 3.0)).astype(dtype)
    x0 = counts_by_quarters(shape, rng).astype(dtype)
    for a in (x, q, x0):
        a.setflags(write=False)
    return x, q, x0, kw, reference(x, gd, x0, TAU, dtype)


def reference(x, gd, x0, tau, dtype):
    """everything the checks need, in fp64 from gd = D^T q: x_new, b, the per-site tolerance, F, R and their tolerances"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    v = x - tau * gd
    b = v - tau
    s = np.sqrt(b * b + 4.0 * tau * x0)
    xn = 0.5 * (b + s)
    rtol = RTOL[dtype]
    btol = rtol * (float(np.max(np.abs(v))) + tau)                          # the rounding of b
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = np.where(xn > 0, rtol * xn * (1.0 + (btol / rtol) / s), 0.0)
        pos = x0 > 0
        ftol = float(np.sum(np.abs(1.0 - x0[pos] / xn[pos]) * tol[pos]) + np.sum(tol[~pos])
                     + rtol * np.sum(np.abs(xn[pos] - x0[pos]) + x0[pos] * np.abs(np.log(x0[pos] / xn[pos]))))
    res = float(np.sum(((x - xn) / tau) ** 2))
    e = float(np.sum((tol / tau) ** 2))
    return dict(x=x, xn=xn, b=b, s=s, tol=tol, btol=btol, fid=kl_np(xn, x0), ftol=ftol, res=res, rtol_res=2.0 * np.sqrt(res * e) + e, rtol=rtol)


def gpu_kl(x, q, x0, tau, theta, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None, residual=False, null_x_bar=False,
           x_bar_fill=7.0):
    """tv_cp_primal_kl on local planes [a, b) of the arrays (whole volume by default), halo planes passed by hand.  Returns (x, x_bar, scalar)
    as numpy / float after the call.  keep: receives the device tensors and copies of their storage made before the call.  drop_halo: "prev" /
    "next" -- pass NULL for that halo plane.  residual: TV_CPP_RESIDUAL; null_x_bar: pass x_bar = NULL."""
    from pytv import _native as nv
    nzg = x.shape[0]
    a, b = (0, nzg) if z_range is None else z_range
    g = nv.Geometry((b - a,) + tuple(x.shape[1:]), scheme, _tdt(dtype), "cuda", nz_global=nzg, z0=a, row_pitch=pitch[0], frame_pitch=pitch[1],
                    **({k: (v[a:b] if (isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[0] == nzg and v.dtype != bool) else v) for k, v in kw.items()}))

    def img(arr):
        t = g.new_image(arr.shape[0])
        t.copy_(torch.as_tensor(np.array(arr)))                # a writable copy: the cached inputs are read-only
        return t

    def grad(arr):
        t = g.new_grad(arr.shape[0])
        t.copy_(torch.as_tensor(np.array(arr)))                # a writable copy: the cached inputs are read-only
        return t

    cb, cf = _z_channels(scheme)
    dev = dict(x=img(x[a:b]), x_bar=img(np.full_like(x[a:b], x_bar_fill)), q=grad(q[a:b]), x0=img(x0[a:b]),
               qp=img(q[a - 1:a, cb]) if (a > 0 and g.z_active and drop_halo != "prev") else None,
               qn=img(q[b:b + 1, cf]) if (b < nzg and g.z_active and drop_halo != "next") else None)
    before = {k: _storage(v).clone() for k, v in dev.items() if v is not None}
    if keep is not None:
        keep.update(dev=dev, before=before)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    nv.check(nv.lib().tv_cp_primal_kl(g.ref, nv.ptr(dev["q"]), nv.ptr(dev["qp"]), nv.ptr(dev["qn"]), nv.ptr(dev["x"]),
                                      None if null_x_bar else nv.ptr(dev["x_bar"]), nv.ptr(dev["x0"]), float(tau), float(theta),
                                      nv.TV_CPP_RESIDUAL if residual else 0, out.data_ptr(), nv.ptr(g.workspace()), nv.current_stream(g.device)))
    return dev["x"].cpu().numpy(), dev["x_bar"].cpu().numpy(), float(out.item())


def _same_bits(t, before):
    """bit for bit, NaN included (``torch.equal`` calls a poisoned array unequal to itself)"""
    return torch.equal(_storage(t).view(torch.uint8), before.view(torch.uint8))


def _untouched_bits(keep, names):
    for k in names:
        if keep["dev"][k] is not None:
            assert _same_bits(keep["dev"][k], keep["before"][k]), k


def _check_step(what, got, ref, theta):
    """x_new, x_bar and F of a step-mode call against the restatement, per site; prints each figure before it asserts"""
    xn, xb, fid = got
    tol = ref["tol"]
    wxb = ref["xn"] + theta * (ref["xn"] - ref["x"])
    btol = tol * (1.0 + theta) + theta * ref["rtol"] * np.abs(ref["x"])
    ex, eb = np.abs(xn - ref["xn"]), np.abs(xb - wxb)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst_x = float(np.max(np.where(tol > 0, ex / tol, np.where(ex > 0, np.inf, 0.0))))
        worst_b = float(np.max(np.where(btol > 0, eb / btol, np.where(eb > 0, np.inf, 0.0))))
    print("%s: max err / tol  x %.3e  x_bar %.3e;  |dF| %.3e (tol %.3e, F %.6e)" % (what, worst_x, worst_b, abs(fid - ref["fid"]), ref["ftol"], ref["fid"]))
    assert np.all(ex <= tol), what
    assert np.all(eb <= btol), what
    assert abs(fid - ref["fid"]) <= ref["ftol"], what


# ------------------------------------------------------------------------------------------------
# 1. entry-point parity against the restatement, per site
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_entry_point_matches_the_restatement(shape, scheme, dtype):
    for weighting in WEIGHTINGS:
        x, q, x0, kw, ref = _inputs(shape, scheme, dtype, weighting)
        shares = (np.mean(ref["b"] < 0), np.mean(x0 == 0), np.mean((x0 == 0) & (ref["b"] < 0)))
        print("%s %s %s %s: sites with b < 0 %.3f, x0 = 0 %.3f, both %.3f" % (weighting, scheme, shape, np.dtype(dtype).name, *shares))
        assert min(shares) >= 0.05, shares
        for theta in (0.0, 1.0):
            for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
                what = "%s %s pitch %r theta %g" % (weighting, scheme, pitch, theta)
                keep = {}
                got = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, kw, pitch=pitch, keep=keep)
                assert got[0].dtype == dtype and got[1].dtype == dtype
                _check_step(what, got, ref, theta)
                if theta == 0.0:
                    np.testing.assert_array_equal(got[1], got[0], err_msg=what)       # x_bar = x_new exactly
                _untouched(keep, INPUTS)


# ------------------------------------------------------------------------------------------------
# 2. what the stable form makes exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_zero_counts_pads_and_sign_are_exact(scheme, dtype):
    for shape in PARITY_SHAPES:
        x, q, x0, kw, ref = _inputs(shape, scheme, dtype, "plain")
        dead = (x0 == 0) & (ref["b"] < -ref["btol"])                  # (nearer to b = 0 the rounding of b decides the side)
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            keep = {}
            xn, xb, fid = gpu_kl(x, q, x0, TAU, 1.0, scheme, dtype, kw, pitch=pitch, keep=keep)
            print("%s %s pitch %r: %d of %d sites with x0 = 0 and b < 0; min x_new %.3e" % (scheme, shape, pitch, dead.sum(), dead.size, xn.min()))
            assert dead.sum() >= 0.05 * dead.size
            assert np.all(xn[dead] == 0.0) and not np.any(np.signbit(xn[dead]))
            assert np.all(np.isfinite(xn)) and np.all(xn >= 0.0) and np.all(np.isfinite(xb)) and np.isfinite(fid)
            assert np.all(xn[x0 > 0] > 0.0)                              # F stays finite
            _pads_are_zero(keep["dev"]["x"])                           # the whole allocation: what is not a voxel is a pad
            _pads_are_zero(keep["dev"]["x_bar"])


# ------------------------------------------------------------------------------------------------
# 3. residual mode: reduce-only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_residual_mode_reduces_and_writes_nothing(scheme, dtype):
    shape = (3, 2, 16, 20)
    x, q, x0, kw, ref = _inputs(shape, scheme, dtype, "plain")
    vals = {}
    for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
        for null_x_bar in (False, True):
            keep = {}
            # theta is ignored: a value the step mode refuses; x_bar is poisoned
            _, _, res = gpu_kl(x, q, x0, TAU, 5.0, scheme, dtype, kw, pitch=pitch, keep=keep, residual=True, null_x_bar=null_x_bar,
                               x_bar_fill=float("nan"))
            _untouched_bits(keep, EVERYTHING)
            vals[(pitch, null_x_bar)] = res
            assert abs(res - ref["res"]) <= ref["rtol_res"], (pitch, null_x_bar, res, ref["res"], ref["rtol_res"])
        assert vals[(pitch, True)] == vals[(pitch, False)]
    # what a step would change: sum (x_before - x_after)^2 / tau^2
    xn, _, _ = gpu_kl(x, q, x0, TAU, 1.0, scheme, dtype, kw)
    stepped = float(np.sum((x.astype(np.float64) - xn.astype(np.float64)) ** 2)) / TAU ** 2
    print("%s %s: R %.12e restated %.12e from a step %.12e (tol %.3e)" % (scheme, np.dtype(dtype).name, vals[((0, 0), False)], ref["res"], stepped,
                                                                          ref["rtol_res"]))
    assert abs(vals[((0, 0), False)] - stepped) <= ref["rtol_res"]


# ------------------------------------------------------------------------------------------------
# 4. z-ranges: planes [a, b) with hand-made halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
Z_SHAPE = (5, 2, 16, 20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_z_ranges_equal_the_whole_volume(scheme, dtype):
    theta = 1.0
    x, q, x0, kw, ref = _inputs(Z_SHAPE, scheme, dtype, "plain")
    wxn, wxb, wfid = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, kw)
    wres = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, kw, residual=True)[2]
    for cut in ((0, 1, 5), (0, 2, 5), (0, 1, 4, 5)):
        fids, ress = [], []
        for a, b in zip(cut[:-1], cut[1:]):
            keep = {}
            xn, xb, fid = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, kw, z_range=(a, b), keep=keep)
            np.testing.assert_array_equal(xn, wxn[a:b], err_msg="x, cut %r planes [%d, %d)" % (cut, a, b))
            np.testing.assert_array_equal(xb, wxb[a:b], err_msg="x_bar, cut %r planes [%d, %d)" % (cut, a, b))
            _untouched(keep, INPUTS)                               # q, x0 and the halo planes
            fids.append(fid)
            keep = {}
            ress.append(gpu_kl(x, q, x0, TAU, theta, scheme, dtype, kw, z_range=(a, b), keep=keep, residual=True)[2])
            _untouched(keep, EVERYTHING)
        print("cut %r: F parts sum %.17g whole %.17g (tol %.3e); R parts sum %.17g whole %.17g (tol %.3e)" % (
            cut, sum(fids), wfid, ref["ftol"], sum(ress), wres, ref["rtol_res"]))
        assert abs(sum(fids) - wfid) <= ref["ftol"], cut
        assert abs(sum(ress) - wres) <= ref["rtol_res"], cut


@pytest.mark.parametrize("scheme", SCHEMES)
def test_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    x, q, x0, kw, _ = _inputs(Z_SHAPE, scheme, np.float32, "plain")
    # the adjoint of a forward difference reads the previous slab, of a backward difference the next one (central, hybrid: both)
    sides = {"upwind": ("prev",), "downwind": ("next",)}.get(scheme, ("prev", "next"))
    for side in sides:
        for residual in (False, True):
            keep = {}
            with pytest.raises(ValueError, match=r"halo.*code -2"):
                gpu_kl(x, q, x0, TAU, 1.0, scheme, np.float32, kw, z_range=(1, 4), keep=keep, drop_halo=side, residual=residual)
            torch.cuda.synchronize()
            _untouched(keep, EVERYTHING)


# ------------------------------------------------------------------------------------------------
# 5. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
MARCH_SHAPE = (2, 2, 1024, 1024)


@functools.lru_cache(maxsize=1)
def _march_inputs(scheme):
    """x and q of tests/test_gpu_cp_prox._march_inputs, a third of x lowered by 80, x0 by quarters; the restatement of the step on them"""
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, MARCH_SHAPE[0], MARCH_SHAPE[1], **PLAIN_KW)
    x = 60.0 * rng.random(MARCH_SHAPE, dtype=np.float32)
    q = LAM * (rng.random((MARCH_SHAPE[0], nd) + MARCH_SHAPE[1:], dtype=np.float32) - 0.5)
    x = x - np.float32(80.0) * (rng.random(MARCH_SHAPE, dtype=np.float32) < 1.0 / 3.0)
    x0 = counts_by_quarters(MARCH_SHAPE, rng).astype(np.float32)
    gd = orc.D_T(q.astype(np.float64), scheme, **PLAIN_KW)
    return x, q, x0, reference(x, gd, x0, TAU, np.float32)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_marching_form_equals_one_site_form(scheme, tvopt):
    dtype, theta = np.float32, 0.37
    x, q, x0, ref = _march_inputs(scheme)
    march = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, PLAIN_KW)
    march_res = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    tvopt("TV_NO_MARCH", 1)
    site = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, PLAIN_KW)
    site_res = gpu_kl(x, q, x0, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    # x to tol_i; x_bar to its own per-site tolerance (module docstring): x_bar has the size of x, not of x_new, so where x_new << |x| one
    # rounding of x_bar is already far more than tol_i
    tol = ref["tol"]
    btol = tol * (1.0 + theta) + theta * ref["rtol"] * np.abs(ref["x"])
    print("%s: max|dx| %.3e  max|dx_bar| %.3e  sites beyond their tolerance: x %d x_bar %d;  F %.9e / %.9e (tol %.3e)  R %.9e / %.9e (tol %.3e)  sites at 0: %.3f" % (
        scheme, np.max(np.abs(march[0] - site[0])), np.max(np.abs(march[1] - site[1])), np.sum(np.abs(march[0] - site[0]) > tol),
        np.sum(np.abs(march[1] - site[1]) > btol), march[2], site[2], ref["ftol"], march_res, site_res, ref["rtol_res"], np.mean(site[0] == 0.0)))
    assert np.all(np.abs(march[0] - site[0]) <= tol)
    assert np.all(np.abs(march[1] - site[1]) <= btol)
    assert abs(march[2] - site[2]) <= ref["ftol"]
    assert abs(march_res - site_res) <= ref["rtol_res"]
    assert np.isfinite(march[2]) and march[2] > 0.0 and np.isfinite(march_res) and march_res > 0.0
    assert 0.05 <= np.mean(site[0] == 0.0) <= 0.15                   # x0 = 0 with b < 0: a quarter of a third of the sites
    # and both are the restatement's step
    _check_step("%s marching" % scheme, march, ref, theta)
    _check_step("%s one-site" % scheme, site, ref, theta)


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 1, theta = 1) and of its optimality residuals
# ------------------------------------------------------------------------------------------------
REG = 0.5
TRAJ_SHAPES = [(1, 1, 24, 28), (3, 2, 16, 20)]
N_TRAJ = 60


@functools.lru_cache(maxsize=None)
def clean_phantom(shape):
    """mean count 2 with a centred square of 20"""
    c = np.full(shape, 2.0)
    ny, nx = shape[2:]
    c[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 20.0
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def counts(shape):
    x = np.random.default_rng(0).poisson(clean_phantom(shape)).astype(np.float64)
    x.setflags(write=False)
    return x


def _steps_of(shape, scheme):
    s = 1.0 / np.sqrt(orc.normal_spectral_bound(scheme, shape, **_kw_of(shape)))
    return s, s


def np_residuals(x, q, x0, lam, scheme, kw, tau, sigma):
    """the dict of ``residuals()``, and the absolute rounding floor of R_x in fp64: x - x_new carries an error of a few eps (|b| + s) per
    site, so R_x carries 2 sqrt(R_x E) + E with E = sum (4 eps (|b| + s) / tau)^2 -- what is left of R_x at x = x0, q = 0, where it is 0"""
    Dx = orc.D(x, scheme, **kw)
    rq = float(np.sum((q - np_project(q + sigma * Dx, lam)) ** 2)) / sigma ** 2
    v = x - tau * orc.D_T(q, scheme, **kw)
    xn = prox_kl_np(v, x0, tau)
    rx = float(np.sum(((x - xn) / tau) ** 2))
    e = float(np.sum((4.0 * np.finfo(np.float64).eps * (np.abs(v - tau) + np.sqrt((v - tau) ** 2 + 4.0 * tau * x0)) / tau) ** 2))
    return {"x": rx, "q": rq, "total": rx + rq, "tv": float(orc.compute_L21_norm(Dx)), "fid": kl_np(x, x0)}, 2.0 * np.sqrt(rx * e) + e


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, n_iter):
    """(x, loss, q, loss tolerance of an fp32 run) after n_iter iterations from the counts.  The fp32 loss tolerance of iteration k is
    1e-5 |loss| + sum_i g_i (1e-5 |x_i| + 2e-3) with g_i = |1 - x0_i / x_i| (1 where x_i = 0): the project's fp32 tolerance of the iterate
    (rtol 1e-5, atol 2e-3) carried through dF / dx."""
    x0, kw, lam = np.asarray(counts(shape)), _kw_of(shape), REG
    tau, sigma = _steps_of(shape, scheme)
    x, xb = x0.copy(), x0.copy()
    q = np.zeros_like(orc.D(x0, scheme, **kw))
    loss, ltol = np.zeros(n_iter), np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project(q + sigma * Dxb, lam)
        xn = prox_kl_np(x - tau * orc.D_T(q, scheme, **kw), x0, tau)
        xb = 2.0 * xn - x
        x = xn
        loss[k] = kl_np(x, x0) + lam * orc.compute_L21_norm(Dxb)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(x > 0, np.abs(1.0 - x0 / x), 1.0)
        ltol[k] = 1e-5 * abs(loss[k]) + float(np.sum(g * (1e-5 * np.abs(x) + 2e-3)))
    return x, loss, q, ltol


def _solver(pytv, shape, dtype, scheme, **how):
    return pytv.solvers.PoissonChambollePock(torch.as_tensor(counts(shape).astype(dtype)).cuda(), REG, scheme=scheme, **_kw_of(shape), **how)


# ------------------------------------------------------------------------------------------------
# 6. solver trajectory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme):
    import pytv
    wx, wloss, _, _ = np_trajectory(shape, scheme, N_TRAJ)
    zeros = int(np.sum(counts(shape) == 0))
    assert zeros == {(1, 1, 24, 28): 62, (3, 2, 16, 20): 207}[shape]        # the data has sites without a count
    cp = _solver(pytv, shape, np.float64, scheme)
    assert cp.it == 0 and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape)) and cp.tau == cp.sigma == 1.0 / np.sqrt(cp.L2)
    loss = cp.run(N_TRAJ)
    x = cp.result().cpu().numpy()
    print("%s %s: loss rel %.3e  max|dx| %.3e  sites with x0 = 0: %d, of them at exactly 0: %d (restatement %d)" % (
        scheme, shape, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx)), zeros, int(np.sum(x == 0.0)), int(np.sum(wx == 0.0))))
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(wloss))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(counts(shape)))
    assert np.all(x >= 0.0) and cp.it == N_TRAJ
    assert np.all(x[wx == 0.0] == 0.0)                                # where the iterate reaches the boundary it is an exact 0, and the loss stayed finite
    if scheme == "upwind":
        assert np.sum(wx == 0.0) > 0
    # run(25); run(35) is run(60) bit for bit; reset() reproduces the run; record_loss=False returns nothing and computes the same
    two = _solver(pytv, shape, np.float64, scheme)
    np.testing.assert_array_equal(np.concatenate([two.run(25), two.run(35)]), loss)
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.x_bar, cp.x_bar) and torch.equal(two.q, cp.q)
    two.reset()
    assert two.it == 0 and torch.equal(two.x, two.x0) and torch.equal(two.x_bar, two.x0) and not bool(two.q.any())
    assert two.run(N_TRAJ, record_loss=False) is None
    assert torch.equal(two.result(), cp.result()) and torch.equal(two.q, cp.q)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme):
    """against the fp64 restatement on the same counts (integers: exact in fp32): result rtol 1e-5, atol 2e-3 (the project's fp32 figures);
    loss to that tolerance carried through dF / dx (``np_trajectory``)"""
    import pytv
    wx, wloss, _, ltol = np_trajectory(shape, scheme, N_TRAJ)
    cp = _solver(pytv, shape, np.float32, scheme)
    loss = cp.run(N_TRAJ)
    x = cp.result().cpu().numpy()
    print("%s %s: max |dloss| / tol %.3e  max|dx| %.3e" % (scheme, shape, np.max(np.abs(loss - wloss) / ltol), np.max(np.abs(x - wx))))
    assert np.all(np.isfinite(loss))
    assert np.all(np.abs(loss - wloss) <= ltol)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)
    assert np.all(x >= 0.0)


# ------------------------------------------------------------------------------------------------
# 7. certificate and stopping
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_residuals_against_the_restatement(shape, scheme):
    import pytv
    kw, x0 = _kw_of(shape), np.asarray(counts(shape))
    tau, sigma = _steps_of(shape, scheme)
    cp = _solver(pytv, shape, np.float64, scheme)
    done = 0
    for n in (0, 1, 30):
        if n > done:
            cp.run(n - done)
            done = n
        wx, _, wq, _ = np_trajectory(shape, scheme, n) if n else (x0, None, np.zeros_like(orc.D(x0, scheme, **kw)), None)
        want, floor = np_residuals(wx, wq, x0, REG, scheme, kw, tau, sigma)
        state = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
        got = cp.residuals()
        print("%s %s after %d: %r  restated %r  (fp64 floor of R_x %.3e)" % (scheme, shape, n, got, want, floor))
        assert sorted(got) == ["fid", "q", "total", "tv", "x"] and got["total"] == got["x"] + got["q"]
        for k in ("q", "tv", "fid"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=0, err_msg="%s after %d" % (k, n))
        np.testing.assert_allclose(got["x"], want["x"], rtol=1e-9, atol=floor, err_msg="x after %d" % n)
        assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q)))
        if n == 0:
            assert got["x"] == 0.0 and got["fid"] == 0.0 and got["total"] == cp.initial_residual() > 0.0      # x = x0, q = 0: F's block is at rest
    np.testing.assert_allclose(cp.initial_residual(), np_residuals(x0, np.zeros_like(orc.D(x0, scheme, **kw)), x0, REG, scheme, kw, tau, sigma)[0]["total"],
                               rtol=1e-9)


@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_run_until_converges(shape, scheme):
    """NumPy restatement on this data, default steps: the relative residual is <= 7.5e-3 after 100 iterations and 2.5 - 3.6e-2 after 50"""
    import pytv
    cp = _solver(pytv, shape, np.float64, scheme)
    r0 = cp.initial_residual()
    loss, info = cp.run_until(1e-2, 400)
    print(scheme, shape, info)
    assert info["converged"] is True and 50 < info["iterations"] <= 200 and info["iterations"] % 10 == 0
    assert len(loss) == info["iterations"] == cp.it and np.all(np.isfinite(loss))
    assert info["initial"] == r0 and info["residuals"]["total"] <= 1e-2 ** 2 * r0
    assert info["relative"] == np.sqrt(cp.residuals()["total"] / r0)
    assert sorted(info) == ["converged", "initial", "iterations", "relative", "residuals"]


def test_run_until_on_a_constant_image_returns_at_once():
    import pytv
    for dtype in (torch.float32, torch.float64):
        for scheme in SCHEMES:
            cp = pytv.solvers.PoissonChambollePock(torch.full((2, 2, 8, 12), 7.0, dtype=dtype, device="cuda"), 1.0, scheme=scheme, reg_time=0.5)
            loss, info = cp.run_until(1e-3, 100)
            assert info["converged"] is True and info["iterations"] == 0 == cp.it and info["initial"] == 0.0 and info["relative"] == 0.0
            assert len(loss) == 0


def test_an_all_zero_image_stays_exactly_zero():
    import pytv
    for dtype in (torch.float32, torch.float64):
        cp = pytv.solvers.PoissonChambollePock(torch.zeros((2, 2, 8, 12), dtype=dtype, device="cuda"), 1.0, reg_time=0.5)
        loss = cp.run(20)
        assert not bool(_storage(cp.x).any()) and not bool(_storage(cp.x_bar).any()) and not bool(cp.q.any())
        np.testing.assert_array_equal(loss, np.zeros(20))


# ------------------------------------------------------------------------------------------------
# 8. it does what it is for: Poisson noise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_it_denoises_poisson_counts(shape):
    """NumPy restatement, mean absolute error against the clean phantom, TV-KL / noisy: 0.989 / 1.626 = 0.61 and 1.008 / 1.710 = 0.59"""
    import pytv
    clean, noisy = clean_phantom(shape), counts(shape)
    cp = _solver(pytv, shape, np.float32, "upwind")
    _, info = cp.run_until(1e-2, 400)
    out = cp.result().cpu().numpy().astype(np.float64)
    m_noisy, m_kl = float(np.mean(np.abs(noisy - clean))), float(np.mean(np.abs(out - clean)))
    print("%s: mean abs error noisy %.3f  TV-KL %.3f  ratio %.3f  %r" % (shape, m_noisy, m_kl, m_kl / m_noisy, info))
    assert info["converged"] is True
    assert m_kl < 0.75 * m_noisy
    assert float(out.min()) >= 0.0


# ------------------------------------------------------------------------------------------------
# 9. constructor and front-end
# ------------------------------------------------------------------------------------------------
def test_constructor_refuses_bad_counts_and_bad_steps():
    import pytv
    good = counts((1, 1, 24, 28)).copy()
    for bad_value in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        bad = good.copy()
        bad[0, 0, 5, 7] = bad_value
        for dtype in (np.float32, np.float64):
            with pytest.raises(ValueError, match="counts"):
                pytv.solvers.PoissonChambollePock(torch.as_tensor(bad.astype(dtype)).cuda(), 1.0)
    x0 = torch.as_tensor(good).cuda()
    L2 = 8.0
    with pytest.raises(ValueError, match="tau"):
        pytv.solvers.PoissonChambollePock(x0, 1.0, scheme="upwind", tau=1.0, sigma=(1.0 + 1e-9) / L2)
    ok = pytv.solvers.PoissonChambollePock(x0, 1.0, scheme="upwind", tau=1.0, sigma=1.0 / L2)
    assert ok.L2 == L2 and (ok.tau, ok.sigma) == (1.0, 1.0 / L2)
    assert pytv.solvers.PoissonChambollePock(x0, 1.0, scheme="upwind", sigma=0.25).tau == 1.0 / (L2 * 0.25)
    with pytest.raises(ValueError, match="tau"):
        pytv.solvers.PoissonChambollePock(x0, 1.0, tau=0.0)


def test_denoise_tv_poisson_front_end():
    import pytv
    shape = (1, 1, 24, 28)
    img = counts(shape)[0, 0].astype(np.float32)
    vol = torch.as_tensor(img.reshape(shape)).cuda()
    out = pytv.denoise_tv_poisson(img, 0.5)
    ref = pytv.solvers.PoissonChambollePock(vol, 0.5, scheme="upwind", reg_z_over_reg=1.0)
    _, info = ref.run_until(1e-2, 400, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] % 10 == 0 and info["iterations"] < 400
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == img.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # never converges: exactly 40 iterations, the solver's run(40), with a step of the caller's
    out = pytv.denoise_tv_poisson(img, 0.5, rel_res=0.0, max_num_iter=40, scheme="hybrid", tau=0.2)
    ref = pytv.solvers.PoissonChambollePock(vol, 0.5, scheme="hybrid", tau=0.2)
    ref.run(40)
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # torch in -> device tensor out, fp64 stays fp64; 3-D input is a stack with a z axis; 4-D refused; so are negative counts
    t = pytv.denoise_tv_poisson(vol[0, 0].double(), 0.5, rel_res=0.0, max_num_iter=10)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.shape == vol.shape[2:]
    stack = np.stack([img, img[::-1], img])
    out3 = pytv.denoise_tv_poisson(stack, 0.5, rel_res=0.0, max_num_iter=10)
    ref3 = pytv.solvers.PoissonChambollePock(torch.as_tensor(stack.reshape(3, 1, 24, 28).copy()).cuda(), 0.5, scheme="upwind", reg_z_over_reg=1.0)
    ref3.run_until(0.0, 10)
    assert out3.shape == stack.shape and out3.dtype == np.float32
    np.testing.assert_array_equal(out3, ref3.result().cpu().numpy().reshape(stack.shape))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.denoise_tv_poisson(np.zeros((1, 1, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="counts"):
        pytv.denoise_tv_poisson(-img)
