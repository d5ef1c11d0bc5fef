"""Chambolle-Pock with a robust data term on the GPU (``-m gpu``): tv_cp_primal_prox through the C-ABI against an fp64 NumPy restatement of the
step (textbook prox formulas on ``orc.D_T`` of the same inputs), its reduce-only residual mode, z-ranges against the whole volume, the
plane-marching form against the one-site form, and ``RobustChambollePock`` / ``denoise_tv_robust`` against a NumPy restatement of Algorithm 1 of
Chambolle & Pock 2011 built on ``orc.D`` / ``orc.D_T`` -- trajectory, optimality residuals, ``run_until``, and that TV-L1 removes impulse noise
where the quadratic model does not.

Tolerances are the project's (tests/test_gpu_cp_accel.py): arrays to tol_x = rtol * max|x_ref| with rtol 1e-5 (fp32) / 1e-11 (fp64); the L2
fidelity scalar to that rtol; the L1 / Huber fidelity value (1-Lipschitz in x_new) to N * tol_x; the residual-mode scalar sum (d / tau)^2 to
2 (tol_x / tau) sqrt(N R_ref) + N (tol_x / tau)^2, which follows from a per-site error of tol_x in x_new (Cauchy-Schwarz); N = voxels."""
import functools

import numpy as np
import pytest
import torch

from conftest import SCHEMES
from oracle import tv_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = {np.float32: 1e-5, np.float64: 1e-11}
DTYPES = [np.float64, np.float32]
FIDELITIES = ("l2", "l1", "huber")
LAM = 5.0
TAU, DELTA = 0.3, 0.5


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


# ------------------------------------------------------------------------------------------------
# the step, restated in fp64 with the textbook formulas (not the clamp form the kernel uses)
# ------------------------------------------------------------------------------------------------
def prox_np(e, fidelity, tau, delta):
    if fidelity == "l2":
        return e / (1.0 + tau)
    if fidelity == "l1":
        return np.sign(e) * np.maximum(np.abs(e) - tau, 0.0)
    return np.where(np.abs(e) <= delta + tau, e * delta / (delta + tau), e - tau * np.sign(e))


def fid_np(e, fidelity, delta):
    if fidelity == "l2":
        return float(0.5 * np.sum(e * e))
    if fidelity == "l1":
        return float(np.sum(np.abs(e)))
    return float(np.sum(np.where(np.abs(e) <= delta, e * e / (2.0 * delta), np.abs(e) - 0.5 * delta)))


def make_inputs(shape, scheme, dtype, kw, seed=5, tau=TAU, delta=DELTA):
    """x, q as in tests/test_gpu_cp_accel.py; x0 = (x - tau D^T q) - e with e uniform in [-3 (delta + tau), 3 (delta + tau)], so that every regime
    of the three prox maps is hit.  Returns (x, q, x0, gd) with gd = D^T q in fp64 from the rounded q."""
    rng = np.random.default_rng(seed)
    x = (60.0 * rng.random(shape)).astype(dtype)
    nd = orc.D(np.zeros(shape), scheme, **kw).shape[1]
    q = rng.standard_normal((shape[0], nd) + tuple(shape[1:]))
    n = np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    q = (q / np.maximum(n, 1e-30) * (LAM * np.minimum(1.0, 1.5 * rng.random(n.shape)))).astype(dtype)     # |q|_2 <= LAM per site
    gd = orc.D_T(q.astype(np.float64), scheme, **kw)
    w = 3.0 * (delta + tau)
    e = w * (2.0 * rng.random(shape) - 1.0)
    x0 = ((x.astype(np.float64) - tau * gd) - e).astype(dtype)
    return x, q, x0, gd


def ref_prox(x, gd, x0, fidelity, tau, theta, delta=DELTA):
    """(x_new, x_bar, F(x_new - x0), e, R) in fp64 from gd = D^T q; R = sum ((x - x_new) / tau)^2, the residual-mode scalar"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    e = (x - tau * gd) - x0
    xn = x0 + prox_np(e, fidelity, tau, delta)
    return xn, xn + theta * (xn - x), fid_np(xn - x0, fidelity, delta), e, float(np.sum(((x - xn) / tau) ** 2))


def fid_tol(fidelity, dtype, wfid, tol_x, n):
    return RTOL[dtype] * wfid if fidelity == "l2" else n * tol_x


def res_tol(wres, tol_x, tau, n):
    return 2.0 * (tol_x / tau) * np.sqrt(n * wres) + n * (tol_x / tau) ** 2


def gpu_prox(x, q, x0, fidelity, tau, theta, scheme, dtype, kw, pitch=(0, 0), z_range=None, keep=None, drop_halo=None, residual=False,
             null_x_bar=False, delta=DELTA, entry="prox"):
    """tv_cp_primal_prox (entry="accel": tv_cp_primal_accel) on local planes [a, b) of the arrays (whole volume by default), halo planes passed by
    hand.  Returns (x, x_bar, scalar) as numpy / float after the call.  keep: receives the device tensors and copies of their storage made
    before the call.  drop_halo: "prev" / "next" -- pass NULL for that halo plane.  residual: TV_CPP_RESIDUAL; null_x_bar: pass x_bar = NULL."""
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
    head = (g.ref, nv.ptr(dev["q"]), nv.ptr(dev["qp"]), nv.ptr(dev["qn"]), nv.ptr(dev["x"]), None if null_x_bar else nv.ptr(dev["x_bar"]),
            nv.ptr(dev["x0"]))
    tail = (out.data_ptr(), nv.ptr(g.workspace()), nv.current_stream(g.device))
    if entry == "accel":
        nv.check(nv.lib().tv_cp_primal_accel(*head, float(tau), float(theta), *tail))
    else:
        nv.check(nv.lib().tv_cp_primal_prox(*head, nv.FIDELITIES[fidelity], float(delta), float(tau), float(theta),
                                            nv.TV_CPP_RESIDUAL if residual else 0, *tail))
    return dev["x"].cpu().numpy(), dev["x_bar"].cpu().numpy(), float(out.item())


def _untouched(keep, names):
    for k in names:
        if keep["dev"][k] is not None:
            assert torch.equal(_storage(keep["dev"][k]), keep["before"][k]), k          # the whole allocation: pad columns included


INPUTS = ("q", "x0", "qp", "qn")
EVERYTHING = ("x", "x_bar", "q", "x0", "qp", "qn")


def _pads_are_zero(t):
    pads = _storage(t).clone()
    pads.as_strided(t.shape, t.stride()).zero_()
    assert not bool(pads.any())                                        # what is not a voxel is a pad


# scalar rows, 2-D | 16-byte lanes | two-plane z (central: forward stencil) | M > 8
PARITY_SHAPES = [(1, 1, 9, 13), (3, 2, 16, 20), (2, 3, 12, 16), (4, 9, 8, 16)]


def _explicit_pitch(shape, dtype):
    lane = 16 // np.dtype(dtype).itemsize
    rp = -(-(shape[3] + 4) // lane) * lane                              # nx + 4 rounded up to 16 bytes
    return rp, shape[2] * rp + 8


# ------------------------------------------------------------------------------------------------
# 1. entry-point parity against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_entry_point_matches_the_restatement(shape, scheme, dtype):
    n = int(np.prod(shape))
    for weighting in WEIGHTINGS:
        kw = _case_kw(weighting, shape)
        x, q, x0, gd = make_inputs(shape, scheme, dtype, kw)
        for fidelity in FIDELITIES:
            for theta in (0.0, 0.37, 1.0):
                wxn, wxb, wfid, e, _ = ref_prox(x, gd, x0, fidelity, TAU, theta)
                ae = np.abs(e)
                shares = (np.mean(ae <= TAU), np.mean((ae > TAU) & (ae <= DELTA + TAU)), np.mean(ae > DELTA + TAU))
                assert min(shares) >= 0.05, shares                      # every regime of the three prox maps is hit
                tol = RTOL[dtype] * float(np.max(np.abs(wxn)))
                for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
                    what = "%s %s %s pitch %r theta %g" % (weighting, scheme, fidelity, pitch, theta)
                    keep = {}
                    xn, xb, fid = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, kw, pitch=pitch, keep=keep)
                    ftol = fid_tol(fidelity, dtype, wfid, tol, n)
                    print("%s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  |dF| %.3e (tol %.3e)  regimes %.2f %.2f %.2f" % (
                        what, np.max(np.abs(xn - wxn)), np.max(np.abs(xb - wxb)), tol, abs(fid - wfid), ftol, *shares))
                    assert xn.dtype == dtype and xb.dtype == dtype
                    assert float(np.max(np.abs(xn - wxn))) <= tol, what
                    assert float(np.max(np.abs(xb - wxb))) <= tol, what
                    assert abs(fid - wfid) <= ftol, what
                    if theta == 0.0:
                        np.testing.assert_array_equal(xb, xn, err_msg=what)       # x_bar = x_new exactly
                    _untouched(keep, INPUTS)
                    if pitch != (0, 0):
                        _pads_are_zero(keep["dev"]["x"])
                        _pads_are_zero(keep["dev"]["x_bar"])


# ------------------------------------------------------------------------------------------------
# 2. L1: a site inside the dead zone returns x0 bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_l1_dead_zone_returns_x0_bit_for_bit(scheme, dtype):
    for shape in PARITY_SHAPES:
        x, q, x0, gd = make_inputs(shape, scheme, dtype, PLAIN_KW)
        wxn, _, _, e, _ = ref_prox(x, gd, x0, "l1", TAU, 1.0)
        tol = RTOL[dtype] * float(np.max(np.abs(wxn)))
        ae = np.abs(e)
        inside = ae <= TAU - tol
        edge = np.abs(ae - TAU) < tol                                   # left out: the rounding of e decides on which side they fall
        for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
            xn, _, _ = gpu_prox(x, q, x0, "l1", TAU, 1.0, scheme, dtype, PLAIN_KW, pitch=pitch)
            print("%s %s pitch %r: %d of %d sites inside the dead zone, %d at its edge" % (scheme, shape, pitch, inside.sum(), inside.size, edge.sum()))
            assert np.mean(edge) <= 0.01 and inside.sum() >= 0.05 * inside.size
            np.testing.assert_array_equal(xn[inside], x0[inside])
            assert np.all(xn[(ae > TAU + tol)] != x0[(ae > TAU + tol)])             # and outside it the site moves


# ------------------------------------------------------------------------------------------------
# 3. the L2 fidelity against the accelerated solver's kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_l2_agrees_with_tv_cp_primal_accel(scheme, dtype):
    for shape in PARITY_SHAPES:
        x, q, x0, _ = make_inputs(shape, scheme, dtype, PLAIN_KW)
        for theta in (0.0, 0.37, 1.0):
            a = gpu_prox(x, q, x0, "l2", TAU, theta, scheme, dtype, PLAIN_KW, entry="accel")
            p = gpu_prox(x, q, x0, "l2", TAU, theta, scheme, dtype, PLAIN_KW)
            tol = RTOL[dtype] * float(np.max(np.abs(a[0])))
            print("%s %s theta %g: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  fid rel %.3e" % (scheme, shape, theta, np.max(np.abs(p[0] - a[0])),
                                                                                               np.max(np.abs(p[1] - a[1])), tol, abs(p[2] / a[2] - 1.0)))
            assert float(np.max(np.abs(p[0] - a[0]))) <= tol and float(np.max(np.abs(p[1] - a[1]))) <= tol
            assert abs(p[2] - a[2]) <= RTOL[dtype] * a[2]


# ------------------------------------------------------------------------------------------------
# 4. residual mode: reduce-only
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("fidelity", FIDELITIES)
def test_residual_mode_reduces_and_writes_nothing(fidelity, scheme, dtype):
    shape = (3, 2, 16, 20)
    n = int(np.prod(shape))
    x, q, x0, gd = make_inputs(shape, scheme, dtype, PLAIN_KW)
    wxn, _, _, _, wres = ref_prox(x, gd, x0, fidelity, TAU, 1.0)
    tol = res_tol(wres, RTOL[dtype] * float(np.max(np.abs(wxn))), TAU, n)
    vals = {}
    for pitch in ((0, 0), _explicit_pitch(shape, dtype)):
        for null_x_bar in (False, True):
            keep = {}
            # theta is ignored: a value the step mode refuses
            _, _, res = gpu_prox(x, q, x0, fidelity, TAU, 5.0, scheme, dtype, PLAIN_KW, pitch=pitch, keep=keep, residual=True, null_x_bar=null_x_bar)
            _untouched(keep, EVERYTHING)
            vals[(pitch, null_x_bar)] = res
            assert abs(res - wres) <= tol, (pitch, null_x_bar, res, wres, tol)
        assert vals[(pitch, True)] == vals[(pitch, False)]
    # what a step would change: sum (x_before - x_after)^2 / tau^2
    xn, _, _ = gpu_prox(x, q, x0, fidelity, TAU, 1.0, scheme, dtype, PLAIN_KW)
    stepped = float(np.sum((x.astype(np.float64) - xn.astype(np.float64)) ** 2)) / TAU ** 2
    print("%s %s %s: R %.12e restated %.12e from a step %.12e (tol %.3e)" % (fidelity, scheme, np.dtype(dtype).name, vals[((0, 0), False)], wres, stepped, tol))
    assert abs(vals[((0, 0), False)] - stepped) <= tol


# ------------------------------------------------------------------------------------------------
# 5. z-ranges: planes [a, b) with hand-made halo planes against the whole-volume call
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_z_ranges_equal_the_whole_volume(scheme, dtype):
    shape, theta = (5, 2, 16, 20), 0.37
    x, q, x0, _ = make_inputs(shape, scheme, dtype, PLAIN_KW)
    for fidelity in FIDELITIES:
        wxn, wxb, wfid = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW)
        wres = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
        for cut in ((0, 1, 5), (0, 2, 5), (0, 1, 4, 5)):
            fids, ress = [], []
            for a, b in zip(cut[:-1], cut[1:]):
                keep = {}
                xn, xb, fid = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW, z_range=(a, b), keep=keep)
                np.testing.assert_array_equal(xn, wxn[a:b], err_msg="x, cut %r planes [%d, %d)" % (cut, a, b))
                np.testing.assert_array_equal(xb, wxb[a:b], err_msg="x_bar, cut %r planes [%d, %d)" % (cut, a, b))
                _untouched(keep, INPUTS)                               # q, x0 and the halo planes
                fids.append(fid)
                keep = {}
                ress.append(gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW, z_range=(a, b), keep=keep, residual=True)[2])
                _untouched(keep, EVERYTHING)
            print("%s cut %r: F parts sum %.17g whole %.17g; R parts sum %.17g whole %.17g" % (fidelity, cut, sum(fids), wfid, sum(ress), wres))
            assert abs(sum(fids) - wfid) <= 1e-13 * wfid, cut
            assert abs(sum(ress) - wres) <= 1e-13 * wres, cut


@pytest.mark.parametrize("scheme", SCHEMES)
def test_missing_halo_plane_is_refused_and_nothing_is_written(scheme):
    shape = (5, 2, 16, 20)
    x, q, x0, _ = make_inputs(shape, scheme, np.float32, PLAIN_KW)
    # the adjoint of a forward difference reads the previous slab, of a backward difference the next one (central, hybrid: both)
    sides = {"upwind": ("prev",), "downwind": ("next",)}.get(scheme, ("prev", "next"))
    for side in sides:
        for residual in (False, True):
            keep = {}
            with pytest.raises(ValueError, match=r"halo.*code -2"):
                gpu_prox(x, q, x0, "l1", TAU, 0.37, scheme, np.float32, PLAIN_KW, z_range=(1, 4), keep=keep, drop_halo=side, residual=residual)
            torch.cuda.synchronize()
            _untouched(keep, EVERYTHING)


# ------------------------------------------------------------------------------------------------
# 6. plane-marching form (fp32, planes of >= 4 MiB) against the one-site form
# ------------------------------------------------------------------------------------------------
MARCH_SHAPE = (2, 2, 1024, 1024)


@functools.lru_cache(maxsize=1)
def _march_inputs(scheme):
    rng = np.random.default_rng(11)
    nd = orc.num_channels(scheme, MARCH_SHAPE[0], MARCH_SHAPE[1], **PLAIN_KW)
    x = 60.0 * rng.random(MARCH_SHAPE, dtype=np.float32)
    q = LAM * (rng.random((MARCH_SHAPE[0], nd) + MARCH_SHAPE[1:], dtype=np.float32) - 0.5)
    # x - x0 uniform in +- 3 (delta + tau) and tau D^T q of the same order: every regime of the prox maps occurs
    x0 = x + np.float32(3.0 * (DELTA + TAU)) * (2.0 * rng.random(MARCH_SHAPE, dtype=np.float32) - 1.0)
    return x, q, x0


@pytest.mark.parametrize("fidelity", ("l1", "huber"))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_marching_form_equals_one_site_form(scheme, fidelity, tvopt):
    dtype, theta = np.float32, 0.37
    n = int(np.prod(MARCH_SHAPE))
    x, q, x0 = _march_inputs(scheme)
    march = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW)
    march_res = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    tvopt("TV_NO_MARCH", 1)
    site = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW)
    site_res = gpu_prox(x, q, x0, fidelity, TAU, theta, scheme, dtype, PLAIN_KW, residual=True)[2]
    tol = 1e-5 * float(np.max(np.abs(site[0])))
    moved = float(np.mean(site[0] != x0))
    print("%s %s: max|dx| %.3e  max|dx_bar| %.3e  (tol %.3e)  F %.9e / %.9e  R %.9e / %.9e  sites off x0 %.3f" % (
        scheme, fidelity, np.max(np.abs(march[0] - site[0])), np.max(np.abs(march[1] - site[1])), tol, march[2], site[2], march_res, site_res, moved))
    assert float(np.max(np.abs(march[0] - site[0]))) <= tol
    assert float(np.max(np.abs(march[1] - site[1]))) <= tol
    assert abs(march[2] - site[2]) <= n * tol
    assert abs(march_res - site_res) <= res_tol(site_res, tol, TAU, n)
    assert np.isfinite(march[2]) and march[2] > 0.0 and np.isfinite(march_res) and march_res > 0.0
    if fidelity == "l1":
        assert 0.02 <= 1.0 - moved <= 0.5                                # the dead zone is populated, and so is its complement


# ------------------------------------------------------------------------------------------------
# NumPy restatement of the loop (Chambolle & Pock 2011, Algorithm 1, theta = 1) and of its optimality residuals
# ------------------------------------------------------------------------------------------------
REG, TAU_S, DELTA_S = 1.0, 5.0, 2.0


def np_project(v, lam):
    return v / np.maximum(1.0, np.sqrt(np.sum(v ** 2, axis=1, keepdims=True)) / lam)


def np_robust(x0, n_iter, lam, fidelity, delta, scheme, kw, tau, sigma):
    x0 = np.asarray(x0, dtype=np.float64)
    x, xb = x0.copy(), x0.copy()
    q = np.zeros_like(orc.D(x0, scheme, **kw))
    loss = np.zeros(n_iter)
    for k in range(n_iter):
        Dxb = orc.D(xb, scheme, **kw)
        q = np_project(q + sigma * Dxb, lam)
        xn = x0 + prox_np((x - tau * orc.D_T(q, scheme, **kw)) - x0, fidelity, tau, delta)
        xb = 2.0 * xn - x
        x = xn
        loss[k] = fid_np(x - x0, fidelity, delta) + lam * orc.compute_L21_norm(Dxb)
    return x, loss, q


def np_residuals(x, q, x0, lam, fidelity, delta, scheme, kw, tau, sigma):
    Dx = orc.D(x, scheme, **kw)
    rq = float(np.sum((q - np_project(q + sigma * Dx, lam)) ** 2)) / sigma ** 2
    xn = x0 + prox_np((x - tau * orc.D_T(q, scheme, **kw)) - x0, fidelity, tau, delta)
    rx = float(np.sum(((x - xn) / tau) ** 2))
    return {"x": rx, "q": rq, "total": rx + rq, "tv": float(orc.compute_L21_norm(Dx)), "fid": fid_np(x - x0, fidelity, delta)}


@functools.lru_cache(maxsize=None)
def clean_square(shape):
    """the centred square of height 100 of tests/test_gpu_cp_accel.py (square_plus_noise without the noise)"""
    x = np.zeros(shape)
    ny, nx = shape[2:]
    x[..., ny // 4:ny - ny // 4, nx // 4:nx - nx // 4] = 100.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def square_with_impulses(shape):
    """the square with 10 % of the sites set to 0 or 255 (exact in fp32)"""
    x = clean_square(shape).copy()
    r = np.random.default_rng(0).random(shape)
    x[r < 0.05] = 0.0
    x[r > 0.95] = 255.0
    x.setflags(write=False)
    return x


def _kw_of(shape):
    return dict(reg_z_over_reg=0.7, reg_time=0.25) if shape[0] > 1 else dict()


def _sigma_of(shape, scheme):
    return 1.0 / (orc.normal_spectral_bound(scheme, shape, **_kw_of(shape)) * TAU_S)


@functools.lru_cache(maxsize=None)
def np_trajectory(shape, scheme, fidelity, n_iter):
    return np_robust(square_with_impulses(shape), n_iter, REG, fidelity, DELTA_S, scheme, _kw_of(shape), TAU_S, _sigma_of(shape, scheme))


def _solver(pytv, shape, dtype, scheme, fidelity, **how):
    how = dict(dict(tau=TAU_S), **how)
    return pytv.solvers.RobustChambollePock(torch.as_tensor(square_with_impulses(shape).astype(dtype)).cuda(), REG, fidelity=fidelity,
                                            delta=DELTA_S if fidelity == "huber" else None, scheme=scheme, **_kw_of(shape), **how)


TRAJ_SHAPES = [(1, 1, 24, 28), (3, 2, 16, 20)]
ROBUST = ("l1", "huber")


# ------------------------------------------------------------------------------------------------
# 7. solver trajectory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fidelity", ROBUST)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp64(shape, scheme, fidelity):
    import pytv
    wx, wloss, _ = np_trajectory(shape, scheme, fidelity, 40)
    cp = _solver(pytv, shape, np.float64, scheme, fidelity)
    assert cp.it == 0 and cp.tau == TAU_S and cp.L2 == orc.normal_spectral_bound(scheme, shape, **_kw_of(shape))
    assert cp.sigma == 1.0 / (cp.L2 * TAU_S)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, fidelity, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-10, atol=0)
    assert float(np.max(np.abs(x - wx))) <= 1e-9 * float(np.max(np.abs(square_with_impulses(shape))))
    assert cp.it == 40
    # run(15); run(25) is run(40) bit for bit
    two = _solver(pytv, shape, np.float64, scheme, fidelity)
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


@pytest.mark.parametrize("fidelity", ROBUST)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_solver_trajectory_fp32(shape, scheme, fidelity):
    """the tolerance tests/test_gpu_cp_accel.py gives fp32 trajectories against the fp64 restatement on the fp32-rounded input (the data are
    0, 100 and 255: exact in fp32): loss rtol 1e-5; result rtol 1e-5, atol 2e-3"""
    import pytv
    wx, wloss, _ = np_trajectory(shape, scheme, fidelity, 40)
    cp = _solver(pytv, shape, np.float32, scheme, fidelity)
    loss = cp.run(40)
    x = cp.result().cpu().numpy()
    print("%s %s %s: loss rel %.3e  max|dx| %.3e" % (scheme, shape, fidelity, np.max(np.abs(loss / wloss - 1.0)), np.max(np.abs(x - wx))))
    np.testing.assert_allclose(loss, wloss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(x, wx, rtol=1e-5, atol=2e-3)


def test_constructor_refuses_bad_steps_and_a_huber_term_without_delta():
    import pytv
    x0 = torch.as_tensor(square_with_impulses((1, 1, 24, 28)).copy()).cuda()
    L2 = 8.0
    with pytest.raises(ValueError, match="tau"):
        pytv.solvers.RobustChambollePock(x0, 1.0, scheme="upwind", tau=1.0, sigma=(1.0 + 1e-9) / L2)
    ok = pytv.solvers.RobustChambollePock(x0, 1.0, scheme="upwind", tau=1.0, sigma=1.0 / L2)
    assert ok.L2 == L2 and ok.fidelity == "l1"
    assert pytv.solvers.RobustChambollePock(x0, 1.0, scheme="upwind", sigma=0.25).tau == 1.0 / (L2 * 0.25)
    both = pytv.solvers.RobustChambollePock(x0, 1.0, scheme="upwind")
    assert both.tau == both.sigma == 1.0 / np.sqrt(L2)
    with pytest.raises(ValueError, match="delta"):
        pytv.solvers.RobustChambollePock(x0, 1.0, fidelity="huber")
    with pytest.raises(ValueError, match="delta"):
        pytv.solvers.RobustChambollePock(x0, 1.0, fidelity="huber", delta=0.0)
    with pytest.raises(ValueError, match="fidelity"):
        pytv.solvers.RobustChambollePock(x0, 1.0, fidelity="poisson")


# ------------------------------------------------------------------------------------------------
# 8. certificate and stopping
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fidelity", ROBUST)
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_residuals_and_run_until(shape, scheme, fidelity):
    """NumPy restatement: every one of the 16 cases meets rel_res = 2e-2 within 100 iterations (relative residual at 100: <= 9.8e-3)"""
    import pytv
    kw, x0 = _kw_of(shape), np.asarray(square_with_impulses(shape))
    cp = _solver(pytv, shape, np.float64, scheme, fidelity)
    done = 0
    for n in (0, 10, 40):
        if n > done:
            cp.run(n - done)
            done = n
        wx, _, wq = np_trajectory(shape, scheme, fidelity, n) if n else (x0, None, np.zeros_like(orc.D(x0, scheme, **kw)))
        want = np_residuals(wx, wq, x0, REG, fidelity, DELTA_S, scheme, kw, TAU_S, _sigma_of(shape, scheme))
        state = [t.clone() for t in (cp.x, cp.x_bar, cp.q)]
        got = cp.residuals()
        print("%s %s %s after %d: %r  restated %r" % (scheme, shape, fidelity, n, got, want))
        assert sorted(got) == ["fid", "q", "total", "tv", "x"] and got["total"] == got["x"] + got["q"]
        for k in ("x", "q", "tv", "fid"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=0, err_msg="%s after %d" % (k, n))
        assert all(torch.equal(a, b) for a, b in zip(state, (cp.x, cp.x_bar, cp.q)))
        if n == 0:
            assert got["x"] == 0.0 and got["fid"] == 0.0 and got["total"] == cp.initial_residual() > 0.0
    r0 = cp.initial_residual()                                          # of the starting pair, whenever it is asked for
    np.testing.assert_allclose(r0, np_residuals(x0, np.zeros_like(orc.D(x0, scheme, **kw)), x0, REG, fidelity, DELTA_S, scheme, kw, TAU_S,
                                                _sigma_of(shape, scheme))["total"], rtol=1e-9)
    cp.reset()
    loss, info = cp.run_until(2e-2, 400, check_every=50)
    print(info)
    assert info["converged"] is True and info["iterations"] in (50, 100) and len(loss) == info["iterations"] == cp.it
    assert info["initial"] == r0 and info["residuals"]["total"] <= 2e-2 ** 2 * r0
    assert info["relative"] == np.sqrt(cp.residuals()["total"] / cp.initial_residual())
    assert sorted(info) == ["converged", "initial", "iterations", "relative", "residuals"]


def test_run_until_on_a_constant_image_returns_at_once():
    import pytv
    cp = pytv.solvers.RobustChambollePock(torch.full((2, 2, 8, 12), 3.0, device="cuda"), 1.0, tau=5.0, reg_time=0.5)
    loss, info = cp.run_until(1e-3, 100)
    assert info["converged"] is True and info["iterations"] == 0 == cp.it and info["initial"] == 0.0 and info["relative"] == 0.0 and len(loss) == 0


# ------------------------------------------------------------------------------------------------
# 9. it does what it is for: impulse noise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("upwind", "hybrid"))
@pytest.mark.parametrize("shape", TRAJ_SHAPES)
def test_tv_l1_removes_impulse_noise_where_the_quadratic_model_does_not(shape, scheme):
    """NumPy figures (this file's restatement), mean absolute error to the clean square after 400 iterations of TV-L1 with reg 1, tau 5:
    upwind 0.03 / 0.35, hybrid 0.56 / 1.94 for the two shapes, against 13.07 / 12.46 of the noisy input and 14.4 - 15.8 of
    1/2 |x - x0|^2 + 25 TV"""
    import pytv
    clean = clean_square(shape)
    noisy = square_with_impulses(shape)
    x0 = torch.as_tensor(noisy.astype(np.float32)).cuda()
    robust = _solver(pytv, shape, np.float32, scheme, "l1")
    robust.run(400, record_loss=False)
    quad = pytv.solvers.ChambollePock(x0, 25.0, scheme=scheme, **_kw_of(shape))
    quad.run(400)
    mae = lambda a: float(np.mean(np.abs(np.asarray(a, dtype=np.float64) - clean)))
    m_noisy, m_l1, m_l2 = mae(noisy), mae(robust.result().cpu().numpy()), mae(quad.result().cpu().numpy())
    print("%s %s: mean abs error noisy %.3f  TV-L1 %.3f  TV-L2 %.3f" % (scheme, shape, m_noisy, m_l1, m_l2))
    assert m_l1 < 0.5 * m_noisy and m_l1 < m_l2


def test_denoise_tv_robust_front_end():
    import pytv
    shape = (1, 1, 24, 28)
    img = square_with_impulses(shape)[0, 0].astype(np.float32)
    vol = torch.as_tensor(img.reshape(shape)).cuda()
    # stops on run_until with its own check_every = 10
    out = pytv.denoise_tv_robust(img, rel_res=2e-2, max_num_iter=100, tau=5.0)
    ref = pytv.solvers.RobustChambollePock(vol, 1.0, fidelity="l1", scheme="upwind", reg_z_over_reg=1.0, tau=5.0)
    _, info = ref.run_until(2e-2, 100, check_every=10)
    print(info)
    assert info["converged"] is True and info["iterations"] % 10 == 0 and info["iterations"] < 100
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == img.shape
    np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # never converges: exactly 40 iterations, the solver's run(40)
    for fidelity, delta in (("l1", None), ("huber", 2.0)):
        out = pytv.denoise_tv_robust(img, 1.0, fidelity, delta, rel_res=0.0, max_num_iter=40, tau=5.0)
        ref = pytv.solvers.RobustChambollePock(vol, 1.0, fidelity=fidelity, delta=delta, scheme="upwind", reg_z_over_reg=1.0, tau=5.0)
        ref.run(40)
        assert ref.it == 40
        np.testing.assert_array_equal(out, ref.result().cpu().numpy().reshape(img.shape))
    # torch in -> device tensor out; 3-D input; 4-D refused
    t = pytv.denoise_tv_robust(vol[0, 0], rel_res=0.0, max_num_iter=40, tau=5.0)
    assert isinstance(t, torch.Tensor) and t.is_cuda and torch.equal(t.cpu(), torch.as_tensor(pytv.denoise_tv_robust(img, rel_res=0.0, max_num_iter=40, tau=5.0)))
    stack = np.stack([img, img, img])
    assert pytv.denoise_tv_robust(stack, rel_res=0.0, max_num_iter=5, tau=5.0).shape == stack.shape
    with pytest.raises(ValueError, match="2-D or 3-D"):
        pytv.denoise_tv_robust(np.zeros((1, 1, 8, 8), dtype=np.float32))
